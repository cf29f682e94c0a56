// spanner_seq_bench.cpp -- the sequential baseline of tools/spanner_bench.py: the plain
// restatement of Spanner.UpdateLocal (csrc/gs_spanner_seq.hpp, SpannerSeq::fold) on one core.
// Reads n edges (n int64 sources, then n int64 targets) from a binary file, folds them in arrival
// order, writes the n accepted bytes to a second file and prints one JSON line with the seconds
// of the fold alone. Built by the tool with the host compiler.
// Usage: spanner_seq_bench <edges file> <n> <k> <accepted file>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gs_spanner_seq.hpp"

int main(int argc, char** argv) {
  if (argc != 5) {
    std::fprintf(stderr, "usage: spanner_seq_bench <edges file> <n> <k> <accepted file>\n");
    return 2;
  }
  const size_t n = (size_t)std::strtoull(argv[2], nullptr, 10);
  const int k = std::atoi(argv[3]);
  std::vector<int64_t> src(n), dst(n);
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(src.data(), 8, n, f) != n || std::fread(dst.data(), 8, n, f) != n) {
    std::fprintf(stderr, "cannot read %zu edges from %s\n", n, argv[1]);
    return 2;
  }
  std::fclose(f);
  std::vector<uint8_t> acc(n);
  gs::SpannerSeq g(k);
  const auto t0 = std::chrono::steady_clock::now();
  const uint64_t kept = g.fold(src.data(), dst.data(), n, acc.data());
  const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  std::FILE* o = std::fopen(argv[4], "wb");
  if (!o || std::fwrite(acc.data(), 1, n, o) != n) {
    std::fprintf(stderr, "cannot write %s\n", argv[4]);
    return 2;
  }
  std::fclose(o);
  std::printf("{\"edges\": %zu, \"k\": %d, \"seconds\": %.6f, \"accepted\": %llu, \"vertices\": %llu}\n", n, k, sec,
              (unsigned long long)kept, (unsigned long long)g.vertices());
  return 0;
}
