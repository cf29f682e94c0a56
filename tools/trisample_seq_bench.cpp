// The sequential definition of the sampling triangle estimate (csrc/gs_trisample_seq.hpp
// ts_fold_seq) on one core, for tools/trisample_bench.py: reads n arrivals (n int64 sources, then
// n int64 targets) from a file, folds them into `samples` instances, writes the rows (int32
// triples) to a file and prints one JSON line with the seconds of the fold.
// Usage: trisample_seq_bench <arrivals.bin> <n> <samples> <vertices> <rows.bin>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gs_trisample_seq.hpp"

int main(int argc, char** argv) {
  if (argc != 6) {
    std::fprintf(stderr, "Usage: trisample_seq_bench <arrivals.bin> <n> <samples> <vertices> <rows.bin>\n");
    return 1;
  }
  const size_t n = std::strtoull(argv[2], nullptr, 10);
  const uint32_t samples = (uint32_t)std::strtoul(argv[3], nullptr, 10);
  const int32_t vertices = (int32_t)std::strtol(argv[4], nullptr, 10);
  std::vector<int64_t> src(n), dst(n);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(src.data(), 8, n, f) != n || std::fread(dst.data(), 8, n, f) != n) {
    std::fprintf(stderr, "cannot read %zu arrivals from %s\n", n, argv[1]);
    return 1;
  }
  std::fclose(f);
  gs::TsSeq q(samples, vertices, gs::kTsDefaultSeed, 0);
  std::vector<gs::TsRow> rows;
  const auto t0 = std::chrono::steady_clock::now();
  gs::ts_fold_seq(q, src.data(), dst.data(), n, &rows);
  const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  FILE* o = std::fopen(argv[5], "wb");
  if (!o || (rows.size() && std::fwrite(rows.data(), sizeof(gs::TsRow), rows.size(), o) != rows.size())) {
    std::fprintf(stderr, "cannot write %s\n", argv[5]);
    return 1;
  }
  std::fclose(o);
  std::printf("{\"arrivals\": %zu, \"samples\": %u, \"seconds\": %.6f, \"rows\": %zu, \"beta_sum\": %d, \"coins\": %llu}\n", n,
              samples, sec, rows.size(), q.beta_sum, (unsigned long long)q.coins);
  return 0;
}
