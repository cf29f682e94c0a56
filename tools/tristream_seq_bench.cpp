// tristream_seq_bench.cpp -- the sequential baseline of tools/tristream_bench.py: the definition of
// the triangle streams' fold (csrc/gs_tristream_seq.hpp, trs_fold_seq: ordered maps, one arrival
// after the other) on one core. Reads n arrivals (n int64 sources, then targets) from a binary
// file, folds them in order in batches of `batch` arrivals, mode `count`, into one state, dropping
// each batch's rows and records once it is folded, and prints one JSON line with the seconds of
// the folds alone.
// Usage: tristream_seq_bench <edges file> <n> <batch>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gs_tristream_seq.hpp"

int main(int argc, char** argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: tristream_seq_bench <edges file> <n> <batch>\n");
    return 2;
  }
  const size_t n = (size_t)std::strtoull(argv[2], nullptr, 10);
  const size_t batch = (size_t)std::strtoull(argv[3], nullptr, 10);
  std::vector<int64_t> src(n), dst(n);
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f || batch == 0 || std::fread(src.data(), 8, n, f) != n || std::fread(dst.data(), 8, n, f) != n) {
    std::fprintf(stderr, "cannot read %zu arrivals from %s\n", n, argv[1]);
    return 2;
  }
  std::fclose(f);
  gs::TrsState st;
  std::vector<gs::TrsRow> rows;
  std::vector<gs::TrsRec> recs;
  unsigned long long records = 0;
  double sec = 0;
  for (size_t at = 0; at < n; at += batch) {
    const size_t len = n - at < batch ? n - at : batch;
    rows.clear();
    recs.clear();
    const auto t0 = std::chrono::steady_clock::now();
    gs::trs_fold_seq(st, src.data() + at, dst.data() + at, len, gs::kTrsCount, &rows, &recs);
    sec += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    records += recs.size();
  }
  std::printf("{\"arrivals\": %zu, \"seconds\": %.6f, \"records\": %llu, \"triangles\": %lld, \"pairs\": %zu}\n", n, sec,
              records, (long long)st.total, st.first.size());
  return 0;
}
