// degstream_seq_bench.cpp -- the sequential baseline of tools/degstream_bench.py: the definition
// of the degree streams' fold (csrc/gs_degstream_seq.hpp, ds_fold_seq: ordered maps, one
// occurrence after the other) on one core. Reads n edges (n int64 sources, then targets, then n
// deletion bytes) from a binary file, folds them in order in batches of `batch` edges, direction
// ALL, into one state, dropping each batch's rows and records once it is folded, and prints one
// JSON line with the seconds of the folds alone.
// Usage: degstream_seq_bench <edges file> <n> <batch>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gs_degstream_seq.hpp"

int main(int argc, char** argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: degstream_seq_bench <edges file> <n> <batch>\n");
    return 2;
  }
  const size_t n = (size_t)std::strtoull(argv[2], nullptr, 10);
  const size_t batch = (size_t)std::strtoull(argv[3], nullptr, 10);
  std::vector<int64_t> src(n), dst(n);
  std::vector<uint8_t> del(n);
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f || batch == 0 || std::fread(src.data(), 8, n, f) != n || std::fread(dst.data(), 8, n, f) != n ||
      std::fread(del.data(), 1, n, f) != n) {
    std::fprintf(stderr, "cannot read %zu edges from %s\n", n, argv[1]);
    return 2;
  }
  std::fclose(f);
  gs::DsState st;
  std::vector<gs::DsRow> rows;
  std::vector<gs::DsRec> recs;
  unsigned long long occs = 0, records = 0;
  double sec = 0;
  for (size_t at = 0; at < n; at += batch) {
    const size_t len = n - at < batch ? n - at : batch;
    rows.clear();
    recs.clear();
    const auto t0 = std::chrono::steady_clock::now();
    gs::ds_fold_seq(st, src.data() + at, dst.data() + at, del.data() + at, len, gs::kDsAll, &rows, &recs);
    sec += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    occs += rows.size();
    records += recs.size();
  }
  std::printf("{\"edges\": %zu, \"seconds\": %.6f, \"occurrences\": %llu, \"records\": %llu, \"vertices\": %zu}\n", n, sec,
              occs, records, st.degree.size());
  return 0;
}
