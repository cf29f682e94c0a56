// matching_seq_bench.cpp -- the sequential baseline of tools/matching_bench.py: the definition
// of the weighted matching fold (csrc/gs_matching_seq.hpp, mt_fold_seq) on one core. Reads n
// arrivals (n int64 sources, then targets, then values) from a binary file, folds them in order,
// writes the n accepted bytes and then the event rows (five int64 each: arrival, type, src, dst,
// value) to a second file and prints one JSON line with the seconds of the fold alone, timed
// without the event rows (a second, untimed fold collects them).
// Usage: matching_seq_bench <arrivals file> <n> <output file>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gs_matching_seq.hpp"

int main(int argc, char** argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: matching_seq_bench <arrivals file> <n> <output file>\n");
    return 2;
  }
  const size_t n = (size_t)std::strtoull(argv[2], nullptr, 10);
  std::vector<int64_t> src(n), dst(n), val(n);
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(src.data(), 8, n, f) != n || std::fread(dst.data(), 8, n, f) != n ||
      std::fread(val.data(), 8, n, f) != n) {
    std::fprintf(stderr, "cannot read %zu arrivals from %s\n", n, argv[1]);
    return 2;
  }
  std::fclose(f);
  std::vector<uint8_t> acc(n);
  uint64_t kept = 0;
  double sec = 0;
  {
    gs::MatchingSeq m;
    const auto t0 = std::chrono::steady_clock::now();
    kept = gs::mt_fold_seq(m, src.data(), dst.data(), val.data(), n, acc.data(), nullptr);
    sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  }
  gs::MatchingSeq m;
  std::vector<gs::MtEvent> ev;
  gs::mt_fold_seq(m, src.data(), dst.data(), val.data(), n, nullptr, &ev);
  std::vector<int64_t> rows;
  rows.reserve(5 * ev.size());
  for (const gs::MtEvent& e : ev) {
    rows.push_back((int64_t)e.arrival);
    rows.push_back((int64_t)e.type);
    rows.push_back(e.src);
    rows.push_back(e.dst);
    rows.push_back(e.val);
  }
  std::FILE* o = std::fopen(argv[3], "wb");
  if (!o || std::fwrite(acc.data(), 1, n, o) != n || std::fwrite(rows.data(), 8, rows.size(), o) != rows.size()) {
    std::fprintf(stderr, "cannot write %s\n", argv[3]);
    return 2;
  }
  std::fclose(o);
  std::printf("{\"edges\": %zu, \"seconds\": %.6f, \"accepted\": %llu, \"events\": %zu, \"matching\": %llu}\n", n, sec,
              (unsigned long long)kept, ev.size(), (unsigned long long)m.edges());
  return 0;
}
