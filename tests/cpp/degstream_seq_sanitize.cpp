// Stand-alone check of csrc/gs_degstream_seq.hpp under the address and undefined-behaviour
// sanitizers (built and run by tests/test_degstream_seq.py; no device):
//   * ds_fold_seq against a brute-force restatement that keeps plain maps and branches on the
//     cases of the rule instead of composing maps;
//   * ds_fold_parts (stable sort, tile reduce, aggregate scan, apply with deferred tails,
//     compaction, second sort, seeded sum) against ds_fold_seq at every tile size from 1 up, on
//     random streams with deletions and self-loops, in all three directions;
//   * the same parts with the stream cut at every position;
//   * the pins of tests/golden/degree_pins.json, handed over as a text file (argv[1]: sections
//     "#name count" followed by count lines): both distribution sequences in order, the three
//     get_*_degrees sets as sorted lines.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "gs_degstream_seq.hpp"

namespace {

int failures = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      ++failures;                                                \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      if (failures > 20) exit(1);                                \
    }                                                            \
  } while (0)

struct Rng {
  uint64_t s;
  uint64_t next() {
    s += 0x9E3779B97F4A7C15ull;
    uint64_t z = s;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  uint64_t below(uint64_t n) { return next() % n; }
};

struct Stream {
  std::vector<int64_t> src, dst;
  std::vector<uint8_t> del;
};

Stream random_stream(Rng& r, size_t n, uint64_t vertices, unsigned del_percent) {
  Stream s;
  for (size_t i = 0; i < n; ++i) {
    int64_t a = (int64_t)r.below(vertices), b = (int64_t)r.below(vertices);
    if (r.below(8) == 0) b = a;  // self-loops
    if (r.below(16) == 0) a = INT64_MIN;
    if (r.below(16) == 0) b = INT64_MAX;
    s.src.push_back(a);
    s.dst.push_back(b);
    s.del.push_back((uint8_t)(r.below(100) < del_percent ? 1 | (r.below(2) << 1) : (r.below(2) << 1)));  // bit 0 alone is read
  }
  return s;
}

// the rule once more, without the map algebra
void brute(std::map<int64_t, long>& deg, std::map<long, long>& cnt, const Stream& s, int dir,
           std::vector<gs::DsRow>* rows, std::vector<gs::DsRec>* recs) {
  uint32_t o = 0;
  for (size_t i = 0; i < s.src.size(); ++i) {
    const bool minus = (s.del[i] & 1) != 0;
    for (int side = 0; side < 2; ++side) {
      if (side == 0 && dir == gs::kDsIn) continue;
      if (side == 1 && dir == gs::kDsOut) continue;
      const int64_t v = side ? s.dst[i] : s.src[i];
      const long old_d = deg.count(v) ? deg[v] : 0;
      long new_d;
      if (old_d == 0 && minus) {
        new_d = 0;  // an absent vertex ignores a deletion
      } else {
        new_d = old_d + (minus ? -1 : 1);
        if (new_d <= 0) {
          new_d = 0;
          deg.erase(v);
        } else {
          deg[v] = new_d;
        }
      }
      rows->push_back(gs::DsRow{v, (uint32_t)old_d, (uint32_t)new_d});
      if (old_d > 0) {
        if (new_d > 0) recs->push_back(gs::DsRec{o, (uint32_t)new_d, (uint32_t)++cnt[new_d]});
        recs->push_back(gs::DsRec{o, (uint32_t)old_d, (uint32_t)--cnt[old_d]});
        CHECK(cnt[old_d] >= 0);
      } else if (!minus) {
        recs->push_back(gs::DsRec{o, 1u, (uint32_t)++cnt[1]});
      }
      ++o;
    }
  }
}

void check_algebra() {
  // composition against application, identity, and the clamp carried through a composition
  Rng r{7};
  for (int it = 0; it < 20000; ++it) {
    gs::DsPair p = gs::ds_identity();
    int64_t x = (int64_t)r.below(6), y = x;
    const int len = (int)r.below(12);
    for (int k = 0; k < len; ++k) {
      const gs::DsPair e = gs::ds_element(r.below(2) ? 1 : -1, r.below(4) != 0);
      p = gs::ds_compose(p, e);
      y = gs::ds_apply(e, y);
    }
    CHECK(gs::ds_apply(p, x) == y);
  }
  CHECK(gs::ds_apply(gs::ds_identity(), 5) == 5);
  const gs::DsSeg h = gs::ds_seg_element(1, true, true), t = gs::ds_seg_element(-1, true, false);
  CHECK(gs::ds_seg_combine(t, h).head == 1 && gs::ds_seg_combine(t, h).a == 1);
  CHECK(gs::ds_seg_combine(h, t).head == 1 && gs::ds_seg_combine(h, t).a == 0 && gs::ds_seg_combine(h, t).b == 0);
  CHECK(gs::ds_seg_combine(gs::ds_seg_identity(), t).head == 0);
  for (uint32_t o = 0; o < 4; ++o)
    for (uint32_t n = 0; n < 4; ++n) CHECK(gs::ds_record_count(o, n, 1) <= 2);
  CHECK(gs::ds_record_count(0, 0, -1) == 0 && gs::ds_record_count(0, 1, 1) == 1 && gs::ds_record_count(1, 0, -1) == 1 &&
        gs::ds_record_count(2, 1, -1) == 2 && gs::ds_record_count(1, 2, 1) == 2);
  CHECK(gs::ds_count_cap(0, 4) == 4 && gs::ds_count_cap(3, 4) == 4 && gs::ds_count_cap(4, 4) == 8);
  CHECK(gs::ds_occurrences(5, gs::kDsAll) == 10 && gs::ds_occurrences(5, gs::kDsIn) == 5);
}

void check_random() {
  Rng r{0x5EED};
  size_t streams = 0;
  for (int it = 0; it < 60; ++it) {
    const size_t n = 1 + r.below(40);
    const Stream s = random_stream(r, n, 1 + r.below(6), (unsigned)r.below(60));
    for (int dir = 0; dir < gs::kDsDirections; ++dir) {
      std::vector<gs::DsRow> rows_b, rows_s;
      std::vector<gs::DsRec> recs_b, recs_s;
      std::map<int64_t, long> bd;
      std::map<long, long> bc;
      brute(bd, bc, s, dir, &rows_b, &recs_b);
      gs::DsState seq;
      gs::ds_fold_seq(seq, s.src.data(), s.dst.data(), s.del.data(), n, dir, &rows_s, &recs_s);
      CHECK(rows_b == rows_s);
      CHECK(recs_b == recs_s);
      const uint64_t occs = gs::ds_occurrences(n, dir);
      // every tile size from 1 up to past the whole fold
      for (uint32_t tile = 1; tile <= occs + 1; ++tile) {
        gs::DsState st;
        std::vector<gs::DsRow> rows_p;
        std::vector<gs::DsRec> recs_p;
        const uint64_t crossed = gs::ds_fold_parts(st, s.src.data(), s.dst.data(), s.del.data(), n, dir, tile, &rows_p, &recs_p);
        CHECK(rows_p == rows_s);
        CHECK(recs_p == recs_s);
        CHECK(st == seq);
        if (tile > 2 * occs) CHECK(crossed == 0);
      }
      // the stream cut at every position, with a tile that is no divisor of anything
      for (size_t cut = 0; cut <= n; ++cut) {
        gs::DsState st;
        std::vector<gs::DsRow> rows_p;
        std::vector<gs::DsRec> recs_p, part;
        gs::ds_fold_parts(st, s.src.data(), s.dst.data(), s.del.data(), cut, dir, 3, &rows_p, &recs_p);
        gs::ds_fold_parts(st, s.src.data() + cut, s.dst.data() + cut, s.del.data() + cut, n - cut, dir, 3, &rows_p, &part);
        for (gs::DsRec x : part) {  // the occurrence index counts inside a fold
          x.occ += (uint32_t)gs::ds_occurrences(cut, dir);
          recs_p.push_back(x);
        }
        CHECK(rows_p == rows_s);
        CHECK(recs_p == recs_s);
        CHECK(st == seq);
      }
      ++streams;
    }
  }
  // null deletions: every edge an addition
  const Stream s = random_stream(r, 50, 5, 0);
  std::vector<gs::DsRow> ra, rb;
  std::vector<gs::DsRec> ca, cb;
  gs::DsState a, b;
  gs::ds_fold_seq(a, s.src.data(), s.dst.data(), nullptr, 50, gs::kDsAll, &ra, &ca);
  gs::ds_fold_parts(b, s.src.data(), s.dst.data(), nullptr, 50, gs::kDsAll, 7, &rb, &cb);
  CHECK(ra == rb && ca == cb && a == b);
  for (const gs::DsRow& x : ra) CHECK(x.new_d == x.old_d + 1);
  printf("random streams: %zu\n", streams);
}

std::map<std::string, std::vector<std::string>> read_pins(const char* path) {
  std::map<std::string, std::vector<std::string>> out;
  std::ifstream f(path);
  std::string line;
  while (std::getline(f, line)) {
    if (line.empty() || line[0] != '#') continue;
    std::istringstream h(line.substr(1));
    std::string name;
    size_t count = 0;
    h >> name >> count;
    for (size_t i = 0; i < count && std::getline(f, line); ++i) out[name].push_back(line);
  }
  return out;
}

Stream parse_events(const std::vector<std::string>& lines) {
  Stream s;
  for (const std::string& l : lines) {
    std::istringstream in(l);
    long long a, b;
    std::string op;
    in >> a >> b >> op;
    s.src.push_back(a);
    s.dst.push_back(b);
    s.del.push_back(op == "-" ? 1 : 0);
  }
  return s;
}

void check_pins(const char* path) {
  auto pins = read_pins(path);
  CHECK(pins["sample_edges"].size() == 7);
  const Stream sample = parse_events(pins["sample_edges"]);  // "src trg +"
  const char* names[3] = {"get_degrees", "get_in_degrees", "get_out_degrees"};
  const int dirs[3] = {gs::kDsAll, gs::kDsIn, gs::kDsOut};
  for (int k = 0; k < 3; ++k) {
    for (uint32_t tile : {1u, 2u, 5u, 64u}) {
      gs::DsState st;
      std::vector<gs::DsRow> rows;
      std::vector<gs::DsRec> recs;
      gs::ds_fold_parts(st, sample.src.data(), sample.dst.data(), nullptr, sample.src.size(), dirs[k], tile, &rows, &recs);
      std::vector<std::string> got;
      for (const gs::DsRow& r : rows) got.push_back(std::to_string(r.vertex) + "," + std::to_string(r.new_d));
      std::sort(got.begin(), got.end());
      std::vector<std::string> want = pins[names[k]];
      std::sort(want.begin(), want.end());
      CHECK(!want.empty() && got == want);
    }
  }
  const char* data[2] = {"degrees_data", "degrees_data_zero"};
  const char* result[2] = {"degrees_result", "degrees_result_zero"};
  for (int k = 0; k < 2; ++k) {
    const Stream s = parse_events(pins[data[k]]);
    CHECK(s.src.size() >= 6);
    for (int parts = 0; parts < 2; ++parts) {
      gs::DsState st;
      std::vector<gs::DsRow> rows;
      std::vector<gs::DsRec> recs;
      if (parts)
        gs::ds_fold_parts(st, s.src.data(), s.dst.data(), s.del.data(), s.src.size(), gs::kDsAll, 4, &rows, &recs);
      else
        gs::ds_fold_seq(st, s.src.data(), s.dst.data(), s.del.data(), s.src.size(), gs::kDsAll, &rows, &recs);
      std::vector<std::string> got;
      for (const gs::DsRec& r : recs) got.push_back("(" + std::to_string(r.degree) + "," + std::to_string(r.count) + ")");
      CHECK(got == pins[result[k]]);
    }
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) {
    printf("usage: %s pins.txt\n", argv[0]);
    return 2;
  }
  check_algebra();
  check_random();
  check_pins(argv[1]);
  if (failures) {
    printf("%d checks failed\n", failures);
    return 1;
  }
  printf("all checks passed\n");
  return 0;
}
