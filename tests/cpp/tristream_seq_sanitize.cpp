// tristream_seq_sanitize.cpp -- the triangle streams' rules header (csrc/gs_tristream_seq.hpp) in a
// stand-alone host program, built with -fsanitize=address,undefined by tests/test_tristream_seq.py:
//   * trs_fold_seq against a literal restatement of the reference's three operators
//     (buildNeighborhood(false) + ProjectCanonicalEdges, IntersectNeighborhoods,
//     SumAndEmitCounters of example/ExactTriangleCount.java) made of std::map and std::set;
//   * trs_fold_parts, the kernels' decomposition, against trs_fold_seq at every tile size 1..9 and
//     every two-way cut of streams of up to 40 arrivals, in both repeat modes;
//   * the pins (tests/golden/tristream_pins.json, handed over as text: argv[1]);
//   * the int64 extremes, the empty fold, a fold of loops only, the record limit.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <fstream>
#include <limits>
#include <map>
#include <set>
#include <sstream>
#include <string>
#include <utility>
#include <vector>

#include "gs_tristream_seq.hpp"

namespace {

int failures = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      ++failures;                                                \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
    }                                                            \
  } while (0)

typedef std::pair<int64_t, int64_t> Tuple;

// ---- the reference, literally (ExactTriangleCount.java:52-56): loop-free streams only
struct Reference {
  std::map<int64_t, std::set<int64_t>> hood;  // buildNeighborhood(false)
  std::map<int64_t, int64_t> counts;          // SumAndEmitCounters
  void sum_and_emit(int64_t k, int64_t v, std::vector<Tuple>* out) {
    const auto it = counts.find(k);
    if (it != counts.end()) {
      it->second += v;
      out->push_back(Tuple(k, it->second));
    } else {
      counts[k] = v;
      out->push_back(Tuple(k, v));
    }
  }
  void edge(int64_t s, int64_t d, std::vector<Tuple>* out) {
    hood[s].insert(d);
    hood[d].insert(s);
    // the two tuples of the edge, keyed by the canonical pair; the second one intersects
    const int64_t f0 = s < d ? s : d, f1 = s < d ? d : s;
    const std::set<int64_t> t1 = hood[s], t2 = hood[d];
    std::vector<Tuple> mid;
    int counter = 0;
    const std::set<int64_t>& walk = t1.size() < t2.size() ? t1 : t2;
    const std::set<int64_t>& look = t1.size() < t2.size() ? t2 : t1;
    for (const int64_t i : walk)
      if (look.count(i)) {
        ++counter;
        mid.push_back(Tuple(i, 1));
      }
    if (counter > 0) {
      mid.push_back(Tuple(f0, counter));
      mid.push_back(Tuple(f1, counter));
      mid.push_back(Tuple(-1, counter));
    }
    for (const Tuple& t : mid) sum_and_emit(t.first, t.second, out);
  }
};

// the definition's rows and records as the reference's tuple sequence
std::vector<Tuple> as_tuples(const std::vector<gs::TrsRow>& rows, const std::vector<gs::TrsRec>& recs) {
  std::vector<Tuple> out;
  size_t r = 0;
  for (size_t a = 0; a < rows.size(); ++a) {
    for (; r < recs.size() && recs[r].arrival == a; ++r) out.push_back(Tuple(recs[r].vertex, recs[r].count));
    if (rows[a].closed) out.push_back(Tuple(-1, rows[a].total));
  }
  return out;
}

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rng() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}

void random_stream(size_t n, int64_t vertices, bool loops, std::vector<int64_t>* s, std::vector<int64_t>* d) {
  s->resize(n);
  d->resize(n);
  for (size_t i = 0; i < n; ++i) {
    (*s)[i] = (int64_t)(rng() % (uint64_t)vertices);
    (*d)[i] = (int64_t)(rng() % (uint64_t)vertices);
    if (!loops && (*s)[i] == (*d)[i]) (*d)[i] = ((*s)[i] + 1) % vertices;
  }
}

void check_reference() {
  for (int round = 0; round < 40; ++round) {
    std::vector<int64_t> s, d;
    random_stream(20 + round * 3, 5 + round % 7, false, &s, &d);
    Reference ref;
    std::vector<Tuple> want;
    for (size_t i = 0; i < s.size(); ++i) ref.edge(s[i], d[i], &want);
    gs::TrsState st;
    std::vector<gs::TrsRow> rows;
    std::vector<gs::TrsRec> recs;
    // in folds of 7: the arrival index restarts with every fold
    std::vector<Tuple> got;
    for (size_t at = 0; at < s.size(); at += 7) {
      rows.clear();
      recs.clear();
      gs::trs_fold_seq(st, s.data() + at, d.data() + at, std::min<size_t>(7, s.size() - at), gs::kTrsCount, &rows, &recs);
      const std::vector<Tuple> t = as_tuples(rows, recs);
      got.insert(got.end(), t.begin(), t.end());
    }
    CHECK(got == want);
    CHECK(st.arrivals == s.size());
  }
  puts("ok trs_fold_seq == the reference's operators (count mode, loop-free)");
}

void check_parts() {
  uint64_t crossed_any = 0, runs = 0;
  for (int round = 0; round < 24; ++round) {
    const size_t n = round < 4 ? (size_t)round : 8 + (size_t)(rng() % 33);  // up to 40
    std::vector<int64_t> s, d;
    random_stream(n, 4 + round % 6, true, &s, &d);
    for (int mode = 0; mode < gs::kTrsModes; ++mode) {
      gs::TrsState whole;
      std::vector<gs::TrsRow> wr;
      std::vector<gs::TrsRec> wc;
      gs::trs_fold_seq(whole, s.data(), d.data(), n, mode, &wr, &wc);
      for (uint32_t tile = 1; tile <= 9; ++tile)
        for (size_t cut = 0; cut <= n; ++cut) {
          gs::TrsState st;
          std::vector<gs::TrsRow> r1, r2;
          std::vector<gs::TrsRec> c1, c2;
          const uint64_t x1 = gs::trs_fold_parts(st, s.data(), d.data(), cut, mode, tile, ~0ull >> 1, &r1, &c1);
          const uint64_t x2 = gs::trs_fold_parts(st, s.data() + cut, d.data() + cut, n - cut, mode, tile, ~0ull >> 1, &r2, &c2);
          CHECK(x1 != ~0ull && x2 != ~0ull);
          crossed_any += x1 + x2;
          ++runs;
          // the second fold's arrival indices follow the cut
          for (gs::TrsRec& r : c2) r.arrival += (uint32_t)cut;
          r1.insert(r1.end(), r2.begin(), r2.end());
          c1.insert(c1.end(), c2.begin(), c2.end());
          CHECK(r1 == wr);
          CHECK(c1 == wc);
          CHECK(st == whole);
        }
    }
  }
  CHECK(crossed_any > 0);  // segments did cross tiles
  printf("ok trs_fold_parts == trs_fold_seq (%llu runs, tiles 1..9, every cut, both modes)\n", (unsigned long long)runs);
}

void check_modes_and_limits() {
  // a repeated closing edge: counted again under `count`, nothing under `ignore`
  const int64_t s[] = {1, 2, 1, 1, 3, 3}, d[] = {2, 3, 3, 3, 1, 3};
  for (int mode = 0; mode < gs::kTrsModes; ++mode) {
    gs::TrsState st;
    std::vector<gs::TrsRow> rows;
    std::vector<gs::TrsRec> recs;
    gs::trs_fold_seq(st, s, d, 6, mode, &rows, &recs);
    CHECK(rows.size() == 6 && rows[2].closed == 1 && rows[5].closed == 0);
    CHECK(rows[3].closed == (mode == gs::kTrsCount ? 1u : 0u) && rows[4].closed == rows[3].closed);
    CHECK(st.total == (mode == gs::kTrsCount ? 3 : 1));
    CHECK(recs.size() == (mode == gs::kTrsCount ? 9u : 3u));
    CHECK(st.first.size() == 3 && st.arrivals == 6);
  }
  // the int64 extremes and -1 as vertices; the order of w is signed
  const int64_t lo = std::numeric_limits<int64_t>::min(), hi = std::numeric_limits<int64_t>::max();
  const int64_t es[] = {lo, hi, -1, 7, lo, 7, hi}, ed[] = {7, 7, 7, 0, hi, hi, 0};
  // pairs: lo-7, hi-7, -1-7, 7-0, then lo-hi closes w = 7; 7-hi is a repeat; hi-0 closes w = 7
  for (uint32_t tile = 1; tile <= 3; ++tile) {
    gs::TrsState a, b;
    std::vector<gs::TrsRow> ra, rb;
    std::vector<gs::TrsRec> ca, cb;
    gs::trs_fold_seq(a, es, ed, 7, gs::kTrsCount, &ra, &ca);
    CHECK(gs::trs_fold_parts(b, es, ed, 7, gs::kTrsCount, tile, 1000, &rb, &cb) != ~0ull);
    CHECK(ra == rb && ca == cb && a == b);
    CHECK(ra[4].closed == 1 && ca.size() >= 3 && ca[0].vertex == 7 && ca[1].vertex == lo && ca[2].vertex == hi);
  }
  {
    // two common neighbours -1 and 5 of lo and hi: -1 first
    const int64_t s2[] = {lo, lo, hi, hi, lo}, d2[] = {5, -1, 5, -1, hi};
    gs::TrsState a;
    std::vector<gs::TrsRow> ra;
    std::vector<gs::TrsRec> ca;
    gs::trs_fold_seq(a, s2, d2, 5, gs::kTrsCount, &ra, &ca);
    CHECK(ca.size() == 4 && ca[0].vertex == -1 && ca[1].vertex == 5 && ca[2].vertex == lo && ca[3].vertex == hi);
    CHECK(ca[2].count == 2 && ca[3].count == 2 && a.total == 2);
  }
  // the empty fold and a fold of loops only
  {
    gs::TrsState a, b;
    std::vector<gs::TrsRow> ra, rb;
    std::vector<gs::TrsRec> ca, cb;
    gs::trs_fold_seq(a, nullptr, nullptr, 0, gs::kTrsCount, &ra, &ca);
    CHECK(gs::trs_fold_parts(b, nullptr, nullptr, 0, gs::kTrsCount, 4, 10, &rb, &cb) == 0);
    CHECK(ra.empty() && rb.empty() && a == b && a.arrivals == 0);
    const int64_t l[] = {3, 3, 9};
    gs::trs_fold_seq(a, l, l, 3, gs::kTrsCount, &ra, &ca);
    CHECK(gs::trs_fold_parts(b, l, l, 3, gs::kTrsCount, 2, 10, &rb, &cb) == 0);
    CHECK(ra.size() == 3 && ra == rb && ca.empty() && cb.empty() && a == b && a.arrivals == 3 && a.first.empty());
  }
  // the record limit: nothing changes, and the two halves give the same stream
  {
    const int64_t s3[] = {1, 2, 1, 4, 4, 1}, d3[] = {2, 3, 3, 1, 2, 2};
    gs::TrsState a, b;
    std::vector<gs::TrsRow> ra, rb;
    std::vector<gs::TrsRec> ca, cb;
    gs::trs_fold_seq(a, s3, d3, 6, gs::kTrsCount, &ra, &ca);
    CHECK(ca.size() > 7);
    CHECK(gs::trs_fold_parts(b, s3, d3, 6, gs::kTrsCount, 4, 7, &rb, &cb) == ~0ull);
    CHECK(rb.empty() && cb.empty() && b == gs::TrsState());
    CHECK(gs::trs_fold_parts(b, s3, d3, 3, gs::kTrsCount, 4, 7, &rb, &cb) != ~0ull);
    CHECK(gs::trs_fold_parts(b, s3 + 3, d3 + 3, 3, gs::kTrsCount, 4, 7, &rb, &cb) != ~0ull);
    CHECK(rb == ra && a == b && cb.size() == ca.size());
  }
  puts("ok modes, extremes, empty and loop folds, the record limit");
}

// ---- the pins: '#name count' and then count lines of integers
std::map<std::string, std::vector<std::vector<int64_t>>> read_pins(const char* path) {
  std::map<std::string, std::vector<std::vector<int64_t>>> out;
  std::ifstream f(path);
  std::string line, name;
  while (std::getline(f, line)) {
    if (line.empty()) continue;
    if (line[0] == '#') {
      std::istringstream h(line.substr(1));
      h >> name;
      out[name];
      continue;
    }
    std::istringstream l(line);
    std::vector<int64_t> row;
    long long x;
    while (l >> x) row.push_back((int64_t)x);
    out[name].push_back(row);
  }
  return out;
}

void run_stream(const std::vector<std::vector<int64_t>>& edges, std::vector<gs::TrsRow>* rows, std::vector<gs::TrsRec>* recs,
                bool parts) {
  std::vector<int64_t> s, d;
  for (const auto& e : edges) {
    s.push_back(e.at(0));
    d.push_back(e.at(1));
  }
  gs::TrsState st;
  if (parts)
    CHECK(gs::trs_fold_parts(st, s.data(), d.data(), s.size(), gs::kTrsCount, 3, 1000, rows, recs) != ~0ull);
  else
    gs::trs_fold_seq(st, s.data(), d.data(), s.size(), gs::kTrsCount, rows, recs);
}

void check_pins(const char* path) {
  auto pins = read_pins(path);
  CHECK(pins.count("builtin") && pins.count("derived_tuples") && pins.count("counts_in") && pins.count("counts_out"));
  for (int parts = 0; parts < 2; ++parts) {
    for (int k = 0; k < 2; ++k) {
      const std::string id = std::to_string(k);
      std::vector<gs::TrsRow> rows;
      std::vector<gs::TrsRec> recs;
      run_stream(pins["stream_" + id], &rows, &recs, parts != 0);
      const auto& want = pins["records_" + id];
      CHECK(recs.size() == want.size());
      for (size_t i = 0; i < recs.size() && i < want.size(); ++i) {
        CHECK(recs[i].vertex == want[i].at(0) && recs[i].count == want[i].at(1));
        CHECK(recs[i].arrival + 1 == rows.size());  // the last arrival alone closes
      }
      CHECK(!rows.empty() && rows.back().total == pins["total_" + id].at(0).at(0));
      // the test's five tuples are the records plus (-1, total), in any order
      std::multiset<Tuple> a, b;
      for (const Tuple& t : as_tuples(rows, recs)) a.insert(t);
      for (const auto& t : pins["tuples_" + id]) b.insert(Tuple(t.at(0), t.at(1)));
      CHECK(a == b);
    }
    std::vector<gs::TrsRow> rows;
    std::vector<gs::TrsRec> recs;
    run_stream(pins["builtin"], &rows, &recs, parts != 0);
    std::vector<Tuple> want;
    for (const auto& t : pins["derived_tuples"]) want.push_back(Tuple(t.at(0), t.at(1)));
    CHECK(as_tuples(rows, recs) == want);
    CHECK(rows.size() == pins["derived_rows"].size());
    for (size_t a = 0; a < rows.size() && a < pins["derived_rows"].size(); ++a)
      CHECK(rows[a].closed == (uint32_t)pins["derived_rows"][a].at(0) && rows[a].total == pins["derived_rows"][a].at(1));
  }
  // testCounts: SumAndEmitCounters alone
  Reference ref;
  std::vector<Tuple> out;
  for (const auto& t : pins["counts_in"]) ref.sum_and_emit(t.at(0), t.at(1), &out);
  CHECK(out.size() == pins["counts_out"].size());
  for (size_t i = 0; i < out.size() && i < pins["counts_out"].size(); ++i)
    CHECK(out[i] == Tuple(pins["counts_out"][i].at(0), pins["counts_out"][i].at(1)));
  puts("ok pins");
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) {
    puts("usage: tristream_seq_sanitize <pins.txt>");
    return 2;
  }
  check_reference();
  check_parts();
  check_modes_and_limits();
  check_pins(argv[1]);
  if (failures) {
    printf("%d failure(s)\n", failures);
    return 1;
  }
  puts("all checks passed");
  return 0;
}
