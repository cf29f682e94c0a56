// matching_seq_sanitize.cpp -- csrc/gs_matching_seq.hpp on the host, under the address and UB
// sanitizers (tests/test_matching_seq.py builds and runs it): the wrapping arithmetic at its
// edges, mt_fold_seq against a brute-force restatement that keeps M as a set of edges and scans
// it for every arrival as CentralizedWeightedMatching.java:79-106 does, and mt_fold_rounds -- the
// round scheme through the phase functions the kernels call -- against mt_fold_seq on random
// streams under every tuning and cut at random places.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <vector>

#include "gs_matching_seq.hpp"

using namespace gs;

static int failures = 0;
#define CHECK(cond)                                            \
  do {                                                         \
    if (!(cond)) {                                             \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                              \
    }                                                          \
  } while (0)

// the Java, literally: M a list of edges, every arrival scans all of it
struct Brute {
  std::vector<MtEdge> M;
  uint64_t folded = 0;
  bool step(int64_t u, int64_t v, int64_t w, uint32_t arrival, std::vector<MtEvent>* ev) {
    std::vector<size_t> at_u, at_v;  // collisions: the edge at the source endpoint, then at the target
    for (size_t i = 0; i < M.size(); ++i) {
      const bool tu = M[i].src == u || M[i].dst == u, tv = M[i].src == v || M[i].dst == v;
      if (tu) at_u.push_back(i);
      else if (tv) at_v.push_back(i);
    }
    int64_t sum = 0;
    for (size_t i : at_u) sum = (int64_t)((uint64_t)sum + (uint64_t)M[i].val);
    for (size_t i : at_v) sum = (int64_t)((uint64_t)sum + (uint64_t)M[i].val);
    const uint64_t number = folded++;
    if (!(w > (int64_t)(2ull * (uint64_t)sum))) return false;
    std::vector<size_t> gone = at_u;
    gone.insert(gone.end(), at_v.begin(), at_v.end());
    for (size_t i : gone) ev->push_back(MtEvent{arrival, kMatchRemove, M[i].src, M[i].dst, M[i].val});
    std::vector<MtEdge> keep;
    for (size_t i = 0; i < M.size(); ++i)
      if (std::find(gone.begin(), gone.end(), i) == gone.end()) keep.push_back(M[i]);
    keep.push_back(MtEdge{u, v, w, number});
    M.swap(keep);
    ev->push_back(MtEvent{arrival, kMatchAdd, u, v, w});
    return true;
  }
};

static void check_arithmetic() {
  const int64_t mn = INT64_MIN, mx = INT64_MAX, q = (int64_t)1 << 62;
  CHECK(mt_wrap_add(mx, 1) == mn);
  CHECK(mt_wrap_add(mn, -1) == mx);
  CHECK(mt_wrap_sub(mn, 1) == mx);
  CHECK(mt_wrap_twice(q) == mn);
  CHECK(mt_wrap_twice(mn) == 0);
  CHECK(mt_wrap_twice(mx) == -2);
  CHECK(mt_wrap_add(q, q) == mn);
  CHECK(mt_accepts(0, q));     // 2 * 2^62 wraps to INT64_MIN
  CHECK(mt_accepts(mn + 1, q));
  CHECK(!mt_accepts(mn, q));
  CHECK(mt_accepts(-1, mx));   // 2 * INT64_MAX wraps to -2
  CHECK(!mt_accepts(-2, mx));
  CHECK(mt_accepts(1, mn));    // 2 * INT64_MIN wraps to 0
  CHECK(!mt_accepts(0, mn));
  CHECK(!mt_accepts(5, 5) && mt_accepts(11, 5) && !mt_accepts(10, 5));
  CHECK(!mt_accepts(0, 0) && !mt_accepts(-1, 0) && mt_accepts(1, 0));
  CHECK(mt_weight_safe(0) && mt_weight_safe(((int64_t)1 << 61) - 1));
  CHECK(!mt_weight_safe((int64_t)1 << 61) && !mt_weight_safe(-1) && !mt_weight_safe(mn) && !mt_weight_safe(mx));
  CHECK(sizeof(MtVertex) == 32 && sizeof(MtRec) == 32);
  MtRec r{kMtNone, kMtNone, kMtNone, kMtNone, 0, 0};
  CHECK(mt_event_rows(0, r) == 0 && mt_event_rows(1, r) == 1);
  r.s0 = r.d0 = 0;
  CHECK(mt_event_rows(1, r) == 2);
  r.s1 = r.d1 = 1;
  CHECK(mt_event_rows(1, r) == 3 && mt_event_rows(0, r) == 0);
}

static void check_pins() {
  // the doubling star, the unit path, the bridge (tests/golden/matching_pins.json)
  {
    const int64_t s[] = {0, 0, 0, 0, 0}, d[] = {1, 2, 3, 4, 5}, w[] = {1, 3, 7, 14, 29};
    MatchingSeq m;
    uint8_t a[5];
    std::vector<MtEvent> ev;
    CHECK(mt_fold_seq(m, s, d, w, 5, a, &ev) == 4);
    CHECK(a[0] && a[1] && a[2] && !a[3] && a[4]);
    CHECK(ev.size() == 7 && m.edges() == 1 && m.weight() == 29);
  }
  {
    const int64_t s[] = {1, 2, 3, 4}, d[] = {2, 3, 4, 5}, w[] = {1, 1, 1, 1};
    MatchingSeq m;
    uint8_t a[4];
    CHECK(mt_fold_seq(m, s, d, w, 4, a, nullptr) == 2);
    CHECK(a[0] && !a[1] && a[2] && !a[3]);
  }
  {
    const int64_t s[] = {1, 3, 2}, d[] = {2, 4, 3}, w[] = {5, 5, 21};
    MatchingSeq m;
    uint8_t a[3];
    std::vector<MtEvent> ev;
    CHECK(mt_fold_seq(m, s, d, w, 3, a, &ev) == 3);
    CHECK(ev.size() == 5);
    CHECK((ev[2] == MtEvent{2, kMatchRemove, 1, 2, 5}));
    CHECK((ev[3] == MtEvent{2, kMatchRemove, 3, 4, 5}));
    CHECK((ev[4] == MtEvent{2, kMatchAdd, 2, 3, 21}));
  }
}

enum ValueMode { kUnit, kSmall, kPow2, kHub, kWrap, kModes };

static void make_stream(std::mt19937_64& rng, int mode, std::vector<int64_t>& s, std::vector<int64_t>& d,
                        std::vector<int64_t>& w) {
  const uint64_t n = rng() % 201, nv = 2 + rng() % 99;
  static const int64_t ids[] = {INT64_MIN, INT64_MAX, -1, 0};
  static const int64_t wrap[] = {(int64_t)1 << 62, INT64_MAX, INT64_MIN, -1, -7, ((int64_t)1 << 62) + 5, 3, 1, 0,
                                 (int64_t)1 << 61, ((int64_t)1 << 61) - 1};
  s.resize(n);
  d.resize(n);
  w.resize(n);
  for (uint64_t i = 0; i < n; ++i) {
    auto vertex = [&]() -> int64_t {
      const uint64_t x = rng() % nv;
      return x < 4 ? ids[x] : (int64_t)(x * 1000003);
    };
    s[i] = (mode == kHub && rng() % 10 < 6) ? 77 : vertex();
    d[i] = vertex();
    switch (mode) {
      case kUnit: w[i] = 1; break;
      case kSmall: w[i] = 10 + (int64_t)(rng() % 41); break;
      case kPow2: w[i] = (int64_t)1 << (rng() % 20); break;
      case kHub: w[i] = (int64_t)(rng() % 1000); break;
      default: w[i] = wrap[rng() % (sizeof(wrap) / sizeof(wrap[0]))]; break;
    }
  }
}

static void check_random() {
  std::mt19937_64 rng(20261020);
  uint64_t rounds = 0, fallbacks = 0, streams = 0, unsafe = 0;
  for (int rep = 0; rep < 400; ++rep)
    for (int mode = 0; mode < kModes; ++mode) {
      std::vector<int64_t> s, d, w;
      make_stream(rng, mode, s, d, w);
      const uint64_t n = s.size();
      // brute force against the definition
      Brute b;
      MatchingSeq m;
      std::vector<MtEvent> ev_b, ev_m;
      std::vector<uint8_t> acc_b(n), acc_m(n);
      for (uint64_t i = 0; i < n; ++i) acc_b[i] = b.step(s[i], d[i], w[i], (uint32_t)i, &ev_b) ? 1 : 0;
      mt_fold_seq(m, s.data(), d.data(), w.data(), n, acc_m.data(), &ev_m);
      CHECK(acc_b == acc_m);
      CHECK(ev_b == ev_m);
      CHECK(b.M == m.sorted_edges());
      // the round scheme under every tuning, whole and cut
      for (int tune = 0; tune < 4; ++tune)
        for (int cut = 0; cut < 2; ++cut) {
          MatchingRounds r;
          r.iter_cap = (tune & 1) ? 1 : kMatchingIterCap;
          r.sharpen = !(tune & 2);
          std::vector<uint8_t> acc_r(n, 7);
          std::vector<MtEvent> ev_r;
          uint64_t at = 0;
          while (at < n || (at == 0 && n == 0)) {
            const uint64_t len = cut ? std::min<uint64_t>(n - at, rng() % 40) : n - at;
            std::vector<MtEvent> part;
            const uint64_t kept = mt_fold_rounds(r, s.data() + at, d.data() + at, w.data() + at, len,
                                                 acc_r.data() + at, &part);
            CHECK(kept != ~0ull);
            for (MtEvent e : part) {
              e.arrival += (uint32_t)at;
              ev_r.push_back(e);
            }
            rounds += r.stats.rounds;
            fallbacks += r.stats.fallbacks;
            at += len;
            if (n == 0) break;
          }
          CHECK(acc_r == acc_m);
          CHECK(ev_r == ev_m);
          CHECK(r.sorted_edges() == m.sorted_edges());
          bool safe = true;
          for (int64_t x : w) safe = safe && mt_weight_safe(x);
          CHECK(r.weight_safe == safe);
          unsafe += safe ? 0 : 1;
          ++streams;
        }
    }
  CHECK(fallbacks > 0);  // iteration cap 1 must have met a round that needed more
  CHECK(unsafe > 0);
  printf("random: %llu folds checked, %llu rounds, %llu fell back to plain reservations\n",
         (unsigned long long)streams, (unsigned long long)rounds, (unsigned long long)fallbacks);
}

// a path in path order is a true chain: one round per edge
static void check_chain() {
  const uint64_t n = 200;
  std::vector<int64_t> s(n), d(n), w(n, 1);
  for (uint64_t i = 0; i < n; ++i) {
    s[i] = (int64_t)i;
    d[i] = (int64_t)i + 1;
  }
  MatchingRounds r;
  MatchingSeq m;
  std::vector<uint8_t> a(n), b(n);
  mt_fold_rounds(r, s.data(), d.data(), w.data(), n, a.data(), nullptr);
  mt_fold_seq(m, s.data(), d.data(), w.data(), n, b.data(), nullptr);
  CHECK(a == b);
  CHECK(r.stats.accepted == 100);
  printf("chain: %llu rounds for %llu path edges\n", (unsigned long long)r.stats.rounds, (unsigned long long)n);
}

int main() {
  check_arithmetic();
  check_pins();
  check_random();
  check_chain();
  if (failures) {
    printf("%d checks FAILED\n", failures);
    return 1;
  }
  printf("all checks passed\n");
  return 0;
}
