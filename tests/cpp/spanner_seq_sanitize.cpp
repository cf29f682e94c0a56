// spanner_seq_sanitize.cpp -- csrc/gs_spanner_seq.hpp against brute force, built with the address
// and undefined-behaviour sanitizers (tests/test_spanner_seq.py). Stand-alone: standard headers
// and the header under test only.
//
// Brute force: the graph as an adjacency matrix over a handful of vertices, within() as "some
// walk of 1..k edges from s ends in t and does not pass through s again" by dynamic programming
// over walk lengths, the fold as the plain loop over it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

#include "gs_spanner_seq.hpp"

namespace {

int failures = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);  \
      if (++failures > 20) std::exit(1);                          \
    }                                                             \
  } while (0)

struct Brute {
  int n;
  std::vector<uint8_t> a;  // n x n, symmetric; a[u][u] is a loop
  explicit Brute(int n_) : n(n_), a((size_t)n_ * n_, 0) {}
  bool has_vertex(int u) const {
    for (int v = 0; v < n; ++v)
      if (a[(size_t)u * n + v]) return true;
    return false;
  }
  bool within(int s, int t, int k) const {
    if (!has_vertex(s)) return false;
    // reach[v]: v is the end of a walk of exactly L edges from s whose inner vertices avoid s
    std::vector<uint8_t> reach((size_t)n, 0), next;
    reach[(size_t)s] = 1;
    for (int L = 1; L <= k; ++L) {
      next.assign((size_t)n, 0);
      for (int u = 0; u < n; ++u)
        if (reach[(size_t)u])
          for (int v = 0; v < n; ++v)
            if (a[(size_t)u * n + v]) next[(size_t)v] = 1;
      if (L > 1) next[(size_t)s] = 0;  // s is not revisited: only its own loop ends in it
      if (next[(size_t)t]) return true;
      next[(size_t)s] = 0;
      reach.swap(next);
    }
    return false;
  }
  void add(int s, int t) { a[(size_t)s * n + t] = a[(size_t)t * n + s] = 1; }
};

int64_t scramble(int v, int salt) {
  if (salt == 0) return v;
  if (v == 0 && salt == 2) return std::numeric_limits<int64_t>::min();
  uint64_t x = (uint64_t)(v + 1) * 0x9E3779B97F4A7C15ull + (uint64_t)salt * 0xD1B54A32D192ED03ull;
  x ^= x >> 31;
  return (int64_t)x;
}

void check_streams() {
  std::mt19937_64 rng(0x5EED5A11u);
  for (int round = 0; round < 300; ++round) {
    const int n = 2 + (int)(rng() % 9), m = 1 + (int)(rng() % 40), k = 1 + (int)(rng() % 5), salt = round % 3;
    std::vector<int> us((size_t)m), vs((size_t)m);
    std::vector<int64_t> src((size_t)m), dst((size_t)m);
    for (int i = 0; i < m; ++i) {
      us[(size_t)i] = (int)(rng() % (uint64_t)n);
      vs[(size_t)i] = (int)(rng() % (uint64_t)n);
      src[(size_t)i] = scramble(us[(size_t)i], salt);
      dst[(size_t)i] = scramble(vs[(size_t)i], salt);
    }
    Brute B(n);
    gs::SpannerSeq S(k), R1(k), R0(k), RH(k);
    std::vector<uint8_t> truth((size_t)m), acc((size_t)m), acc1((size_t)m), acc0((size_t)m), acch((size_t)m);
    for (int i = 0; i < m; ++i) {
      // every pair of vertices, both searches, before the edge is decided
      if (i % 7 == 0)
        for (int s = 0; s < n; ++s)
          for (int t = 0; t < n; ++t)
            for (int kk = 1; kk <= 4; ++kk) {
              const bool w = B.within(s, t, kk);
              CHECK(S.within(scramble(s, salt), scramble(t, salt), kk) == w);
              CHECK(S.within_two_sided(scramble(s, salt), scramble(t, salt), kk) == w);
            }
      const bool keep = !B.within(us[(size_t)i], vs[(size_t)i], k);
      truth[(size_t)i] = keep ? 1 : 0;
      if (keep) B.add(us[(size_t)i], vs[(size_t)i]);
      const uint64_t kept = S.fold(&src[(size_t)i], &dst[(size_t)i], 1, &acc[(size_t)i]);
      CHECK(kept == (keep ? 1u : 0u));
    }
    CHECK(acc == truth);
    // the fold by rounds: two batches, three round caps
    const uint64_t cut = (uint64_t)m / 3;
    uint32_t r1 = 0, r0 = 0, rh = 0, rounds = 0;
    R1.fold_rounds(src.data(), dst.data(), cut, acc1.data(), 1, &rounds);
    R1.fold_rounds(src.data() + cut, dst.data() + cut, (uint64_t)m - cut, acc1.data() + cut, 1, &r1);
    R0.fold_rounds(src.data(), dst.data(), cut, acc0.data(), 0, &rounds);
    R0.fold_rounds(src.data() + cut, dst.data() + cut, (uint64_t)m - cut, acc0.data() + cut, 0, &r0);
    RH.fold_rounds(src.data(), dst.data(), cut, acch.data(), 1u << 30, &rounds);
    RH.fold_rounds(src.data() + cut, dst.data() + cut, (uint64_t)m - cut, acch.data() + cut, 1u << 30, &rh);
    CHECK(acc1 == truth);
    CHECK(acc0 == truth);
    CHECK(acch == truth);
    CHECK(r1 <= 1 && r0 == 0 && rh <= (uint32_t)m);
    CHECK(R1.sorted_edges() == S.sorted_edges() && RH.sorted_edges() == S.sorted_edges());
    CHECK(R0.edges() == S.edges() && R0.vertices() == S.vertices());
    // the export is ascending and holds each edge once
    const auto e = S.sorted_edges();
    CHECK(e.size() == S.edges());
    for (size_t i = 0; i < e.size(); ++i) {
      CHECK(e[i].first <= e[i].second);
      if (i) CHECK(e[i - 1] < e[i]);
    }
  }
}

void check_rules() {
  // the traversal predicate, every combination
  for (int view = 0; view < 3; ++view)
    for (uint32_t j : {0u, 3u, 4u, 5u, gs::kSpDead})
      for (uint8_t st : {gs::kSpUndecided, gs::kSpAccepted, gs::kSpDropped}) {
        const uint32_t i = 4;
        bool want = false;
        if (j < i && view == gs::kSpUpper) want = st != gs::kSpDropped;
        if (j < i && view == gs::kSpLower) want = st == gs::kSpAccepted;
        CHECK(gs::sp_traversable(view, j, i, st) == want);
      }
  CHECK(gs::sp_round_verdict(false, false) == gs::kSpAccepted);
  CHECK(gs::sp_round_verdict(true, true) == gs::kSpDropped);
  CHECK(gs::sp_round_verdict(true, false) == gs::kSpUndecided);
  CHECK(gs::sp_pick_side(1, 1) == 0 && gs::sp_pick_side(2, 1) == 1 && gs::sp_pick_side(0, 5) == 0);
  // capacity arithmetic: a power of two of at least twice the entries, within the LDS budget
  for (uint32_t e = 1; e <= gs::kSpannerLdsSet; ++e) {
    const uint32_t s = gs::sp_set_slots(e);
    CHECK((s & (s - 1)) == 0 && s >= 2 * e && s < 4 * e + 2);
    CHECK(gs::sp_set_bytes(e) == 2 * (s + e) * 8);
    CHECK(gs::sp_clamp_set(e) == e);
  }
  CHECK(gs::sp_set_bytes(gs::kSpannerLdsSet) == 12288);
  CHECK(13 * gs::sp_set_bytes(gs::kSpannerLdsSet) <= 160 * 1024);
  CHECK(gs::sp_clamp_set(0) == 1 && gs::sp_clamp_set(-5) == 1 && gs::sp_clamp_set(1 << 20) == gs::kSpannerLdsSet);
  std::mt19937_64 rng(7);
  for (int i = 0; i < 100000; ++i) {
    const uint32_t slots = 2u << (rng() % 10);
    CHECK(gs::sp_hash((int64_t)rng(), slots) < slots);
  }
  CHECK(gs::sp_hash(std::numeric_limits<int64_t>::min(), 8) < 8);
  CHECK(gs::sp_slow_round(8, 8) && gs::sp_slow_round(800, 701) && !gs::sp_slow_round(800, 700));
  CHECK(!gs::sp_slow_round(1, 0) && !gs::sp_slow_round(7, 6));
  // stamps: never zero, distinct across sides and generations up to the limit
  CHECK(gs::sp_stamp(0, 0) == 1 && gs::sp_stamp(0, 1) == 2 && gs::sp_stamp(1, 0) == 3);
  CHECK(gs::sp_stamp(gs::kSpMaxGen, 1) > gs::sp_stamp(gs::kSpMaxGen, 0));
  CHECK(gs::sp_stamp(gs::kSpMaxGen, 0) > gs::sp_stamp(gs::kSpMaxGen - 1, 1));
}

// AdjacencyListGraphTest.testBoundedBFS and SpannerExample's default stream
void check_pins() {
  gs::SpannerSeq g(3);
  const int64_t a[][2] = {{1, 4}, {4, 5}, {5, 6}, {4, 7}, {7, 8}};
  for (const auto& e : a) g.add(e[0], e[1]);
  CHECK(!g.within(2, 3, 3));
  g.add(2, 3);
  CHECK(!g.within(3, 4, 3));
  g.add(3, 4);
  CHECK(g.within(3, 6, 3));
  CHECK(!g.within(8, 9, 3));
  g.add(8, 9);
  CHECK(!g.within(8, 6, 3));
  g.add(8, 6);
  CHECK(g.within(5, 9, 3));
  const int64_t s[] = {1, 4, 7, 4, 4, 5, 2, 3, 3, 8, 6, 5}, d[] = {4, 7, 8, 8, 5, 6, 3, 4, 6, 9, 8, 9};
  gs::SpannerSeq h(3), hr(3);
  uint8_t acc[12], accr[12];
  uint32_t rounds = 0;
  h.fold(s, d, 12, acc);
  hr.fold_rounds(s, d, 12, accr, 16, &rounds);
  const uint8_t want[12] = {1, 1, 1, 0, 1, 1, 1, 1, 0, 1, 1, 0};
  for (int i = 0; i < 12; ++i) CHECK(acc[i] == want[i] && accr[i] == want[i]);
  CHECK(rounds >= 1);
  // a loop: kept once; a repeated edge: dropped
  gs::SpannerSeq l(2);
  const int64_t ls[] = {5, 5, 5, 6}, ld[] = {5, 5, 6, 5};
  uint8_t la[4];
  l.fold(ls, ld, 4, la);
  CHECK(la[0] == 1 && la[1] == 0 && la[2] == 1 && la[3] == 0);
  CHECK(l.edges() == 2 && l.vertices() == 2);
}

}  // namespace

int main() {
  check_rules();
  check_pins();
  check_streams();
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
