// The row arithmetic of the triangle summary (csrc/gs_triangle_rows.hpp) against brute
// force, built with -fsanitize=address,undefined and run by tests/test_triangle_rows.py:
// random sorted pair arrays with repeated x values, rows at the array's first and last
// position, the empty array, the int64 extremes, and the three-way merge positions. Every
// array is a heap allocation of its exact size, so a read one past an end is reported.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <memory>
#include <random>
#include <set>
#include <utility>
#include <vector>

#include "gs_triangle_rows.hpp"

using Pair = std::pair<int64_t, int64_t>;
static const int64_t kMin = std::numeric_limits<int64_t>::min(), kMax = std::numeric_limits<int64_t>::max();
static long checks = 0;

#define CHECK(c)                                                    \
  do {                                                              \
    ++checks;                                                       \
    if (!(c)) {                                                     \
      std::printf("FAILED %s (line %d)\n", #c, __LINE__);           \
      std::exit(1);                                                 \
    }                                                               \
  } while (0)

struct Cols {  // exact-size heap copies (nullptr when empty)
  std::unique_ptr<int64_t[]> x, y;
  uint64_t n;
  explicit Cols(const std::vector<Pair>& p) : n(p.size()) {
    if (n) {
      x.reset(new int64_t[n]);
      y.reset(new int64_t[n]);
    }
    for (uint64_t i = 0; i < n; ++i) x[i] = p[i].first, y[i] = p[i].second;
  }
};

static void check_array(const std::vector<Pair>& sorted, const std::vector<int64_t>& probes) {
  const Cols c(sorted);
  const int64_t *x = c.x.get(), *y = c.y.get();
  const uint64_t n = c.n;
  for (int64_t k : probes) {
    uint64_t lo = 0, up = 0;
    for (uint64_t i = 0; i < n; ++i) lo += x[i] < k, up += x[i] <= k;
    CHECK(gs::tri_lower(x, 0, n, k) == lo);
    CHECK(gs::tri_upper(x, 0, n, k) == up);
    uint64_t b = 99, e = 99;
    gs::tri_row(x, n, k, &b, &e);
    CHECK(b == lo && e == up);
    for (int64_t w : probes) {
      uint64_t below = 0, at = gs::kTriNone;
      for (uint64_t i = 0; i < n; ++i) {
        below += Pair(x[i], y[i]) < Pair(k, w);
        if (x[i] == k && y[i] == w) at = i;
      }
      CHECK(gs::tri_pair_lower(x, y, n, k, w) == below);
      CHECK(gs::tri_has_pair(x, y, n, k, w) == (at != gs::kTriNone));
      CHECK(gs::tri_member(y, b, e, w) == at);  // membership inside the row of k
    }
  }
}

static void check_before() {
  const int64_t ids[] = {kMin, kMin + 1, -1, 0, 1, kMax - 1, kMax};
  for (int64_t ex : ids)
    for (int64_t ey : ids)
      for (int64_t u : ids)
        for (int64_t v : ids) {
          if (ex == ey || !(u < v)) continue;
          const Pair f(std::min(ex, ey), std::max(ex, ey));
          CHECK(gs::tri_edge_before(ex, ey, u, v) == (f < Pair(u, v)));
        }
  CHECK(gs::tri_pair_less(kMin, kMax, kMin + 1, kMin));
  CHECK(!gs::tri_pair_less(kMax, kMin, kMax, kMin));
}

// three disjoint sorted lists: every entry's merge position is its rank in the sorted union
static void check_merge(std::mt19937_64& rng, uint64_t total, int64_t span) {
  std::set<Pair> all;
  while (all.size() < total) {
    const int64_t a = (int64_t)(rng() % (uint64_t)span) - span / 2, b = (int64_t)(rng() % (uint64_t)span) - span / 2;
    all.insert({a, b});
  }
  std::vector<Pair> part[3], merged(all.begin(), all.end());
  for (const Pair& p : merged) part[rng() % 3].push_back(p);
  const Cols c0(part[0]), c1(part[1]), c2(part[2]);
  const Cols* c[3] = {&c0, &c1, &c2};
  std::vector<int> hit(merged.size(), 0);
  for (int s = 0; s < 3; ++s) {
    const Cols *o1 = c[(s + 1) % 3], *o2 = c[(s + 2) % 3];
    for (uint64_t i = 0; i < c[s]->n; ++i) {
      const uint64_t pos = gs::tri_merge_pos(i, c[s]->x[i], c[s]->y[i], o1->x.get(), o1->y.get(), o1->n, o2->x.get(),
                                             o2->y.get(), o2->n);
      CHECK(pos < merged.size());
      CHECK(merged[pos] == Pair(c[s]->x[i], c[s]->y[i]));
      ++hit[pos];
    }
  }
  for (int h : hit) CHECK(h == 1);
}

int main() {
  std::mt19937_64 rng(0x7121A61E5ull);
  // the empty array
  check_array({}, {kMin, -1, 0, 1, kMax});
  CHECK(gs::tri_member(nullptr, 0, 0, 5) == gs::kTriNone);
  // the int64 extremes, rows at the first and the last position
  {
    std::vector<Pair> p = {{kMin, kMin + 1}, {kMin, 0}, {kMin, kMax}, {-1, kMin}, {-1, kMax},
                           {0, kMin},        {0, -1},   {0, kMax},    {kMax, kMin}, {kMax, kMax - 1}};
    std::sort(p.begin(), p.end());
    check_array(p, {kMin, kMin + 1, -2, -1, 0, 1, kMax - 1, kMax});
  }
  // one entry; one row only
  check_array({{3, 4}}, {2, 3, 4, 5});
  check_array({{7, 1}, {7, 2}, {7, 9}}, {1, 2, 6, 7, 8, 9});
  // random sorted arrays with repeated x values
  for (int round = 0; round < 60; ++round) {
    const uint64_t n = 1 + rng() % 40;
    const int64_t span = 2 + (int64_t)(rng() % 9);
    std::set<Pair> s;
    for (uint64_t i = 0; i < n; ++i) s.insert({(int64_t)(rng() % (uint64_t)span) - 3, (int64_t)(rng() % (uint64_t)span) - 3});
    std::vector<int64_t> probes;
    for (int64_t k = -5; k <= span; ++k) probes.push_back(k);
    probes.push_back(kMin);
    probes.push_back(kMax);
    check_array(std::vector<Pair>(s.begin(), s.end()), probes);
  }
  check_before();
  check_merge(rng, 0, 8);
  check_merge(rng, 1, 8);
  for (int round = 0; round < 40; ++round) check_merge(rng, 1 + rng() % 60, 10);
  std::printf("all checks passed (%ld)\n", checks);
  return 0;
}
