// The removal arithmetic of the triangle summary (csrc/gs_triangle_rows.hpp: tri_pair_at,
// tri_is_old, tri_rebase, tri_row_gone) against brute force, built with
// -fsanitize=address,undefined and run by tests/test_triangle_removal_rows.py. Host code only.
// A removal on the host, composed of the same functions as the kernels compose them -- the
// dying bytes, the survivors' positions, the vanished rows, the compaction, and the once-only
// rule over the dying edges with tri_edge_before -- is compared with a recount of the
// surviving graph. Every array is a heap allocation of its exact size, so a read one past an
// end is reported.
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

template <class T>
static std::unique_ptr<T[]> exact(const std::vector<T>& v) {
  std::unique_ptr<T[]> p(v.empty() ? nullptr : new T[v.size()]);
  std::copy(v.begin(), v.end(), p.get());
  return p;
}

static void check_stamps() {
  const uint32_t top = 0xFFFFFFFFu, half = 0x80000000u;
  const uint32_t stamps[] = {0, 1, 2, 5, half - 1, half, half + 1, top - 2, top - 1, top};
  const uint64_t folds[] = {1, 2, 3, half - 1, half, (uint64_t)top, (uint64_t)top + 1, 1ull << 40, ~0ull};
  for (uint32_t cur : stamps)
    for (uint32_t s : stamps)
      for (uint64_t f : folds) {
        if (s > cur) {
          CHECK(!gs::tri_is_old(s, cur, f));
          continue;
        }
        // s + f <= cur in arithmetic wide enough for it (f up to 2^64 - 1: compare by parts)
        const bool want = f <= (uint64_t)cur && (uint64_t)s <= (uint64_t)cur - f;
        CHECK(gs::tri_is_old(s, cur, f) == want);
      }
  // the wrap: the fold after number 2^32 - 1 is number 2^31, and every age of at most 2^31 - 1
  // folds is what it was
  for (uint32_t s : stamps) {
    const uint32_t r = gs::tri_rebase(s);
    CHECK(r < half);
    const uint64_t age_before = (1ull << 32) - s;  // to the fold that wrapped
    const uint64_t age_after = (uint64_t)half - r;
    if (age_before <= half) CHECK(age_after == age_before);
    else CHECK(r == 0 && age_after == half);
  }
}

// adjacency of the undirected edges, sorted by (x, y)
static std::vector<Pair> adjacency(const std::set<Pair>& g) {
  std::vector<Pair> a;
  for (const Pair& e : g) a.push_back(e), a.push_back({e.second, e.first});
  std::sort(a.begin(), a.end());
  return a;
}

static long triangles(const std::set<Pair>& g) {
  std::set<int64_t> v;
  for (const Pair& e : g) v.insert(e.first), v.insert(e.second);
  const std::vector<int64_t> id(v.begin(), v.end());
  long t = 0;
  for (size_t a = 0; a < id.size(); ++a)
    for (size_t b = a + 1; b < id.size(); ++b)
      for (size_t c = b + 1; c < id.size(); ++c)
        t += g.count({id[a], id[b]}) && g.count({id[b], id[c]}) && g.count({id[a], id[c]});
  return t;
}

static void check_removal(const std::set<Pair>& g, const std::set<Pair>& dying) {
  const std::vector<Pair> adj = adjacency(g);
  const uint64_t n = adj.size();
  std::vector<int64_t> vx, vy;
  for (const Pair& p : adj) vx.push_back(p.first), vy.push_back(p.second);
  const auto x = exact(vx), y = exact(vy);
  // the dying bytes, as k_tri_flag_new<true> sets them
  std::vector<uint8_t> vdead(n, 0);
  for (const Pair& e : dying) {
    const uint64_t p = gs::tri_pair_at(x.get(), y.get(), n, e.first, e.second);
    const uint64_t p2 = gs::tri_pair_at(x.get(), y.get(), n, e.second, e.first);
    CHECK((p != gs::kTriNone) == (g.count(e) != 0) && (p == gs::kTriNone) == (p2 == gs::kTriNone));
    if (p == gs::kTriNone) continue;
    CHECK(adj[p] == e && adj[p2] == Pair(e.second, e.first));
    vdead[p] = vdead[p2] = 1;
  }
  CHECK(gs::tri_pair_at(x.get(), y.get(), n, kMax, kMin) == gs::kTriNone || g.count({kMin, kMax}));
  // the survivors' positions and the vanished rows
  std::vector<uint32_t> vpos(n, 0);
  uint32_t live = 0;
  for (uint64_t i = 0; i < n; ++i) vpos[i] = live, live += vdead[i] ? 0 : 1;
  const auto pos = exact(vpos);
  std::set<Pair> rest;
  for (const Pair& e : g)
    if (!dying.count(e)) rest.insert(e);
  std::set<int64_t> alive;
  for (const Pair& e : rest) alive.insert(e.first), alive.insert(e.second);
  uint64_t gone = 0, heads = 0;
  for (uint64_t i = 0; i < n; ++i) {
    if (i && x[i - 1] == x[i]) continue;
    ++heads;
    const bool g1 = gs::tri_row_gone(x.get(), n, i, pos.get(), live);
    CHECK(g1 == (alive.count(x[i]) == 0));
    gone += g1;
  }
  CHECK(heads - gone == alive.size());
  // the compaction is the survivors' adjacency
  std::vector<Pair> kept(live);
  for (uint64_t i = 0; i < n; ++i)
    if (!vdead[i]) kept[vpos[i]] = adj[i];
  CHECK(kept == adjacency(rest));
  // the once-only rule over the dying edges: every destroyed triangle at its greatest dying edge
  long destroyed = 0;
  for (const Pair& e : dying) {
    if (!g.count(e)) continue;
    uint64_t ub, ue, vb, ve;
    gs::tri_row(x.get(), n, e.first, &ub, &ue);
    gs::tri_row(x.get(), n, e.second, &vb, &ve);
    for (uint64_t q = ub; q < ue; ++q) {
      const int64_t w = y[q];
      const uint64_t p = gs::tri_member(y.get(), vb, ve, w);
      if (p == gs::kTriNone) continue;
      const bool ok1 = !vdead[q] || gs::tri_edge_before(e.first, w, e.first, e.second);
      const bool ok2 = !vdead[p] || gs::tri_edge_before(e.second, w, e.first, e.second);
      destroyed += ok1 && ok2;
    }
  }
  CHECK(destroyed == triangles(g) - triangles(rest));
}

int main() {
  std::mt19937_64 rng(0x5E11D1E5ull);
  check_stamps();
  check_removal({}, {});
  check_removal({}, {{1, 2}});
  // K4 with the int64 extremes: every subset of its edges
  {
    const int64_t id[4] = {kMin, -1, 7, kMax};
    std::vector<Pair> e;
    for (int a = 0; a < 4; ++a)
      for (int b = a + 1; b < 4; ++b) e.push_back({id[a], id[b]});
    const std::set<Pair> g(e.begin(), e.end());
    for (int m = 0; m < 64; ++m) {
      std::set<Pair> d;
      for (int k = 0; k < 6; ++k)
        if (m >> k & 1) d.insert(e[k]);
      check_removal(g, d);
    }
  }
  // random graphs, random dying sets with absent pairs among them
  for (int round = 0; round < 200; ++round) {
    const int64_t span = 3 + (int64_t)(rng() % 9);
    const uint64_t m = rng() % 40;
    std::set<Pair> g, d;
    for (uint64_t i = 0; i < m; ++i) {
      const int64_t a = (int64_t)(rng() % (uint64_t)span) - 2, b = (int64_t)(rng() % (uint64_t)span) - 2;
      if (a != b) g.insert({std::min(a, b), std::max(a, b)});
    }
    const uint64_t pct = rng() % 101;
    for (const Pair& e : g)
      if (rng() % 100 < pct) d.insert(e);
    for (int i = 0; i < 3; ++i) {
      const int64_t a = (int64_t)(rng() % (uint64_t)span) - 2, b = a + 1 + (int64_t)(rng() % 3);
      d.insert({a, b});
    }
    check_removal(g, d);
  }
  std::printf("all checks passed (%ld)\n", checks);
  return 0;
}
