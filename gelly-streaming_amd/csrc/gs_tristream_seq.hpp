// gs_tristream_seq.hpp -- the rules of the triangle streams (gs_tristream_k.hip, gs_tristream.cpp):
// every record example/ExactTriangleCount.java emits (buildNeighborhood(false), ProjectCanonicalEdges,
// IntersectNeighborhoods, SumAndEmitCounters), exact in arrival order. Plain functions of their
// arguments with standard headers and gs_triangle_rows.hpp only: the kernels include this header,
// and a host compiler builds tests/cpp/tristream_seq_sanitize.cpp from it.
//
// The sequential definition (parallelism 1). State: G, a set of unordered pairs {u, v}, u != v,
// each with first{u,v}, the number of the arrival that added it (1-based, every arrival counted,
// loops included); a 64-bit counter t(v) per vertex; the 64-bit total T; the arrival count.
// Arrival number t = (s, d):
//   1. s == d: nothing is emitted, G, t() and T stay; its row is (closed 0, total T). The
//      reference's self-loop artefacts (a vertex in its own neighbourhood) are NOT reproduced.
//   2. u = min(s, d), v = max(s, d) in signed order; {u, v} not in G: it joins with first = t.
//   3. C = { w : {u, w} in G with first < t and {v, w} in G with first < t }, c = |C|.
//   4. mode `count` (the reference, ExactTriangleCount.java:82-103): a repeated pair is intersected
//      again. Mode `ignore`: an arrival whose pair was in G before it has c = 0.
//   5. c > 0: the records, in this order: (w, t(w) += 1) for every w of C ascending in signed
//      order; (u, t(u) += c); (v, t(v) += c); then T += c. The total is not a record (-1 may be
//      a vertex).
//   6. the arrival's row is (closed = c, total = T after).
// Rows and records of consecutive folds, concatenated, are the same wherever the stream is cut.
//
// The parallel form (trs_fold_parts walks exactly these steps on the host). The arrivals of a fold
// are sorted stably by (u, v); the head of a run of equal pairs that is not in A is a new pair
// with the stamp of that arrival; A, the new pairs and their reverses are merged by position
// (tri_merge_pos). The merged adjacency holds pairs that arrive later in the same fold: the stamp
// test of rule 3 is what excludes them. c is scanned over the arrivals (rows, record offsets);
// the records are written in arrival order, sorted stably by vertex, and a segmented sum seeded
// with the stored counter gives every record its count: tiles reduced to one TrsSeg, the tile
// aggregates scanned, every position applied; the segment tails are the new counters.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "gs_triangle_rows.hpp"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GS_TRS_HD __host__ __device__ inline
#else
#define GS_TRS_HD inline
#endif

namespace gs {

// the values of include/gs_summary.h's gs_tristream_repeats
enum TrsRepeats : int { kTrsCount = 0, kTrsIgnore = 1, kTrsModes = 2 };

constexpr uint64_t kTrsMaxTotal = 0x7FFFFFFFull;  // arrivals since reset: stamps and record arrival indices are 32-bit
constexpr uint64_t kTrsMaxFold = 1ull << 22;      // arrivals of the largest fold whose rows are kept
constexpr uint64_t kTrsMaxRecords = 1ull << 27;   // records of one fold (gsamd.TRISTREAM_MAX_RECORDS)

// ---- rule 2
GS_TRS_HD void trs_canon(int64_t s, int64_t d, int64_t* u, int64_t* v) {
  *u = s < d ? s : d;
  *v = s < d ? d : s;
}
// ---- rule 3: an entry counts for arrival number t iff its pair joined G before it
GS_TRS_HD bool trs_stamp_ok(uint32_t first, uint32_t t) { return first < t; }
// the number of arrival a of a fold that follows t0 arrivals
GS_TRS_HD uint32_t trs_arrival_no(uint64_t t0, uint64_t a) { return (uint32_t)(t0 + 1 + a); }
// ---- rule 5: the records of an arrival that closes c triangles, and the delta of its k-th
GS_TRS_HD uint64_t trs_record_count(uint32_t c) { return c ? (uint64_t)c + 2 : 0; }
GS_TRS_HD uint32_t trs_record_delta(uint64_t k, uint32_t c) { return k < c ? 1u : c; }

// ---- the segmented sum: two sums since the last segment head, and whether one was seen. The
// arrival scan runs it with one segment (a = c, b = records); the record scan with a = delta.
struct TrsSeg {
  int64_t a, b;
  uint32_t head;
};
GS_TRS_HD TrsSeg trs_seg_identity() { return TrsSeg{0, 0, 0u}; }
GS_TRS_HD TrsSeg trs_seg_element(int64_t a, int64_t b, bool head) { return TrsSeg{a, b, head ? 1u : 0u}; }
GS_TRS_HD TrsSeg trs_seg_combine(const TrsSeg& first, const TrsSeg& then) {
  if (then.head) return then;
  return TrsSeg{first.a + then.a, first.b + then.b, first.head};
}
// the value after a position: its segment's seed plus everything since the head, itself included
// (`upto`: carry-in, in-tile prefix and the position combined)
GS_TRS_HD int64_t trs_seg_after(const TrsSeg& upto, int64_t seed) { return seed + upto.a; }
#if defined(__HIPCC__)
// what gs_scan.hpp's block_seg_excl needs of a TrsSeg
struct TrsSegOps {
  using Seg = TrsSeg;
  static __device__ __forceinline__ TrsSeg identity() { return trs_seg_identity(); }
  static __device__ __forceinline__ TrsSeg combine(const TrsSeg& a, const TrsSeg& b) { return trs_seg_combine(a, b); }
  static __device__ __forceinline__ TrsSeg shfl_up(const TrsSeg& x, int o) {
    TrsSeg y;
    y.a = __shfl_up((long long)x.a, o, 64);
    y.b = __shfl_up((long long)x.b, o, 64);
    y.head = __shfl_up(x.head, o, 64);
    return y;
  }
};
#endif

GS_TRS_HD uint64_t trs_tiles(uint64_t n, uint32_t tile) { return (n + tile - 1) / tile; }

// ---- rule 3 over a sorted adjacency (x, y, first) of n entries: the common neighbours of the
// rows [sb, se) (walked) and [lb, le) (searched) whose two entries both pass the stamp test.
// The entry q of the walked row is a hit iff trs_hit() names its partner.
GS_TRS_HD bool trs_hit(const int64_t* y, const uint32_t* first, uint64_t q, uint64_t lb, uint64_t le, uint32_t t) {
  if (!trs_stamp_ok(first[q], t)) return false;
  const uint64_t p = tri_member(y, lb, le, y[q]);
  return p != kTriNone && trs_stamp_ok(first[p], t);
}
// the shorter of two rows is walked: rows u = [ub, ue), v = [vb, ve)
GS_TRS_HD void trs_pick_rows(uint64_t ub, uint64_t ue, uint64_t vb, uint64_t ve, uint64_t* sb, uint64_t* se, uint64_t* lb,
                             uint64_t* le) {
  const bool ushort = ue - ub <= ve - vb;
  *sb = ushort ? ub : vb;
  *se = ushort ? ue : ve;
  *lb = ushort ? vb : ub;
  *le = ushort ? ve : ue;
}

}  // namespace gs

#ifndef GS_TRISTREAM_SEQ_RULES_ONLY
// ---- host restatements: the definition, and the kernels' decomposition
#include <algorithm>
#include <iterator>
#include <map>
#include <numeric>
#include <utility>
#include <vector>

namespace gs {

struct TrsRow {
  uint32_t closed;
  int64_t total;
  bool operator==(const TrsRow& o) const { return closed == o.closed && total == o.total; }
};
struct TrsRec {
  uint32_t arrival;  // index in the fold
  int64_t vertex, count;
  bool operator==(const TrsRec& o) const { return arrival == o.arrival && vertex == o.vertex && count == o.count; }
};
struct TrsState {
  std::map<std::pair<int64_t, int64_t>, uint32_t> first;  // G: (u, v), u < v -> the arrival that added it
  std::map<int64_t, std::map<int64_t, uint32_t>> nb;      // the same pairs by vertex: neighbour -> first
  std::map<int64_t, int64_t> t;                           // (entries at 0 are vertices without a triangle)
  int64_t total = 0;
  uint64_t arrivals = 0;
  bool operator==(const TrsState& o) const {
    const auto live = [](std::map<int64_t, int64_t> m) {
      for (auto it = m.begin(); it != m.end();) it = it->second ? std::next(it) : m.erase(it);
      return m;
    };
    return first == o.first && live(t) == live(o.t) && total == o.total && arrivals == o.arrivals;
  }
};

// The definition: rules 1 - 6, one arrival after the other. rows / recs are appended to.
inline void trs_fold_seq(TrsState& st, const int64_t* src, const int64_t* dst, size_t n, int mode, std::vector<TrsRow>* rows,
                         std::vector<TrsRec>* recs) {
  std::map<int64_t, std::map<int64_t, uint32_t>>& nb = st.nb;
  for (size_t a = 0; a < n; ++a) {
    const uint32_t t = trs_arrival_no(st.arrivals, 0);
    ++st.arrivals;
    if (src[a] == dst[a]) {
      rows->push_back(TrsRow{0u, st.total});
      continue;
    }
    int64_t u, v;
    trs_canon(src[a], dst[a], &u, &v);
    const bool was = st.first.count(std::make_pair(u, v)) != 0;
    if (!was) {
      st.first[std::make_pair(u, v)] = t;
      nb[u][v] = t;
      nb[v][u] = t;
    }
    std::vector<int64_t> C;
    if (!(mode == kTrsIgnore && was)) {
      // the smaller neighbourhood is walked, as the reference does; either way ascending in signed order
      const bool ushort = nb[u].size() <= nb[v].size();
      const std::map<int64_t, uint32_t>& walk = ushort ? nb[u] : nb[v];
      const std::map<int64_t, uint32_t>& look = ushort ? nb[v] : nb[u];
      for (const auto& e : walk) {
        const auto it = look.find(e.first);
        if (it != look.end() && trs_stamp_ok(e.second, t) && trs_stamp_ok(it->second, t)) C.push_back(e.first);
      }
    }
    const uint32_t c = (uint32_t)C.size();
    for (const int64_t w : C) recs->push_back(TrsRec{(uint32_t)a, w, st.t[w] += 1});
    if (c) {
      recs->push_back(TrsRec{(uint32_t)a, u, st.t[u] += c});
      recs->push_back(TrsRec{(uint32_t)a, v, st.t[v] += c});
      st.total += c;
    }
    rows->push_back(TrsRow{c, st.total});
  }
}

// One seeded segmented sum as the kernels run it: positions pay[0 .. n) (sorted stably by key
// when `segmented`, one segment in index order otherwise), a reduce of every tile to one TrsSeg,
// an exclusive scan of the tile aggregates, an apply pass. after_a / before_b are written at the
// position's own index. *crossed += tiles that begin inside a segment (segmented scans only).
inline TrsSeg trs_scan_parts(const std::vector<int64_t>& key, const std::vector<int64_t>& a, const std::vector<int64_t>& b,
                             bool segmented, const std::map<int64_t, int64_t>* seeds, int64_t seed0, uint32_t tile,
                             std::vector<uint32_t>* order, std::vector<int64_t>* after_a, std::vector<int64_t>* before_b,
                             uint64_t* crossed) {
  const size_t n = a.size();
  after_a->assign(n, 0);
  before_b->assign(n, 0);
  std::vector<uint32_t>& pay = *order;
  pay.resize(n);
  std::iota(pay.begin(), pay.end(), 0u);
  if (segmented) std::stable_sort(pay.begin(), pay.end(), [&](uint32_t x, uint32_t y) { return key[x] < key[y]; });
  const auto head = [&](size_t j) { return j == 0 || (segmented && key[pay[j]] != key[pay[j - 1]]); };
  const size_t tiles = (size_t)trs_tiles(n, tile);
  std::vector<TrsSeg> agg(tiles), carry(tiles);
  for (size_t t = 0; t < tiles; ++t) {  // reduce
    TrsSeg s = trs_seg_identity();
    for (size_t j = t * tile; j < std::min(n, (t + 1) * (size_t)tile); ++j)
      s = trs_seg_combine(s, trs_seg_element(a[pay[j]], b[pay[j]], head(j)));
    agg[t] = s;
    if (segmented && t && !head(t * tile)) ++*crossed;
  }
  TrsSeg run = trs_seg_identity();
  for (size_t t = 0; t < tiles; ++t) {  // the scan of the aggregates
    carry[t] = run;
    run = trs_seg_combine(run, agg[t]);
  }
  for (size_t t = 0; t < tiles; ++t) {  // apply
    TrsSeg in = trs_seg_identity();
    for (size_t j = t * tile; j < std::min(n, (t + 1) * (size_t)tile); ++j) {
      int64_t seed = seed0;
      if (seeds) {
        const auto it = seeds->find(key[pay[j]]);
        seed = it == seeds->end() ? 0 : it->second;
      }
      const TrsSeg before = trs_seg_combine(carry[t], in);
      (*before_b)[pay[j]] = head(j) ? 0 : before.b;
      in = trs_seg_combine(in, trs_seg_element(a[pay[j]], b[pay[j]], head(j)));
      (*after_a)[pay[j]] = trs_seg_after(trs_seg_combine(carry[t], in), seed);
    }
  }
  return run;
}

// The kernels' decomposition of a fold, from the same functions. Returns the tiles of the record
// scan that began inside a segment; a fold whose records would pass max_records changes nothing
// and returns ~0.
inline uint64_t trs_fold_parts(TrsState& st, const int64_t* src, const int64_t* dst, size_t n, int mode, uint32_t tile,
                               uint64_t max_records, std::vector<TrsRow>* rows, std::vector<TrsRec>* recs) {
  const uint64_t t0 = st.arrivals;
  // A: the sorted adjacency with stamps
  std::vector<int64_t> ax, ay;
  std::vector<uint32_t> af;
  {
    std::vector<std::pair<std::pair<int64_t, int64_t>, uint32_t>> e;
    for (const auto& p : st.first) {
      e.push_back(std::make_pair(std::make_pair(p.first.first, p.first.second), p.second));
      e.push_back(std::make_pair(std::make_pair(p.first.second, p.first.first), p.second));
    }
    std::sort(e.begin(), e.end());
    for (const auto& p : e) {
      ax.push_back(p.first.first);
      ay.push_back(p.first.second);
      af.push_back(p.second);
    }
  }
  // canonise; sort the arrival indices stably by (min, max); the run heads not in A are N
  std::vector<int64_t> lo(n), hi(n);
  for (size_t a = 0; a < n; ++a) trs_canon(src[a], dst[a], &lo[a], &hi[a]);
  std::vector<uint32_t> pay(n);
  std::iota(pay.begin(), pay.end(), 0u);
  std::stable_sort(pay.begin(), pay.end(),
                   [&](uint32_t x, uint32_t y) { return tri_pair_less(lo[x], hi[x], lo[y], hi[y]); });
  std::vector<int64_t> nx, ny;
  std::vector<uint32_t> nf;
  std::vector<uint8_t> isnew(n, 0);
  for (size_t i = 0; i < n; ++i) {
    const uint32_t r = pay[i];
    bool keep = lo[r] != hi[r];
    if (keep && i > 0 && lo[pay[i - 1]] == lo[r] && hi[pay[i - 1]] == hi[r]) keep = false;
    if (keep && tri_has_pair(ax.data(), ay.data(), ax.size(), lo[r], hi[r])) keep = false;
    if (!keep) continue;
    isnew[r] = 1;
    nx.push_back(lo[r]);
    ny.push_back(hi[r]);
    nf.push_back(trs_arrival_no(t0, r));
  }
  const size_t m = nx.size();
  // the reverse entries ordered by (max, min): a stable sort of N by max
  std::vector<uint32_t> rp(m);
  std::iota(rp.begin(), rp.end(), 0u);
  std::stable_sort(rp.begin(), rp.end(), [&](uint32_t x, uint32_t y) { return ny[x] < ny[y]; });
  std::vector<int64_t> rx(m), ry(m);
  std::vector<uint32_t> rf(m);
  for (size_t j = 0; j < m; ++j) {
    rx[j] = ny[rp[j]];
    ry[j] = nx[rp[j]];
    rf[j] = nf[rp[j]];
  }
  // the stamped merge, every entry to its own position
  const size_t an = ax.size(), total = an + 2 * m;
  std::vector<int64_t> ox(total), oy(total);
  std::vector<uint32_t> of(total);
  const auto put = [&](uint64_t pos, int64_t x, int64_t y, uint32_t f) {
    ox.at(pos) = x;
    oy.at(pos) = y;
    of.at(pos) = f;
  };
  for (size_t i = 0; i < an; ++i)
    put(tri_merge_pos(i, ax[i], ay[i], nx.data(), ny.data(), m, rx.data(), ry.data(), m), ax[i], ay[i], af[i]);
  for (size_t j = 0; j < m; ++j) {
    put(tri_merge_pos(j, nx[j], ny[j], ax.data(), ay.data(), an, rx.data(), ry.data(), m), nx[j], ny[j], nf[j]);
    put(tri_merge_pos(j, rx[j], ry[j], ax.data(), ay.data(), an, nx.data(), ny.data(), m), rx[j], ry[j], rf[j]);
  }
  // the filtered intersection, counted
  struct Info {
    uint64_t sb, se, lb, le;
  };
  std::vector<Info> info(n, Info{0, 0, 0, 0});
  std::vector<int64_t> c(n, 0), rc(n, 0), none(n, 0);
  for (size_t a = 0; a < n; ++a) {
    if (lo[a] == hi[a] || (mode == kTrsIgnore && !isnew[a])) continue;
    uint64_t ub, ue, vb, ve;
    tri_row(ox.data(), total, lo[a], &ub, &ue);
    tri_row(ox.data(), total, hi[a], &vb, &ve);
    Info& ri = info[a];
    trs_pick_rows(ub, ue, vb, ve, &ri.sb, &ri.se, &ri.lb, &ri.le);
    for (uint64_t q = ri.sb; q < ri.se; ++q)
      if (trs_hit(oy.data(), of.data(), q, ri.lb, ri.le, trs_arrival_no(t0, a))) ++c[a];
    rc[a] = (int64_t)trs_record_count((uint32_t)c[a]);
  }
  // rows and record offsets: one scan over the arrivals
  std::vector<uint32_t> order;
  std::vector<int64_t> tot, off;
  uint64_t crossed = 0;
  const TrsSeg sum = trs_scan_parts(none, c, rc, false, nullptr, st.total, tile, &order, &tot, &off, &crossed);
  const uint64_t R = (uint64_t)sum.b;
  if (R > max_records) return ~0ull;  // nothing was changed
  // the ordered write
  std::vector<uint32_t> r_arr(R);
  std::vector<int64_t> r_v(R), r_delta(R), zero(R, 0);
  for (size_t a = 0; a < n; ++a) {
    if (!c[a]) continue;
    uint64_t k = (uint64_t)off[a];
    const Info& ri = info[a];
    for (uint64_t q = ri.sb; q < ri.se; ++q)
      if (trs_hit(oy.data(), of.data(), q, ri.lb, ri.le, trs_arrival_no(t0, a))) r_v.at(k++) = oy[q];
    r_v.at(k++) = lo[a];
    r_v.at(k++) = hi[a];
    for (uint64_t j = 0; j < trs_record_count((uint32_t)c[a]); ++j) {
      r_arr.at((uint64_t)off[a] + j) = (uint32_t)a;
      r_delta.at((uint64_t)off[a] + j) = trs_record_delta(j, (uint32_t)c[a]);
    }
  }
  // running counts: the segmented sum seeded with the stored counters, then the tails
  std::vector<int64_t> cnt, unused;
  trs_scan_parts(r_v, r_delta, zero, true, &st.t, 0, tile, &order, &cnt, &unused, &crossed);
  for (size_t j = 0; j < R; ++j)
    if (j + 1 == R || r_v[order[j]] != r_v[order[j + 1]]) st.t[r_v[order[j]]] = cnt[order[j]];
  // commit
  for (size_t j = 0; j < m; ++j) {
    st.first[std::make_pair(nx[j], ny[j])] = nf[j];
    st.nb[nx[j]][ny[j]] = nf[j];
    st.nb[ny[j]][nx[j]] = nf[j];
  }
  st.total = n ? tot[n - 1] : st.total;
  st.arrivals += n;
  for (size_t a = 0; a < n; ++a) rows->push_back(TrsRow{(uint32_t)c[a], tot[a]});
  for (size_t r = 0; r < R; ++r) recs->push_back(TrsRec{r_arr[r], r_v[r], cnt[r]});
  return crossed;
}

}  // namespace gs
#endif  // GS_TRISTREAM_SEQ_RULES_ONLY
