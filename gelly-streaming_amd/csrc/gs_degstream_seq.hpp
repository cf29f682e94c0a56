// gs_degstream_seq.hpp -- the rules of the degree streams (gs_degstream_k.hip, gs_degstream.cpp):
// every running degree of SimpleEdgeStream.getDegrees / getInDegrees / getOutDegrees and every
// (degree, count) record of example/DegreeDistribution.java, exact in arrival order. Plain
// functions of their arguments with standard headers only: the kernels include this header, and
// a host compiler builds tests/cpp/degstream_seq_sanitize.cpp from it.
//
// The sequential definition. The occurrences of a fold are its collected endpoints in arrival
// order: for edge i the source (direction OUT or ALL), then the target (IN or ALL). An
// occurrence carries c = +1, or -1 when bit 0 of the edge's deletion byte is set; d is the
// vertex's degree before it, 0 while the vertex is absent.
//   1. degree row    old = d, new = max(d + c, 0): the row is (vertex, old, new). A vertex is
//                    present iff d > 0, and an absent vertex forgets a deletion.
//   2. records       old > 0: (new, +1) if new > 0, then (old, -1); old == 0 and c > 0: (1, +1);
//                    old == 0 and c < 0: none.
//   3. distribution  records in arrival order: count[degree] += delta, the row is
//                    (degree, count[degree]). A count may reach 0; it never falls below.
//
// The parallel form. The maps x -> max(x + a, b) are closed under composition (ds_compose) with
// identity (0, -inf), so rule 1 is a segmented scan of pairs over the occurrences sorted stably
// by vertex, seeded with the vertex's stored degree. Rule 3 is the same scan with b = -inf (a
// plain sum) over the records sorted stably by degree, seeded with the stored count. DsSeg adds
// the "a segment head was seen" bit that makes the scan segmented; a tile is reduced to one
// DsSeg, the tile aggregates are scanned, and every position applies carry-in, then its in-tile
// prefix, to the seed (ds_fold_parts walks exactly these steps on the host).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GS_DS_HD __host__ __device__ inline
#else
#define GS_DS_HD inline
#endif

namespace gs {

// the values of include/gs_summary.h's gs_degree_dir
enum DsDirection : int { kDsAll = 0, kDsIn = 1, kDsOut = 2, kDsDirections = 3 };

constexpr int64_t kDsNegInf = -(1ll << 62);            // the b of a map that does not clamp
constexpr uint64_t kDsMaxTotal = 0x7FFFFFFFull;        // occurrences since reset: every degree and count fits 31 bits
constexpr uint64_t kDsMaxFold = 1ull << 24;            // edges of the largest fold whose rows are kept

// ---- occurrences
GS_DS_HD uint64_t ds_occurrences(uint64_t n, int dir) { return dir == kDsAll ? 2 * n : n; }
GS_DS_HD uint64_t ds_occ_edge(uint64_t o, int dir) { return dir == kDsAll ? o >> 1 : o; }
GS_DS_HD bool ds_occ_is_dst(uint64_t o, int dir) { return dir == kDsAll ? (o & 1ull) != 0 : dir == kDsIn; }
GS_DS_HD int ds_sign(const uint8_t* del, uint64_t edge) { return del && (del[edge] & 1u) ? -1 : 1; }

// ---- the maps x -> max(x + a, b)
struct DsPair {
  int64_t a, b;
};
GS_DS_HD DsPair ds_identity() { return DsPair{0, kDsNegInf}; }
// the map of one occurrence (clamp: at 0) or of one record (no clamp: a sum)
GS_DS_HD DsPair ds_element(int c, bool clamp) { return DsPair{(int64_t)c, clamp ? 0 : kDsNegInf}; }
GS_DS_HD int64_t ds_apply(const DsPair& p, int64_t x) {
  const int64_t y = x + p.a;
  return y > p.b ? y : p.b;
}
// `first`, then `then`: (a2, b2) o (a1, b1) = (a1 + a2, max(b1 + a2, b2))
GS_DS_HD DsPair ds_compose(const DsPair& first, const DsPair& then) {
  const int64_t b = first.b + then.a;
  return DsPair{first.a + then.a, b > then.b ? b : then.b};
}

// ---- the segmented form: the maps since the last segment head, and whether one was seen
struct DsSeg {
  int64_t a, b;
  uint32_t head;
};
GS_DS_HD DsSeg ds_seg_identity() { return DsSeg{0, kDsNegInf, 0u}; }
GS_DS_HD DsSeg ds_seg_element(int c, bool clamp, bool head) {
  const DsPair p = ds_element(c, clamp);
  return DsSeg{p.a, p.b, head ? 1u : 0u};
}
GS_DS_HD DsSeg ds_seg_combine(const DsSeg& first, const DsSeg& then) {
  if (then.head) return then;
  const DsPair p = ds_compose(DsPair{first.a, first.b}, DsPair{then.a, then.b});
  return DsSeg{p.a, p.b, first.head};
}
// the value before a position: its segment's seed through everything since the head (`before`:
// carry-in and in-tile prefix combined; the position itself a head: the seed)
GS_DS_HD int64_t ds_seg_before(const DsSeg& before, bool head, int64_t seed) {
  return head ? seed : ds_apply(DsPair{before.a, before.b}, seed);
}
#if defined(__HIPCC__)
// what gs_scan.hpp's block_seg_excl needs of a DsSeg
struct DsSegOps {
  using Seg = DsSeg;
  static __device__ __forceinline__ DsSeg identity() { return ds_seg_identity(); }
  static __device__ __forceinline__ DsSeg combine(const DsSeg& a, const DsSeg& b) { return ds_seg_combine(a, b); }
  static __device__ __forceinline__ DsSeg shfl_up(const DsSeg& x, int o) {
    DsSeg y;
    y.a = __shfl_up((long long)x.a, o, 64);
    y.b = __shfl_up((long long)x.b, o, 64);
    y.head = __shfl_up(x.head, o, 64);
    return y;
  }
};
#endif

// ---- rule 2
GS_DS_HD uint32_t ds_record_count(uint32_t old_d, uint32_t new_d, int c) {
  if (old_d > 0) return new_d > 0 ? 2u : 1u;
  return c > 0 ? 1u : 0u;
}
// record k < ds_record_count of an occurrence
GS_DS_HD void ds_record(uint32_t old_d, uint32_t new_d, uint32_t k, uint32_t* degree, int* delta) {
  if (old_d > 0 && !(new_d > 0 && k == 0)) {
    *degree = old_d;
    *delta = -1;
  } else {
    *degree = old_d > 0 ? new_d : 1u;
    *delta = 1;
  }
}

// ---- tiles of the scans: positions 0 .. n - 1 cut into tiles, a thread owns `per` consecutive ones
GS_DS_HD uint64_t ds_tiles(uint64_t n, uint32_t tile) { return (n + tile - 1) / tile; }
// the count array holds degrees 0 .. cap - 1
GS_DS_HD uint64_t ds_count_cap(uint64_t max_degree, uint64_t min_cap) {
  uint64_t c = min_cap;
  while (c < max_degree + 1) c <<= 1;
  return c;
}

}  // namespace gs

#ifndef GS_DEGSTREAM_SEQ_RULES_ONLY
// ---- host restatements: the definition, and the kernels' decomposition
#include <algorithm>
#include <map>
#include <iterator>
#include <numeric>
#include <utility>
#include <vector>

namespace gs {

struct DsRow {
  int64_t vertex;
  uint32_t old_d, new_d;
  bool operator==(const DsRow& o) const { return vertex == o.vertex && old_d == o.old_d && new_d == o.new_d; }
};
struct DsRec {
  uint32_t occ, degree, count;
  bool operator==(const DsRec& o) const { return occ == o.occ && degree == o.degree && count == o.count; }
};
struct DsState {
  std::map<int64_t, uint32_t> degree;  // (entries at 0 are absent vertices)
  std::map<uint32_t, uint32_t> count;
  bool operator==(const DsState& o) const {
    const auto live = [](const auto& m) {
      auto c = m;
      for (auto it = c.begin(); it != c.end();) it = it->second ? std::next(it) : c.erase(it);
      return c;
    };
    return live(degree) == live(o.degree) && live(count) == live(o.count);
  }
};

// The definition: rules 1 - 3, one occurrence after the other. rows / recs are appended to.
inline void ds_fold_seq(DsState& st, const int64_t* src, const int64_t* dst, const uint8_t* del, size_t n, int dir,
                        std::vector<DsRow>* rows, std::vector<DsRec>* recs) {
  const uint64_t occs = ds_occurrences(n, dir);
  for (uint64_t o = 0; o < occs; ++o) {
    const uint64_t e = ds_occ_edge(o, dir);
    const int64_t v = ds_occ_is_dst(o, dir) ? dst[e] : src[e];
    const int c = ds_sign(del, e);
    uint32_t& d = st.degree[v];
    const uint32_t old_d = d, new_d = (uint32_t)ds_apply(ds_element(c, true), (int64_t)d);
    d = new_d;
    rows->push_back(DsRow{v, old_d, new_d});
    for (uint32_t k = 0; k < ds_record_count(old_d, new_d, c); ++k) {
      uint32_t deg;
      int delta;
      ds_record(old_d, new_d, k, &deg, &delta);
      uint32_t& cnt = st.count[deg];
      cnt = (uint32_t)((int64_t)cnt + delta);
      recs->push_back(DsRec{(uint32_t)o, deg, cnt});
    }
  }
}

// One seeded segmented scan as the kernels run it: a stable sort of the positions by key, a
// reduce of every tile to one DsSeg, an exclusive scan of the tile aggregates, and an apply
// pass that writes (before, after) at each position's arrival index and the state at segment
// tails. Key: the state map's key type. *crossed += tiles that begin inside a segment.
template <class Key>
inline void ds_scan_parts(const std::vector<Key>& key, const std::vector<int>& c, bool clamp,
                          std::map<Key, uint32_t>& state, uint32_t tile, std::vector<uint32_t>* before,
                          std::vector<uint32_t>* after, uint64_t* crossed) {
  const size_t n = key.size();
  before->assign(n, 0);
  after->assign(n, 0);
  if (n == 0) return;
  std::vector<uint32_t> pay(n);
  std::iota(pay.begin(), pay.end(), 0u);
  std::stable_sort(pay.begin(), pay.end(), [&](uint32_t x, uint32_t y) { return key[x] < key[y]; });
  const auto head = [&](size_t j) { return j == 0 || key[pay[j]] != key[pay[j - 1]]; };
  const auto tail = [&](size_t j) { return j + 1 == n || key[pay[j]] != key[pay[j + 1]]; };
  const size_t tiles = (size_t)ds_tiles(n, tile);
  std::vector<DsSeg> agg(tiles), carry(tiles);
  for (size_t t = 0; t < tiles; ++t) {  // reduce
    DsSeg s = ds_seg_identity();
    for (size_t j = t * tile; j < std::min(n, (t + 1) * (size_t)tile); ++j)
      s = ds_seg_combine(s, ds_seg_element(c[pay[j]], clamp, head(j)));
    agg[t] = s;
    if (t && !head(t * tile)) ++*crossed;
  }
  DsSeg run = ds_seg_identity();
  for (size_t t = 0; t < tiles; ++t) {  // the scan of the aggregates
    carry[t] = run;
    run = ds_seg_combine(run, agg[t]);
  }
  std::vector<std::pair<Key, uint32_t>> late;  // at most one per tile
  for (size_t t = 0; t < tiles; ++t) {  // apply
    DsSeg in = ds_seg_identity();
    for (size_t j = t * tile; j < std::min(n, (t + 1) * (size_t)tile); ++j) {
      const Key k = key[pay[j]];
      const auto it = state.find(k);
      const int64_t seed = it == state.end() ? 0 : (int64_t)it->second;
      const int64_t x = ds_seg_before(ds_seg_combine(carry[t], in), head(j), seed);
      const int64_t y = ds_apply(ds_element(c[pay[j]], clamp), x);
      (*before)[pay[j]] = (uint32_t)x;
      (*after)[pay[j]] = (uint32_t)y;
      in = ds_seg_combine(in, ds_seg_element(c[pay[j]], clamp, head(j)));
      if (!tail(j)) continue;
      // a segment inside one tile: every reader of its seed is this tile; one that began in an
      // earlier tile has readers there, so its tail is committed after the pass
      if (in.head)
        state[k] = (uint32_t)y;
      else
        late.push_back(std::make_pair(k, (uint32_t)y));
    }
  }
  for (const auto& kv : late) state[kv.first] = kv.second;  // commit
}

// The kernels' decomposition of a fold, from the same functions: the clamped scan over the
// occurrences sorted by vertex, the record compaction in arrival order, the seeded sum over the
// records sorted by degree. A key's seed is read inside its one segment and its state is written
// at that segment's tail, the last position to read it. Returns the tiles that began inside a
// segment.
inline uint64_t ds_fold_parts(DsState& st, const int64_t* src, const int64_t* dst, const uint8_t* del, size_t n,
                              int dir, uint32_t tile, std::vector<DsRow>* rows, std::vector<DsRec>* recs) {
  const uint64_t occs = ds_occurrences(n, dir);
  std::vector<int64_t> v(occs);
  std::vector<int> c(occs);
  for (uint64_t o = 0; o < occs; ++o) {
    const uint64_t e = ds_occ_edge(o, dir);
    v[o] = ds_occ_is_dst(o, dir) ? dst[e] : src[e];
    c[o] = ds_sign(del, e);
  }
  uint64_t crossed = 0;
  std::vector<uint32_t> old_d, new_d;
  ds_scan_parts(v, c, true, st.degree, tile, &old_d, &new_d, &crossed);
  // compaction: records per occurrence, their exclusive scan, the rows in arrival order
  std::vector<uint32_t> base(occs + 1, 0);
  for (uint64_t o = 0; o < occs; ++o) base[o + 1] = base[o] + ds_record_count(old_d[o], new_d[o], c[o]);
  std::vector<uint32_t> r_occ(base[occs]), r_deg(base[occs]);
  std::vector<int> r_delta(base[occs]);
  for (uint64_t o = 0; o < occs; ++o)
    for (uint32_t k = 0; k < base[o + 1] - base[o]; ++k) {
      r_occ[base[o] + k] = (uint32_t)o;
      ds_record(old_d[o], new_d[o], k, &r_deg[base[o] + k], &r_delta[base[o] + k]);
    }
  std::vector<uint32_t> c_before, c_after;
  ds_scan_parts(r_deg, r_delta, false, st.count, tile, &c_before, &c_after, &crossed);
  for (uint64_t o = 0; o < occs; ++o) rows->push_back(DsRow{v[o], old_d[o], new_d[o]});
  for (size_t r = 0; r < r_occ.size(); ++r) recs->push_back(DsRec{r_occ[r], r_deg[r], c_after[r]});
  return crossed;
}

}  // namespace gs
#endif  // GS_DEGSTREAM_SEQ_RULES_ONLY
