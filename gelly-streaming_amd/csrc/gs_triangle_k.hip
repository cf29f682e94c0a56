// gs_triangle_k.hip -- kernels of the triangle summary (gfx950).
//
//   k_tri_canon        : (src, dst) -> (min, max)
//   k_tri_flag_new     : over the fold's pairs sorted by (min, max): keep a pair that is no loop,
//                        differs from the pair before it and is not in A yet; count per tile
//   k_tri_compact_new  : the kept pairs in order: N, the fold's new edges; between a flag and
//                        a compact kernel, the sort's launch_tile_scan turns the tile counts
//                        into tile bases and the total
//   k_tri_reverse      : N's reverse entries (max, min), through the sort by max
//   k_tri_merge        : A' = merge(A, N, reverse N): every entry finds its position by binary
//                        search in the two other lists (gs_triangle_rows.hpp tri_merge_pos)
//   k_tri_rows         : per new edge: endpoints inserted into the relabel table, their rows in
//                        A', the edge binned by the length of its shorter row
//   k_tri_count        : the intersection, a lane group (8 or 64 lanes) per new edge
//   k_tri_count_lds    : the same with a workgroup per edge and 1024 samples of the longer row
//                        in LDS: the upper ten levels of every search stay on chip
//   k_tri_find / k_tri_flag_heads / k_tri_compact_rows / k_tri_rehash : reads of the counters,
//                        the sorted export (A's row heads are the vertices in order), growth
// Removal (gs_triangle_remove / _expire): the dying edges D and a dying byte per entry of A
//   k_tri_flag_new<true>  : the flag pass with the test turned round: keep a pair that IS in A,
//                        and set the dying byte of its two directed entries
//   k_tri_mark_old     : by age instead: the dying byte from the entry's stamp; D's entries are
//                        the dying ones with x < y, in A's order (k_tri_compact_new writes them)
//   k_tri_live_count / k_tri_live_pos : the survivors' positions (flag, tile scan, rank)
//   k_tri_vanish       : the rows without a survivor, counted before the host looks
//   k_tri_rows<true>   : D's rows in A as it stands; finds slots, inserts nothing; own lists
//   k_tri_count / k_tri_count_lds with TriDyingMark : the same walk, the counts taken away
//   k_tri_keep / k_tri_removed : the survivors into the other buffer; |G|, vertices, INT64_MIN
//   k_tri_restamp / k_tri_rebase : refresh behind a fold's count; the stamps at the wrap
//
// What bounds every loop:
//   * per-element passes handle kTriPer elements per thread, each index tested against n;
//   * every binary search halves an index interval inside its array (gs_triangle_rows.hpp);
//   * a row walk runs q from the row's first to its last index, both at most A.n, read from
//     TriRowInfo that k_tri_rows computed from the same A;
//   * list-driven loops run to min(list length word, n_new) and test each list element < n_new;
//   * table probes are gs_device.hpp's (at most cap + 1 steps);
//   * every output position is tested against the capacity of its array before the store.
// The removal's kernels add no other kind of loop:
//   * k_tri_mark_old, k_tri_live_count and k_tri_live_pos are per-element passes of kTriPer
//     elements per thread, each index tested against A.n; k_tri_vanish, k_tri_keep,
//     k_tri_restamp and k_tri_rebase handle one element per thread, tested against its count;
//   * their searches are gs_triangle_rows.hpp's (tri_pair_at, and tri_row_gone's one tri_upper
//     inside [i, A.n)); a dying byte or a stamp is stored only at an index a search returned,
//     which is below A.n; pos[] is read at i < A.n and at a row end below A.n;
//   * k_tri_rows<true> and the count kernels run the fold's loops over D, with the removal's own
//     list length words, each clamped to |D| (list_length);
//   * k_tri_keep tests pos[i] against the capacity of the other buffer before the store.
// Counters change by atomic adds only -- a removal adds the two's complement --; the count
// kernels read A and the table that earlier launches wrote, never a counter. The tile count and the rank inside a tile are gs_scan.hpp's.
#include "gs_scan.hpp"
#include "gs_triangle.hpp"
#include "gs_triangle_rows.hpp"

namespace gs {
namespace {

constexpr uint32_t kTriMinSlot = 0xFFFFFFFEu;  // "slot" of INT64_MIN: its words live in ctl

__device__ __forceinline__ unsigned long long* tri_counter(const Table& t, unsigned long long* ctl, uint32_t s) {
  return s == kTriMinSlot ? ctl + TRI_MINC : reinterpret_cast<unsigned long long*>(&t.tab[s].link);
}

__device__ __forceinline__ uint64_t tri_read(const Table& t, const unsigned long long* ctl, uint32_t s) {
  if (s == kTriMinSlot) return ctl[TRI_MINC];
  return *reinterpret_cast<const unsigned long long*>(&t.tab[s].link) - ((uint64_t)s << 1);
}

__device__ __forceinline__ uint32_t tri_find_slot(const Table& t, const unsigned long long* ctl, int64_t key) {
  if (key == kEmpty) return ctl[TRI_MINP] ? kTriMinSlot : kNoSlot;
  uint32_t link;
  return lookup_find(t, key, link);
}

__device__ __forceinline__ uint32_t tri_insert_slot(const Table& t, unsigned long long* ctl, int64_t key,
                                                    bool& fresh) {
  if (key == kEmpty) {
    fresh = atomicExch(ctl + TRI_MINP, 1ull) == 0ull;
    return kTriMinSlot;
  }
  uint32_t link;
  return lookup_insert(t, key, link, fresh);
}

__global__ __launch_bounds__(kTriBS) void k_tri_init(Table t) {
  const uint64_t s = (uint64_t)blockIdx.x * kTriBS + threadIdx.x;
  if (s > (uint64_t)t.r0) return;
  Slot v;
  v.key = kEmpty;
  v.link = (uint32_t)s << 1;
  v.aux = 0;
  t.tab[s] = v;
}

__global__ __launch_bounds__(kTriBS) void k_tri_canon(const int64_t* __restrict__ src, const int64_t* __restrict__ dst,
                                                      uint64_t n, uint64_t stride, int64_t* __restrict__ lo,
                                                      int64_t* __restrict__ hi) {
  const uint64_t base = (uint64_t)blockIdx.x * TRIANGLE_TILE;
#pragma unroll
  for (uint32_t k = 0; k < kTriPer; ++k) {
    const uint64_t i = base + k * kTriBS + threadIdx.x;
    if (i < n) {
      const int64_t s = __builtin_nontemporal_load(src + i * stride);
      const int64_t d = __builtin_nontemporal_load(dst + i * stride);
      lo[i] = s < d ? s : d;
      hi[i] = s < d ? d : s;
    }
  }
}

// kDying == false: keep the rows that are not in A (a fold's new edges). kDying: keep the rows
// that are in A (a removal's dying edges) and set dead[] of their two directed entries.
template <bool kDying>
__global__ __launch_bounds__(kTriBS) void k_tri_flag_new(const uint32_t* __restrict__ pay,
                                                         const int64_t* __restrict__ lo, const int64_t* __restrict__ hi,
                                                         uint64_t n, TriAdj A, uint8_t* __restrict__ flags,
                                                         uint32_t* __restrict__ blk, uint8_t* __restrict__ dead) {
  __shared__ uint32_t total;
  const uint64_t i0 = (uint64_t)blockIdx.x * TRIANGLE_TILE + threadIdx.x * kTriPer;
  uint32_t cnt = 0;
#pragma unroll
  for (uint32_t k = 0; k < kTriPer; ++k) {
    const uint64_t i = i0 + k;
    if (i >= n) continue;
    const uint64_t r = pay ? pay[i] : i;
    bool keep = false;
    if (r < n) {
      const int64_t a = lo[r], b = hi[r];
      keep = a != b;
      if (keep && i > 0) {
        const uint64_t rp = pay ? pay[i - 1] : i - 1;
        if (rp < n && lo[rp] == a && hi[rp] == b) keep = false;
      }
      if constexpr (kDying) {
        if (keep) {
          const uint64_t p = tri_pair_at(A.x, A.y, A.n, a, b);
          keep = p != kTriNone;
          if (keep) {
            dead[p] = 1;
            const uint64_t p2 = tri_pair_at(A.x, A.y, A.n, b, a);
            if (p2 != kTriNone) dead[p2] = 1;
          }
        }
      } else {
        if (keep && tri_has_pair(A.x, A.y, A.n, a, b)) keep = false;
      }
    }
    flags[i] = keep ? 1 : 0;
    cnt += keep ? 1u : 0u;
  }
  block_count_to<kTriBS>(cnt, &total, blk + blockIdx.x);
}

__global__ __launch_bounds__(kTriBS) void k_tri_compact_new(const uint32_t* __restrict__ pay,
                                                            const int64_t* __restrict__ lo,
                                                            const int64_t* __restrict__ hi, uint64_t n,
                                                            const uint8_t* __restrict__ flags,
                                                            const uint32_t* __restrict__ blk, int64_t* __restrict__ nx,
                                                            int64_t* __restrict__ ny, uint64_t cap) {
  __shared__ uint32_t wsum[kTriBS / 64];
  const uint64_t i0 = (uint64_t)blockIdx.x * TRIANGLE_TILE + threadIdx.x * kTriPer;
  uint32_t bits = 0;
#pragma unroll
  for (uint32_t k = 0; k < kTriPer; ++k)
    if (i0 + k < n && flags[i0 + k]) bits |= 1u << k;
  uint64_t pos = (uint64_t)blk[blockIdx.x] + block_excl_scan<kTriBS>((uint32_t)__popc(bits), wsum);
#pragma unroll
  for (uint32_t k = 0; k < kTriPer; ++k) {
    if (!(bits & (1u << k))) continue;
    const uint64_t r = pay ? pay[i0 + k] : i0 + k;
    if (pos < cap && r < n) {
      nx[pos] = lo[r];
      ny[pos] = hi[r];
    }
    ++pos;
  }
}

__global__ __launch_bounds__(kTriBS) void k_tri_reverse(const uint32_t* __restrict__ pay, const int64_t* __restrict__ nx,
                                                        const int64_t* __restrict__ ny, uint64_t n,
                                                        int64_t* __restrict__ rx, int64_t* __restrict__ ry) {
  const uint64_t j = (uint64_t)blockIdx.x * kTriBS + threadIdx.x;
  if (j >= n) return;
  const uint64_t r = pay ? pay[j] : j;
  if (r >= n) return;
  rx[j] = ny[r];
  ry[j] = nx[r];
}

__global__ __launch_bounds__(kTriBS) void k_tri_merge(TriAdj A, const int64_t* __restrict__ nx,
                                                      const int64_t* __restrict__ ny, const int64_t* __restrict__ rx,
                                                      const int64_t* __restrict__ ry, uint64_t m, TriAdjOut O,
                                                      uint32_t seq) {
  const uint64_t i = (uint64_t)blockIdx.x * kTriBS + threadIdx.x;
  if (i >= A.n + 2 * m) return;
  int64_t kx, ky;
  uint32_t s = seq;
  uint64_t pos;
  if (i < A.n) {
    kx = A.x[i];
    ky = A.y[i];
    s = A.seq[i];
    pos = tri_merge_pos(i, kx, ky, nx, ny, m, rx, ry, m);
  } else if (i < A.n + m) {
    const uint64_t j = i - A.n;
    kx = nx[j];
    ky = ny[j];
    pos = tri_merge_pos(j, kx, ky, A.x, A.y, A.n, rx, ry, m);
  } else {
    const uint64_t j = i - A.n - m;
    kx = rx[j];
    ky = ry[j];
    pos = tri_merge_pos(j, kx, ky, A.x, A.y, A.n, nx, ny, m);
  }
  if (pos < O.cap) {
    O.x[pos] = kx;
    O.y[pos] = ky;
    O.seq[pos] = s;
  }
}

// what a counter gains for c triangles counted: c, or its two's complement when they are destroyed
template <class Mark>
__device__ __forceinline__ unsigned long long tri_delta(unsigned long long c) {
  return Mark::kRemove ? 0ull - c : c;
}

// one append position per flagged lane of the wave with a single atomic on *ctr
__device__ __forceinline__ uint64_t wave_append(bool has, unsigned long long* ctr) {
  const unsigned long long m = __ballot(has);
  if (!m) return 0;  // wave-uniform
  const int lane = (int)(threadIdx.x & 63u);
  const int leader = __ffsll((long long)m) - 1;
  unsigned long long b = 0;
  if (lane == leader) b = atomicAdd(ctr, (unsigned long long)__popcll(m));
  const uint32_t blo = (uint32_t)__shfl((int)(uint32_t)b, leader, 64);
  const uint32_t bhi = (uint32_t)__shfl((int)(uint32_t)(b >> 32), leader, 64);
  return (((uint64_t)bhi << 32) | blo) + (uint64_t)__popcll(m & ((1ull << lane) - 1ull));
}

// kRemove: the edges are a removal's D, still in A: slots are found, nothing is inserted, and
// the lists and the steps go to the removal's own control words.
template <bool kRemove>
__global__ __launch_bounds__(kTriBS) void k_tri_rows(Table t, unsigned long long* __restrict__ ctl, TriAdj A,
                                                     const int64_t* __restrict__ nx, const int64_t* __restrict__ ny,
                                                     uint64_t m, TriRowInfo* __restrict__ info,
                                                     uint32_t* __restrict__ list1, uint32_t* __restrict__ list2,
                                                     int binned) {
  const uint64_t e = (uint64_t)blockIdx.x * kTriBS + threadIdx.x;
  const bool valid = e < m;
  bool fu = false, fv = false;
  uint32_t slen = 0, llen = 0;
  if (valid) {
    const int64_t u = nx[e], v = ny[e];
    uint64_t ub, ue, vb, ve;
    tri_row(A.x, A.n, u, &ub, &ue);
    tri_row(A.x, A.n, v, &vb, &ve);
    const uint32_t su = kRemove ? tri_find_slot(t, ctl, u) : tri_insert_slot(t, ctl, u, fu);
    const uint32_t sv = kRemove ? tri_find_slot(t, ctl, v) : tri_insert_slot(t, ctl, v, fv);
    const bool ushort = ue - ub <= ve - vb;
    TriRowInfo ri;
    ri.sb = (uint32_t)(ushort ? ub : vb);
    ri.se = (uint32_t)(ushort ? ue : ve);
    ri.lb = (uint32_t)(ushort ? vb : ub);
    ri.le = (uint32_t)(ushort ? ve : ue);
    ri.ss = ushort ? su : sv;
    ri.sl = ushort ? sv : su;
    info[e] = ri;
    slen = ri.se - ri.sb;
    llen = ri.le - ri.lb;
  }
  constexpr int kSteps = kRemove ? TRI_RSTEPS : TRI_STEPS;
  constexpr int kBin1 = kRemove ? TRI_RBIN1 : TRI_BIN1, kBin2 = kRemove ? TRI_RBIN2 : TRI_BIN2;
  if (!kRemove && e == 0) atomicAdd(ctl + TRI_E, (unsigned long long)m);  // the fold's edges join G here, with their rows
  // new vertices: one add per wave
  const uint32_t fresh = (uint32_t)__popcll(__ballot(fu)) + (uint32_t)__popcll(__ballot(fv));
  if (fresh && (threadIdx.x & 63u) == 0) atomicAdd(ctl + TRI_NV, (unsigned long long)fresh);
  // diagnostics: intersection steps and the hottest row
  uint64_t steps = slen;
  uint32_t hot = llen;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    steps += ((uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)(steps >> 32), o, 64) << 32) |
             (uint32_t)__shfl_xor((int)(uint32_t)steps, o, 64);
    const uint32_t h2 = (uint32_t)__shfl_xor((int)hot, o, 64);
    hot = h2 > hot ? h2 : hot;
  }
  if ((threadIdx.x & 63u) == 0 && steps) {
    atomicAdd(ctl + kSteps, (unsigned long long)steps);
    if (!kRemove) atomicMax(ctl + TRI_HOT, (unsigned long long)hot);
  }
  if (!binned) return;  // kernel-uniform
  const bool big = valid && slen > kTriWaveRow && llen >= kTriLdsRow;
  const bool mid = valid && slen > kTriShortRow && !big;
  const uint64_t p1 = wave_append(mid, ctl + kBin1);
  if (mid && p1 < m) list1[p1] = (uint32_t)e;
  const uint64_t p2 = wave_append(big, ctl + kBin2);
  if (big && p2 < m) list2[p2] = (uint32_t)e;
}

// The lanes of one group (lane of G) walk the shorter row of edge (u, v) and search each
// neighbour in the longer row; samp (optional, LDS): every step-th entry of the longer row.
// Returns the triangles this lane counted at the edge; t(w) is added here.
// Mark (gs_triangle.hpp) names the marked entries of A -- a fold's own, a removal's dying --:
// the triangle is counted at (u, v) iff each of its two other edges is unmarked or marked and
// before (u, v), so once, at the greatest marked edge. Mark::kRemove: t(w) loses the triangle.
template <uint32_t G, class Mark>
__device__ __forceinline__ uint32_t tri_walk(const Table& t, unsigned long long* ctl, const TriAdj& A,
                                             const TriRowInfo& ri, int64_t u, int64_t v, const Mark& mark,
                                             uint32_t lane, const int64_t* samp, uint32_t nsamp, uint32_t step) {
  if (ri.sb >= ri.se || ri.lb >= ri.le || ri.se > A.n || ri.le > A.n) return 0;
  const int64_t a = A.x[ri.sb], b = A.x[ri.lb];
  uint32_t cnt = 0;
  for (uint64_t q = (uint64_t)ri.sb + lane; q < ri.se; q += G) {
    const int64_t w = A.y[q];
    uint64_t lb = ri.lb, le = ri.le;
    if (samp) {
      const uint64_t c = tri_upper(samp, 0, nsamp, w);  // samples <= w
      if (c == 0) continue;                             // below the row's first entry
      lb = (uint64_t)ri.lb + (c - 1) * step;
      const uint64_t e2 = lb + step;
      le = e2 < le ? e2 : le;
    }
    const uint64_t p = tri_member(A.y, lb, le, w);
    if (p == kTriNone) continue;
    const bool ok1 = !mark.marked(q) || tri_edge_before(a, w, u, v);
    const bool ok2 = !mark.marked(p) || tri_edge_before(b, w, u, v);
    if (!(ok1 && ok2)) continue;
    ++cnt;
    const uint32_t sw = tri_find_slot(t, ctl, w);
    if (sw != kNoSlot) atomicAdd(tri_counter(t, ctl, sw), tri_delta<Mark>(1ull));
  }
  return cnt;
}

__device__ __forceinline__ uint64_t list_length(const unsigned long long* ctl, int word, uint64_t m) {
  const uint64_t c = ctl[word];
  return c < m ? c : m;
}

// G lanes per edge, kTriBS / G edges per workgroup and iteration. list == nullptr: every
// new edge whose shorter row has at most max_short entries; else the edges of the list.
// The edges are a fold's N (Mark = TriFoldMark) or a removal's D (TriDyingMark).
template <uint32_t G, class Mark>
__global__ __launch_bounds__(kTriBS) void k_tri_count(Table t, unsigned long long* __restrict__ ctl, TriAdj A,
                                                      const int64_t* __restrict__ nx, const int64_t* __restrict__ ny,
                                                      uint64_t m, const TriRowInfo* __restrict__ info,
                                                      const uint32_t* __restrict__ list, int list_word, Mark mark,
                                                      uint32_t max_short) {
  constexpr uint32_t kPer = kTriBS / G;
  const uint32_t g = threadIdx.x / G, lane = threadIdx.x % G;
  const uint64_t count = list ? list_length(ctl, list_word, m) : m;
  uint64_t tsum = 0;
  for (uint64_t base = (uint64_t)blockIdx.x * kPer; base < count; base += (uint64_t)gridDim.x * kPer) {  // block-uniform
    const uint64_t item = base + g;
    bool active = item < count;
    uint64_t e = 0;
    if (active) e = list ? list[item] : item;
    if (e >= m) active = false;
    TriRowInfo ri = {0, 0, 0, 0, kNoSlot, kNoSlot};
    if (active) ri = info[e];
    if (active && !list && ri.se - ri.sb > max_short) active = false;
    uint32_t c = 0;
    if (active) c = tri_walk<G>(t, ctl, A, ri, nx[e], ny[e], mark, lane, nullptr, 0, 0);
#pragma unroll
    for (int o = (int)G / 2; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if (lane == 0 && c) {
      if (ri.ss != kNoSlot) atomicAdd(tri_counter(t, ctl, ri.ss), tri_delta<Mark>(c));
      if (ri.sl != kNoSlot) atomicAdd(tri_counter(t, ctl, ri.sl), tri_delta<Mark>(c));
      tsum += c;
    }
  }
  // T: one add per wave
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
    tsum += ((uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)(tsum >> 32), o, 64) << 32) |
            (uint32_t)__shfl_xor((int)(uint32_t)tsum, o, 64);
  if ((threadIdx.x & 63u) == 0 && tsum) {
    atomicAdd(ctl + TRI_T, tri_delta<Mark>(tsum));
    if (Mark::kRemove) atomicAdd(ctl + TRI_RTRI, (unsigned long long)tsum);
  }
}

// a workgroup per listed edge; the longer row's samples in LDS
template <class Mark>
__global__ __launch_bounds__(kTriBS) void k_tri_count_lds(Table t, unsigned long long* __restrict__ ctl, TriAdj A,
                                                          const int64_t* __restrict__ nx,
                                                          const int64_t* __restrict__ ny, uint64_t m,
                                                          const TriRowInfo* __restrict__ info,
                                                          const uint32_t* __restrict__ list, Mark mark) {
  __shared__ int64_t samp[kTriSamples];
  __shared__ unsigned long long bsum;
  const uint64_t count = list_length(ctl, Mark::kRemove ? TRI_RBIN2 : TRI_BIN2, m);
  for (uint64_t item = blockIdx.x; item < count; item += gridDim.x) {  // block-uniform
    const uint64_t e = list[item];
    if (e >= m) continue;
    const TriRowInfo ri = info[e];
    const uint32_t llen = ri.le > ri.lb ? ri.le - ri.lb : 0;
    if (llen == 0 || ri.le > A.n) continue;  // (block-uniform: every thread read the same info)
    const uint32_t step = (llen + kTriSamples - 1) / kTriSamples;
    const uint32_t nsamp = (llen + step - 1) / step;  // <= kTriSamples
    if (threadIdx.x == 0) bsum = 0;
    for (uint32_t j = threadIdx.x; j < nsamp; j += kTriBS) samp[j] = A.y[(uint64_t)ri.lb + (uint64_t)j * step];
    __syncthreads();
    uint32_t c = tri_walk<kTriBS>(t, ctl, A, ri, nx[e], ny[e], mark, threadIdx.x, samp, nsamp, step);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63u) == 0 && c) atomicAdd(&bsum, (unsigned long long)c);
    __syncthreads();
    if (threadIdx.x == 0 && bsum) {
      if (ri.ss != kNoSlot) atomicAdd(tri_counter(t, ctl, ri.ss), tri_delta<Mark>(bsum));
      if (ri.sl != kNoSlot) atomicAdd(tri_counter(t, ctl, ri.sl), tri_delta<Mark>(bsum));
      atomicAdd(ctl + TRI_T, tri_delta<Mark>(bsum));
      if (Mark::kRemove) atomicAdd(ctl + TRI_RTRI, bsum);
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kTriBS) void k_tri_find(Table t, const unsigned long long* __restrict__ ctl,
                                                     const int64_t* __restrict__ v, uint64_t n,
                                                     int64_t* __restrict__ count, uint8_t* __restrict__ found) {
  const uint64_t i = (uint64_t)blockIdx.x * kTriBS + threadIdx.x;
  if (i >= n) return;
  const uint32_t s = tri_find_slot(t, ctl, v[i]);
  count[i] = s == kNoSlot ? 0 : (int64_t)tri_read(t, ctl, s);
  if (found) found[i] = s == kNoSlot ? 0 : 1;
}

__global__ __launch_bounds__(kTriBS) void k_tri_flag_heads(Table t, const unsigned long long* __restrict__ ctl,
                                                           TriAdj A, int nonzero, uint8_t* __restrict__ flags,
                                                           uint32_t* __restrict__ blk) {
  __shared__ uint32_t total;
  const uint64_t i0 = (uint64_t)blockIdx.x * TRIANGLE_TILE + threadIdx.x * kTriPer;
  uint32_t cnt = 0;
#pragma unroll
  for (uint32_t k = 0; k < kTriPer; ++k) {
    const uint64_t i = i0 + k;
    if (i >= A.n) continue;
    const int64_t v = A.x[i];
    bool head = i == 0 || A.x[i - 1] != v;
    if (head && nonzero) {
      const uint32_t s = tri_find_slot(t, ctl, v);
      head = s != kNoSlot && tri_read(t, ctl, s) != 0;
    }
    flags[i] = head ? 1 : 0;
    cnt += head ? 1u : 0u;
  }
  block_count_to<kTriBS>(cnt, &total, blk + blockIdx.x);
}

__global__ __launch_bounds__(kTriBS) void k_tri_compact_rows(Table t, const unsigned long long* __restrict__ ctl,
                                                             TriAdj A, const uint8_t* __restrict__ flags,
                                                             const uint32_t* __restrict__ blk, int64_t* __restrict__ ov,
                                                             int64_t* __restrict__ oc, uint64_t cap) {
  __shared__ uint32_t wsum[kTriBS / 64];
  const uint64_t i0 = (uint64_t)blockIdx.x * TRIANGLE_TILE + threadIdx.x * kTriPer;
  uint32_t bits = 0;
#pragma unroll
  for (uint32_t k = 0; k < kTriPer; ++k)
    if (i0 + k < A.n && flags[i0 + k]) bits |= 1u << k;
  uint64_t pos = (uint64_t)blk[blockIdx.x] + block_excl_scan<kTriBS>((uint32_t)__popc(bits), wsum);
#pragma unroll
  for (uint32_t k = 0; k < kTriPer; ++k) {
    if (!(bits & (1u << k))) continue;
    if (pos < cap) {
      const int64_t v = A.x[i0 + k];
      const uint32_t s = tri_find_slot(t, ctl, v);
      ov[pos] = v;
      oc[pos] = s == kNoSlot ? 0 : (int64_t)tri_read(t, ctl, s);
    }
    ++pos;
  }
}

__global__ __launch_bounds__(kTriBS) void k_tri_rehash(Table from, Table to, TriAdj A) {
  const uint64_t i = (uint64_t)blockIdx.x * kTriBS + threadIdx.x;
  if (i >= A.n) return;
  const int64_t v = A.x[i];
  if (v == kEmpty || (i > 0 && A.x[i - 1] == v)) return;
  uint32_t link;
  const uint32_t so = lookup_find(from, v, link);
  if (so == kNoSlot) return;
  const uint64_t c = *reinterpret_cast<const unsigned long long*>(&from.tab[so].link) - ((uint64_t)so << 1);
  bool fresh;
  const uint32_t sn = lookup_insert(to, v, link, fresh);
  if (sn != kNoSlot && c) atomicAdd(reinterpret_cast<unsigned long long*>(&to.tab[sn].link), (unsigned long long)c);
}

// ---- removal: the mark by age, the survivors' positions, the vanished rows, the compaction

__global__ __launch_bounds__(kTriBS) void k_tri_mark_old(TriAdj A, uint32_t cur, uint64_t folds,
                                                         uint8_t* __restrict__ dead, uint8_t* __restrict__ flags,
                                                         uint32_t* __restrict__ blk) {
  __shared__ uint32_t total;
  const uint64_t i0 = (uint64_t)blockIdx.x * TRIANGLE_TILE + threadIdx.x * kTriPer;
  uint32_t cnt = 0;
#pragma unroll
  for (uint32_t k = 0; k < kTriPer; ++k) {
    const uint64_t i = i0 + k;
    if (i >= A.n) continue;
    const bool old = tri_is_old(A.seq[i], cur, folds);
    const bool first = old && A.x[i] < A.y[i];
    dead[i] = old ? 1 : 0;
    flags[i] = first ? 1 : 0;
    cnt += first ? 1u : 0u;
  }
  block_count_to<kTriBS>(cnt, &total, blk + blockIdx.x);
}

__global__ __launch_bounds__(kTriBS) void k_tri_live_count(const uint8_t* __restrict__ dead, uint64_t n,
                                                           uint32_t* __restrict__ blk) {
  __shared__ uint32_t total;
  const uint64_t i0 = (uint64_t)blockIdx.x * TRIANGLE_TILE + threadIdx.x * kTriPer;
  uint32_t cnt = 0;
#pragma unroll
  for (uint32_t k = 0; k < kTriPer; ++k)
    if (i0 + k < n && !dead[i0 + k]) ++cnt;
  block_count_to<kTriBS>(cnt, &total, blk + blockIdx.x);
}

__global__ __launch_bounds__(kTriBS) void k_tri_live_pos(const uint8_t* __restrict__ dead, uint64_t n,
                                                         const uint32_t* __restrict__ blk, uint32_t* __restrict__ pos) {
  __shared__ uint32_t wsum[kTriBS / 64];
  const uint64_t i0 = (uint64_t)blockIdx.x * TRIANGLE_TILE + threadIdx.x * kTriPer;
  uint32_t bits = 0;
#pragma unroll
  for (uint32_t k = 0; k < kTriPer; ++k)
    if (i0 + k < n && !dead[i0 + k]) bits |= 1u << k;
  uint32_t p = blk[blockIdx.x] + block_excl_scan<kTriBS>((uint32_t)__popc(bits), wsum);
#pragma unroll
  for (uint32_t k = 0; k < kTriPer; ++k) {
    if (i0 + k < n) pos[i0 + k] = p;
    p += (bits >> k) & 1u;
  }
}

// A row vanishes when no entry of it survives: pos at its end equals pos at its head. A row
// whose head survives is not searched.
__global__ __launch_bounds__(kTriBS) void k_tri_vanish(TriAdj A, const uint8_t* __restrict__ dead,
                                                       const uint32_t* __restrict__ pos,
                                                       unsigned long long* __restrict__ ctl) {
  const uint64_t i = (uint64_t)blockIdx.x * kTriBS + threadIdx.x;
  bool gone = false;
  if (i < A.n && dead[i]) {
    const int64_t v = A.x[i];
    if (i == 0 || A.x[i - 1] != v) gone = tri_row_gone(A.x, A.n, i, pos, ctl[TRI_RLIVE]);
  }
  const uint32_t c = (uint32_t)__popcll(__ballot(gone));
  if (c && (threadIdx.x & 63u) == 0) atomicAdd(ctl + TRI_RVAN, (unsigned long long)c);
}

__global__ __launch_bounds__(kTriBS) void k_tri_keep(TriAdj A, const uint8_t* __restrict__ dead,
                                                     const uint32_t* __restrict__ pos, TriAdjOut O) {
  const uint64_t i = (uint64_t)blockIdx.x * kTriBS + threadIdx.x;
  if (i >= A.n || dead[i]) return;
  const uint64_t p = pos[i];
  if (p >= O.cap) return;
  O.x[p] = A.x[i];
  O.y[p] = A.y[i];
  O.seq[p] = A.seq[i];
}

// one thread: the words of G after the removal
__global__ void k_tri_removed(unsigned long long* __restrict__ ctl, const int64_t* __restrict__ ox, uint64_t n_live,
                              uint64_t n_dying) {
  if (blockIdx.x || threadIdx.x) return;
  ctl[TRI_E] -= n_dying;
  ctl[TRI_NV] -= ctl[TRI_RVAN];
  if (n_live == 0 || ox[0] != kEmpty) {  // INT64_MIN sorts first: it heads row 0 or none
    ctl[TRI_MINP] = 0;
    ctl[TRI_MINC] = 0;
  }
}

__global__ __launch_bounds__(kTriBS) void k_tri_restamp(const int64_t* __restrict__ lo, const int64_t* __restrict__ hi,
                                                        uint64_t n, TriAdj A, uint32_t* __restrict__ seq,
                                                        uint32_t cur) {
  const uint64_t i = (uint64_t)blockIdx.x * kTriBS + threadIdx.x;
  if (i >= n) return;
  const int64_t a = lo[i], b = hi[i];
  if (a == b) return;
  const uint64_t p = tri_pair_at(A.x, A.y, A.n, a, b);
  if (p != kTriNone) seq[p] = cur;
  const uint64_t p2 = tri_pair_at(A.x, A.y, A.n, b, a);
  if (p2 != kTriNone) seq[p2] = cur;
}

__global__ __launch_bounds__(kTriBS) void k_tri_rebase(uint32_t* __restrict__ seq, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * kTriBS + threadIdx.x;
  if (i >= n) return;
  seq[i] = tri_rebase(seq[i]);
}

uint32_t grid_of(uint64_t n) { return (uint32_t)((n + kTriBS - 1) / kTriBS); }

}  // namespace

void launch_tri_init(const Table& t, hipStream_t st) {
  hipLaunchKernelGGL(k_tri_init, dim3(grid_of((uint64_t)t.r0 + 1)), dim3(kTriBS), 0, st, t);
}

void launch_tri_canon(const int64_t* src, const int64_t* dst, uint64_t n, uint64_t stride, int64_t* lo, int64_t* hi,
                      hipStream_t st) {
  if (!n) return;
  hipLaunchKernelGGL(k_tri_canon, dim3((uint32_t)tri_blocks(n)), dim3(kTriBS), 0, st, src, dst, n, stride, lo, hi);
}

void launch_tri_flag_new(const uint32_t* pay, const int64_t* lo, const int64_t* hi, uint64_t n, const TriAdj& A,
                         uint8_t* flags, uint32_t* blk, hipStream_t st) {
  if (!n) return;
  hipLaunchKernelGGL(k_tri_flag_new<false>, dim3((uint32_t)tri_blocks(n)), dim3(kTriBS), 0, st, pay, lo, hi, n, A,
                     flags, blk, (uint8_t*)nullptr);
}

void launch_tri_flag_dying(const uint32_t* pay, const int64_t* lo, const int64_t* hi, uint64_t n, const TriAdj& A,
                           uint8_t* flags, uint32_t* blk, uint8_t* dead, hipStream_t st) {
  if (!n) return;
  hipLaunchKernelGGL(k_tri_flag_new<true>, dim3((uint32_t)tri_blocks(n)), dim3(kTriBS), 0, st, pay, lo, hi, n, A,
                     flags, blk, dead);
}

void launch_tri_mark_old(const TriAdj& A, uint32_t cur, uint64_t folds, uint8_t* dead, uint8_t* flags,
                         uint32_t* blk, hipStream_t st) {
  if (!A.n) return;
  hipLaunchKernelGGL(k_tri_mark_old, dim3((uint32_t)tri_blocks(A.n)), dim3(kTriBS), 0, st, A, cur, folds, dead, flags,
                     blk);
}

void launch_tri_live_count(const uint8_t* dead, uint64_t n, uint32_t* blk, hipStream_t st) {
  if (!n) return;
  hipLaunchKernelGGL(k_tri_live_count, dim3((uint32_t)tri_blocks(n)), dim3(kTriBS), 0, st, dead, n, blk);
}

void launch_tri_live_pos(const uint8_t* dead, uint64_t n, const uint32_t* blk, uint32_t* pos, hipStream_t st) {
  if (!n) return;
  hipLaunchKernelGGL(k_tri_live_pos, dim3((uint32_t)tri_blocks(n)), dim3(kTriBS), 0, st, dead, n, blk, pos);
}

void launch_tri_vanish(const TriAdj& A, const uint8_t* dead, const uint32_t* pos, unsigned long long* ctl,
                       hipStream_t st) {
  if (!A.n) return;
  hipLaunchKernelGGL(k_tri_vanish, dim3(grid_of(A.n)), dim3(kTriBS), 0, st, A, dead, pos, ctl);
}

void launch_tri_keep(const TriAdj& A, const uint8_t* dead, const uint32_t* pos, const TriAdjOut& O, hipStream_t st) {
  if (!A.n) return;
  hipLaunchKernelGGL(k_tri_keep, dim3(grid_of(A.n)), dim3(kTriBS), 0, st, A, dead, pos, O);
}

void launch_tri_removed(unsigned long long* ctl, const int64_t* ox, uint64_t n_live, uint64_t n_dying,
                        hipStream_t st) {
  hipLaunchKernelGGL(k_tri_removed, dim3(1), dim3(64), 0, st, ctl, ox, n_live, n_dying);
}

void launch_tri_restamp(const int64_t* lo, const int64_t* hi, uint64_t n, const TriAdj& A, uint32_t* seq,
                        uint32_t cur, hipStream_t st) {
  if (!n || !A.n) return;
  hipLaunchKernelGGL(k_tri_restamp, dim3(grid_of(n)), dim3(kTriBS), 0, st, lo, hi, n, A, seq, cur);
}

void launch_tri_rebase(uint32_t* seq, uint64_t n, hipStream_t st) {
  if (!n) return;
  hipLaunchKernelGGL(k_tri_rebase, dim3(grid_of(n)), dim3(kTriBS), 0, st, seq, n);
}

void launch_tri_compact_new(const uint32_t* pay, const int64_t* lo, const int64_t* hi, uint64_t n,
                            const uint8_t* flags, const uint32_t* blk, int64_t* nx, int64_t* ny, uint64_t cap,
                            hipStream_t st) {
  if (!n) return;
  hipLaunchKernelGGL(k_tri_compact_new, dim3((uint32_t)tri_blocks(n)), dim3(kTriBS), 0, st, pay, lo, hi, n, flags,
                     blk, nx, ny, cap);
}

void launch_tri_reverse(const uint32_t* pay, const int64_t* nx, const int64_t* ny, uint64_t n, int64_t* rx,
                        int64_t* ry, hipStream_t st) {
  if (!n) return;
  hipLaunchKernelGGL(k_tri_reverse, dim3(grid_of(n)), dim3(kTriBS), 0, st, pay, nx, ny, n, rx, ry);
}

void launch_tri_merge(const TriAdj& A, const int64_t* nx, const int64_t* ny, const int64_t* rx, const int64_t* ry,
                      uint64_t n_new, const TriAdjOut& O, uint32_t seq, hipStream_t st) {
  const uint64_t total = A.n + 2 * n_new;
  if (!total) return;
  hipLaunchKernelGGL(k_tri_merge, dim3(grid_of(total)), dim3(kTriBS), 0, st, A, nx, ny, rx, ry, n_new, O, seq);
}

void launch_tri_rows(const Table& t, unsigned long long* ctl, const TriAdj& A, const int64_t* nx, const int64_t* ny,
                     uint64_t n_new, TriRowInfo* info, uint32_t* list1, uint32_t* list2, int variant,
                     hipStream_t st) {
  if (!n_new) return;
  hipLaunchKernelGGL(k_tri_rows<false>, dim3(grid_of(n_new)), dim3(kTriBS), 0, st, t, ctl, A, nx, ny, n_new, info,
                     list1, list2, variant == kTriangleBinned ? 1 : 0);
}

void launch_tri_rows_dying(const Table& t, unsigned long long* ctl, const TriAdj& A, const int64_t* dx,
                           const int64_t* dy, uint64_t n_dying, TriRowInfo* info, uint32_t* list1, uint32_t* list2,
                           int variant, hipStream_t st) {
  if (!n_dying) return;
  hipLaunchKernelGGL(k_tri_rows<true>, dim3(grid_of(n_dying)), dim3(kTriBS), 0, st, t, ctl, A, dx, dy, n_dying, info,
                     list1, list2, variant == kTriangleBinned ? 1 : 0);
}

namespace {

// the count step over the edges (nx, ny): a fold's with TriFoldMark, a removal's with TriDyingMark
template <class Mark>
void launch_count_with(const Table& t, unsigned long long* ctl, const TriAdj& A, const int64_t* nx, const int64_t* ny,
                       uint64_t n_new, const TriRowInfo* info, const uint32_t* list1, const uint32_t* list2,
                       const Mark& mark, int variant, hipStream_t st) {
  if (!n_new) return;
  const auto grid = [](uint64_t items, uint32_t per, uint32_t most) {
    const uint64_t b = (items + per - 1) / per;
    return dim3((uint32_t)(b < most ? b : most));
  };
  if (variant == kTriangleWave) {
    hipLaunchKernelGGL((k_tri_count<64, Mark>), grid(n_new, kTriBS / 64, 1u << 16), dim3(kTriBS), 0, st, t, ctl, A, nx,
                       ny, n_new, info, (const uint32_t*)nullptr, 0, mark, 0xFFFFFFFFu);
    return;
  }
  hipLaunchKernelGGL((k_tri_count<TRIANGLE_LANES, Mark>), grid(n_new, kTriBS / TRIANGLE_LANES, 1u << 16), dim3(kTriBS),
                     0, st, t, ctl, A, nx, ny, n_new, info, (const uint32_t*)nullptr, 0, mark, kTriShortRow);
  hipLaunchKernelGGL((k_tri_count<64, Mark>), grid(n_new, kTriBS / 64, 4096), dim3(kTriBS), 0, st, t, ctl, A, nx, ny,
                     n_new, info, list1, (int)(Mark::kRemove ? TRI_RBIN1 : TRI_BIN1), mark, 0xFFFFFFFFu);
  hipLaunchKernelGGL(k_tri_count_lds<Mark>, grid(n_new, 1, 1024), dim3(kTriBS), 0, st, t, ctl, A, nx, ny, n_new, info,
                     list2, mark);
}

}  // namespace

void launch_tri_count(const Table& t, unsigned long long* ctl, const TriAdj& A, const int64_t* nx, const int64_t* ny,
                      uint64_t n_new, const TriRowInfo* info, const uint32_t* list1, const uint32_t* list2,
                      uint32_t seq, int variant, hipStream_t st) {
  launch_count_with(t, ctl, A, nx, ny, n_new, info, list1, list2, TriFoldMark{A.seq, seq}, variant, st);
}

void launch_tri_uncount(const Table& t, unsigned long long* ctl, const TriAdj& A, const uint8_t* dead,
                        const int64_t* dx, const int64_t* dy, uint64_t n_dying, const TriRowInfo* info,
                        const uint32_t* list1, const uint32_t* list2, int variant, hipStream_t st) {
  launch_count_with(t, ctl, A, dx, dy, n_dying, info, list1, list2, TriDyingMark{dead}, variant, st);
}

void launch_tri_find(const Table& t, const unsigned long long* ctl, const int64_t* v, uint64_t n, int64_t* count,
                     uint8_t* found, hipStream_t st) {
  if (!n) return;
  hipLaunchKernelGGL(k_tri_find, dim3(grid_of(n)), dim3(kTriBS), 0, st, t, ctl, v, n, count, found);
}

void launch_tri_flag_heads(const Table& t, const unsigned long long* ctl, const TriAdj& A, int nonzero,
                           uint8_t* flags, uint32_t* blk, hipStream_t st) {
  if (!A.n) return;
  hipLaunchKernelGGL(k_tri_flag_heads, dim3((uint32_t)tri_blocks(A.n)), dim3(kTriBS), 0, st, t, ctl, A, nonzero,
                     flags, blk);
}

void launch_tri_compact_rows(const Table& t, const unsigned long long* ctl, const TriAdj& A, const uint8_t* flags,
                             const uint32_t* blk, int64_t* ov, int64_t* oc, uint64_t cap, hipStream_t st) {
  if (!A.n) return;
  hipLaunchKernelGGL(k_tri_compact_rows, dim3((uint32_t)tri_blocks(A.n)), dim3(kTriBS), 0, st, t, ctl, A, flags, blk,
                     ov, oc, cap);
}

void launch_tri_rehash(const Table& from, const Table& to, const TriAdj& A, hipStream_t st) {
  if (!A.n) return;
  hipLaunchKernelGGL(k_tri_rehash, dim3(grid_of(A.n)), dim3(kTriBS), 0, st, from, to, A);
}

}  // namespace gs
