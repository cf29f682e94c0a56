// gs_tristream_k.hip -- kernels of the triangle streams (gfx950, wave size 64).
//
//   k_trs_compact_new : the flagged run heads of the sorted arrivals in order: the new pairs with
//                       the number of their arrival as stamp; is_new per arrival
//   k_trs_reverse     : the new pairs' reverse entries, through the sort by max
//   k_trs_merge       : A' = merge(A, N, reverse N) with stamps: every entry finds its position by
//                       binary search in the two other lists (gs_triangle_rows.hpp tri_merge_pos)
//   k_trs_head_count / k_trs_head_write : the row heads of an adjacency: the vertices of G in order
//   k_trs_rows        : per arrival the rows of its endpoints in A', the shorter one to be walked
//   k_trs_walk<WRITE, G> : the filtered intersection. A group of G lanes owns G arrivals, one per
//                       lane, and takes those with work one after the other: it walks the shorter
//                       row in chunks of G entries, every lane searches its entry in the longer
//                       row and tests both stamps; a ballot cut to the group counts the hits
//                       (count pass) and the prefix popcount places them in the row's ascending
//                       order (write pass). G = 8 for walked rows of at most 32 entries, else 64
//   k_trs_arr_reduce / k_trs_carry / k_trs_arr_apply : the scan over the arrivals: rows, offsets
//   k_trs_seg_reduce / k_trs_carry / k_trs_seg_apply / k_trs_commit : the seeded segmented sum over
//                       the records sorted by rank; the tails become the counters
//   k_trs_live_count / k_trs_live_write : the vertices with t > 0, compacted in A's row order
// The stamp test, the record layout and the segmented combine are gs_tristream_seq.hpp's; the
// tile count, the rank inside a tile and the block-wide segmented scan are gs_scan.hpp's.
//
// Concurrency. No atomics carry data: the only atomics are the error flag, the diagnostics and
// the crossed-tile counter, read by the host after the fold. The apply kernels read the counters
// and never write them; k_trs_commit, a later launch, stores one counter per segment. Nobody waits.
//
// What bounds every loop:
//   * per-element passes handle one element, or kTrsPer / kTriPer consecutive ones, per thread,
//     each index tested against n; the neighbours j - 1 and j + 1 of a position are read only
//     inside [0, n);
//   * every binary search halves an index interval inside its array (gs_triangle_rows.hpp);
//   * a row walk runs from the row's first to its last index in steps of G, both at most A.n,
//     read from TrsRowInfo that k_trs_rows computed from the same A and tested against A.n again;
//   * a group's loop over its arrivals clears one bit of a 64-bit ballot per step;
//   * a sort payload is tested against the row count, a rank against the counters' capacity
//     (TRS_ERR is raised, the position reads seed 0 and stores nothing) before it is an index;
//   * every output position is tested against the capacity of its array before the store;
//   * k_trs_carry's loop runs ceil(tiles / kTrsBS) times.
#include "gs_scan.hpp"
#include "gs_sort.hpp"
#include "gs_triangle_rows.hpp"
#include "gs_tristream.hpp"

namespace gs {
namespace {

__device__ __forceinline__ void raise_err(unsigned long long* ctl) { atomicOr(ctl + TRS_ERR, 1ull); }

__device__ __forceinline__ uint32_t shfl_u32(uint32_t x, int lane) { return (uint32_t)__shfl((int)x, lane, 64); }

// ---- the new pairs
__global__ __launch_bounds__(kTriBS) void k_trs_compact_new(const uint32_t* __restrict__ pay,
                                                            const int64_t* __restrict__ lo,
                                                            const int64_t* __restrict__ hi, uint64_t n,
                                                            const uint8_t* __restrict__ flags,
                                                            const uint32_t* __restrict__ blk, uint64_t t0,
                                                            int64_t* __restrict__ nx, int64_t* __restrict__ ny,
                                                            uint32_t* __restrict__ nfirst, uint8_t* __restrict__ is_new,
                                                            uint64_t cap) {
  __shared__ uint32_t wsum[kTriBS / 64];
  const uint64_t i0 = (uint64_t)blockIdx.x * TRIANGLE_TILE + threadIdx.x * kTriPer;
  uint32_t bits = 0;
#pragma unroll
  for (uint32_t k = 0; k < kTriPer; ++k)
    if (i0 + k < n && flags[i0 + k]) bits |= 1u << k;
  uint64_t pos = (uint64_t)blk[blockIdx.x] + block_excl_scan<kTriBS>((uint32_t)__popc(bits), wsum);
#pragma unroll
  for (uint32_t k = 0; k < kTriPer; ++k) {
    if (i0 + k >= n) continue;
    const uint64_t r = pay ? pay[i0 + k] : i0 + k;
    if (r >= n) continue;
    const bool keep = (bits & (1u << k)) != 0;
    is_new[r] = keep ? 1 : 0;
    if (!keep) continue;
    if (pos < cap) {
      nx[pos] = lo[r];
      ny[pos] = hi[r];
      nfirst[pos] = trs_arrival_no(t0, r);
    }
    ++pos;
  }
}

__global__ __launch_bounds__(kTrsBS) void k_trs_reverse(const uint32_t* __restrict__ pay, const int64_t* __restrict__ nx,
                                                        const int64_t* __restrict__ ny,
                                                        const uint32_t* __restrict__ nfirst, uint64_t m,
                                                        int64_t* __restrict__ rx, int64_t* __restrict__ ry,
                                                        uint32_t* __restrict__ rfirst) {
  const uint64_t j = (uint64_t)blockIdx.x * kTrsBS + threadIdx.x;
  if (j >= m) return;
  const uint64_t r = pay ? pay[j] : j;
  if (r >= m) return;
  rx[j] = ny[r];
  ry[j] = nx[r];
  rfirst[j] = nfirst[r];
}

__global__ __launch_bounds__(kTrsBS) void k_trs_merge(TrsAdj A, const int64_t* __restrict__ nx,
                                                      const int64_t* __restrict__ ny,
                                                      const uint32_t* __restrict__ nfirst, const int64_t* __restrict__ rx,
                                                      const int64_t* __restrict__ ry,
                                                      const uint32_t* __restrict__ rfirst, uint64_t m, TrsAdjOut O) {
  const uint64_t i = (uint64_t)blockIdx.x * kTrsBS + threadIdx.x;
  if (i >= A.n + 2 * m) return;
  int64_t kx, ky;
  uint32_t f;
  uint64_t pos;
  if (i < A.n) {
    kx = A.x[i];
    ky = A.y[i];
    f = A.first[i];
    pos = tri_merge_pos(i, kx, ky, nx, ny, m, rx, ry, m);
  } else if (i < A.n + m) {
    const uint64_t j = i - A.n;
    kx = nx[j];
    ky = ny[j];
    f = nfirst[j];
    pos = tri_merge_pos(j, kx, ky, A.x, A.y, A.n, rx, ry, m);
  } else {
    const uint64_t j = i - A.n - m;
    kx = rx[j];
    ky = ry[j];
    f = rfirst[j];
    pos = tri_merge_pos(j, kx, ky, A.x, A.y, A.n, nx, ny, m);
  }
  if (pos < O.cap) {
    O.x[pos] = kx;
    O.y[pos] = ky;
    O.first[pos] = f;
  }
}

// ---- row heads
__device__ __forceinline__ uint32_t head_bits(const int64_t* __restrict__ x, uint64_t n, uint64_t i0) {
  uint32_t bits = 0;
#pragma unroll
  for (uint32_t k = 0; k < kTrsPer; ++k) {
    const uint64_t i = i0 + k;
    if (i < n && (i == 0 || x[i - 1] != x[i])) bits |= 1u << k;
  }
  return bits;
}

__global__ __launch_bounds__(kTrsBS) void k_trs_head_count(const int64_t* __restrict__ x, uint64_t n,
                                                           uint32_t* __restrict__ blk) {
  __shared__ uint32_t total;
  const uint64_t i0 = (uint64_t)blockIdx.x * TRISTREAM_TILE + (uint64_t)threadIdx.x * kTrsPer;
  block_count_to<kTrsBS>((uint32_t)__popc(head_bits(x, n, i0)), &total, blk + blockIdx.x);
}

__global__ __launch_bounds__(kTrsBS) void k_trs_head_write(const int64_t* __restrict__ x, uint64_t n,
                                                           const uint32_t* __restrict__ blk, int64_t* __restrict__ out,
                                                           uint64_t cap) {
  __shared__ uint32_t wsum[kTrsBS / 64];
  const uint64_t i0 = (uint64_t)blockIdx.x * TRISTREAM_TILE + (uint64_t)threadIdx.x * kTrsPer;
  const uint32_t bits = head_bits(x, n, i0);
  uint64_t pos = (uint64_t)blk[blockIdx.x] + block_excl_scan<kTrsBS>((uint32_t)__popc(bits), wsum);
#pragma unroll
  for (uint32_t k = 0; k < kTrsPer; ++k) {
    if (!(bits & (1u << k))) continue;
    if (pos < cap) out[pos] = x[i0 + k];
    ++pos;
  }
}

// ---- rows
__global__ __launch_bounds__(kTrsBS) void k_trs_rows(TrsAdj A, const int64_t* __restrict__ lo,
                                                     const int64_t* __restrict__ hi, const uint8_t* __restrict__ is_new,
                                                     uint64_t n, TrsRowInfo* __restrict__ info,
                                                     unsigned long long* __restrict__ ctl) {
  const uint64_t a = (uint64_t)blockIdx.x * kTrsBS + threadIdx.x;
  uint64_t steps = 0;
  uint32_t hot = 0;
  if (a < n) {
    TrsRowInfo ri = {0, 0, 0, 0};
    const int64_t u = lo[a], v = hi[a];
    if (u != v && !(is_new && !is_new[a])) {
      uint64_t ub, ue, vb, ve, sb, se, lb, le;
      tri_row(A.x, A.n, u, &ub, &ue);
      tri_row(A.x, A.n, v, &vb, &ve);
      trs_pick_rows(ub, ue, vb, ve, &sb, &se, &lb, &le);
      ri.sb = (uint32_t)sb;
      ri.se = (uint32_t)se;
      ri.lb = (uint32_t)lb;
      ri.le = (uint32_t)le;
      steps = se - sb;
      hot = (uint32_t)(le - lb);
    }
    info[a] = ri;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    steps += ((uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)(steps >> 32), o, 64) << 32) |
             (uint32_t)__shfl_xor((int)(uint32_t)steps, o, 64);
    const uint32_t h2 = (uint32_t)__shfl_xor((int)hot, o, 64);
    hot = h2 > hot ? h2 : hot;
  }
  if ((threadIdx.x & 63u) == 0 && steps) {
    atomicAdd(ctl + TRS_STEPS, (unsigned long long)steps);
    atomicMax(ctl + TRS_HOT, (unsigned long long)hot);
  }
}

// ---- the filtered intersection
// A group of G lanes owns G arrivals, one per lane, and takes those of its bin that have work one
// after the other: G = TRISTREAM_LANES for walked rows of at most kTrsShortRow entries (eight
// arrivals of a wave in flight), G = 64 for longer ones. The loops are uniform inside a group; a
// ballot is cut to the group's own lanes, so what other groups of the wave do never shows.
template <bool WRITE, uint32_t G>
__global__ __launch_bounds__(kTrsBS) void k_trs_walk(TrsAdj A, const TrsRowInfo* __restrict__ info,
                                                     const int64_t* __restrict__ lo, const int64_t* __restrict__ hi,
                                                     uint64_t n, uint64_t t0, uint32_t* __restrict__ cnt,
                                                     const uint32_t* __restrict__ roff, uint32_t* __restrict__ r_arr,
                                                     int64_t* __restrict__ r_v, uint32_t* __restrict__ r_delta,
                                                     uint64_t cap, unsigned long long* __restrict__ ctl) {
  static_assert(kTrsWaveArrivals == 64, "one arrival per lane");
  static_assert(G == 64 || (G < 64 && 64 % G == 0), "whole groups in a wave");
  const int lane = (int)(threadIdx.x & 63u);
  const uint32_t gl = (uint32_t)lane % G;
  const unsigned long long gmask = G == 64 ? ~0ull : ((1ull << (G & 63u)) - 1ull) << ((uint32_t)lane - gl);
  const uint64_t wave = (uint64_t)blockIdx.x * (kTrsBS / 64) + (threadIdx.x >> 6);
  const uint64_t a = wave * kTrsWaveArrivals + (uint64_t)lane;
  TrsRowInfo ri = {0, 0, 0, 0};
  uint32_t want = 0, off = 0;
  if (a < n) {
    ri = info[a];
    if (WRITE) {
      want = cnt[a];
      off = roff[a];
    }
  }
  const bool is_short = ri.se - ri.sb <= kTrsShortRow;  // (an empty row is a short one)
  const bool my_bin = a < n && ri.se >= ri.sb && (G == 64 ? !is_short : is_short);
  bool work = my_bin && ri.se > ri.sb && ri.le > ri.lb && (!WRITE || want > 0);
  if (work && (ri.se > A.n || ri.le > A.n)) {
    raise_err(ctl);
    work = false;
  }
  uint32_t mine = 0;
  bool bad = false;
  for (unsigned long long todo = __ballot(work) & gmask; todo; todo &= todo - 1) {  // group-uniform
    const int b = __ffsll((long long)todo) - 1;
    const uint32_t sb = shfl_u32(ri.sb, b), se = shfl_u32(ri.se, b), lb = shfl_u32(ri.lb, b), le = shfl_u32(ri.le, b);
    const uint64_t ab = wave * kTrsWaveArrivals + (uint64_t)b;
    const uint32_t t = trs_arrival_no(t0, ab);
    const uint64_t base = WRITE ? (uint64_t)shfl_u32(off, b) : 0;
    uint32_t hits = 0;
    for (uint64_t q0 = sb; q0 < se; q0 += G) {
      const uint64_t q = q0 + (uint64_t)gl;
      const bool hit = q < se && trs_hit(A.y, A.first, q, lb, le, t);
      const unsigned long long m = __ballot(hit) & gmask;
      if (WRITE && hit) {
        const uint64_t pos = base + hits + (uint64_t)__popcll(m & ((1ull << lane) - 1ull));
        if (pos < cap) {
          r_arr[pos] = (uint32_t)ab;
          r_v[pos] = A.y[q];
          r_delta[pos] = trs_record_delta(0, 1);
        } else {
          bad = true;
        }
      }
      hits += (uint32_t)__popcll(m);
    }
    if (!WRITE) {
      if (lane == b) mine = hits;
    } else if (lane == b) {
      // u, then v, each with delta c; the count pass and this one read the same A
      const uint64_t pos = base + hits;
      if (hits != want || pos + 1 >= cap) {
        bad = true;
      } else {
        r_arr[pos] = (uint32_t)ab;
        r_v[pos] = lo[ab];
        r_delta[pos] = trs_record_delta(hits, hits);
        r_arr[pos + 1] = (uint32_t)ab;
        r_v[pos + 1] = hi[ab];
        r_delta[pos + 1] = trs_record_delta(hits + 1, hits);
      }
    }
  }
  if (bad) raise_err(ctl);
  if (!WRITE && my_bin) cnt[a] = mine;
}

// ---- the scan over the arrivals
__device__ __forceinline__ TrsSeg arr_element(uint32_t c, uint64_t j) {
  return trs_seg_element((int64_t)c, (int64_t)trs_record_count(c), j == 0);
}

__global__ __launch_bounds__(kTrsBS) void k_trs_arr_reduce(const uint32_t* __restrict__ cnt, uint64_t n,
                                                           TrsSeg* __restrict__ agg) {
  __shared__ TrsSeg wagg[kTrsBS / 64];
  const uint64_t j0 = (uint64_t)blockIdx.x * TRISTREAM_TILE + (uint64_t)threadIdx.x * kTrsPer;
  TrsSeg s = trs_seg_identity();
#pragma unroll
  for (uint32_t k = 0; k < kTrsPer; ++k)
    if (j0 + k < n) s = trs_seg_combine(s, arr_element(cnt[j0 + k], j0 + k));
  TrsSeg total;
  (void)block_seg_excl<kTrsBS, TrsSegOps>(s, wagg, &total);
  if (threadIdx.x == 0) agg[blockIdx.x] = total;
}

// one workgroup: the exclusive scan of the tile aggregates; sums (may be null): the two sums of
// everything, side by side
__global__ __launch_bounds__(kTrsBS) void k_trs_carry(const TrsSeg* __restrict__ agg, TrsSeg* __restrict__ carry,
                                                      uint64_t tiles, unsigned long long* __restrict__ sums) {
  __shared__ TrsSeg wagg[kTrsBS / 64];
  TrsSeg run = trs_seg_identity();
  for (uint64_t t0 = 0; t0 < tiles; t0 += kTrsBS) {
    const uint64_t t = t0 + threadIdx.x;
    const TrsSeg mine = t < tiles ? agg[t] : trs_seg_identity();
    TrsSeg total;
    const TrsSeg excl = block_seg_excl<kTrsBS, TrsSegOps>(mine, wagg, &total);
    if (t < tiles) carry[t] = trs_seg_combine(run, excl);
    run = trs_seg_combine(run, total);
    __syncthreads();  // wagg is written again
  }
  if (sums && threadIdx.x == 0) {
    sums[0] = (unsigned long long)run.a;
    sums[1] = (unsigned long long)run.b;
  }
}

__global__ __launch_bounds__(kTrsBS) void k_trs_arr_apply(const uint32_t* __restrict__ cnt, uint64_t n,
                                                          const TrsSeg* __restrict__ carry, int64_t total0,
                                                          uint32_t* __restrict__ closed, int64_t* __restrict__ total,
                                                          uint32_t* __restrict__ roff) {
  __shared__ TrsSeg wagg[kTrsBS / 64];
  const uint64_t j0 = (uint64_t)blockIdx.x * TRISTREAM_TILE + (uint64_t)threadIdx.x * kTrsPer;
  uint32_t c[kTrsPer];
  TrsSeg s = trs_seg_identity();
#pragma unroll
  for (uint32_t k = 0; k < kTrsPer; ++k) {
    c[k] = j0 + k < n ? cnt[j0 + k] : 0u;
    if (j0 + k < n) s = trs_seg_combine(s, arr_element(c[k], j0 + k));
  }
  TrsSeg all;
  TrsSeg in = block_seg_excl<kTrsBS, TrsSegOps>(s, wagg, &all);
  const TrsSeg cin = carry[blockIdx.x];
#pragma unroll
  for (uint32_t k = 0; k < kTrsPer; ++k) {
    const uint64_t j = j0 + k;
    if (j >= n) continue;
    roff[j] = j == 0 ? 0u : (uint32_t)trs_seg_combine(cin, in).b;
    in = trs_seg_combine(in, arr_element(c[k], j));
    closed[j] = c[k];
    total[j] = trs_seg_after(trs_seg_combine(cin, in), total0);
  }
}

// ---- the seeded segmented sum over the records
struct TrsMine {
  uint32_t idx[kTrsPer];  // the key's low 32 bits: the rank
  uint32_t pay[kTrsPer];
  uint32_t d[kTrsPer];
  uint32_t head, live;  // bit k: position k is a segment head / below n
};

__device__ __forceinline__ void load_mine(const unsigned long long* __restrict__ skey, const uint32_t* __restrict__ spay,
                                          const uint32_t* __restrict__ delta, uint64_t n, uint64_t j0, TrsMine& m) {
  m.head = m.live = 0;
  unsigned long long prev = 0;
  if (j0 > 0 && j0 - 1 < n) prev = skey[j0 - 1];
#pragma unroll
  for (uint32_t k = 0; k < kTrsPer; ++k) {
    const uint64_t j = j0 + k;
    m.idx[k] = 0;
    m.pay[k] = 0;
    m.d[k] = 0;
    if (j < n) {
      const unsigned long long x = skey[j];
      const uint32_t p = spay[j];
      m.live |= 1u << k;
      m.idx[k] = (uint32_t)x;
      m.pay[k] = p;
      m.d[k] = p < n ? delta[p] : 0u;
      if (j == 0 || x != prev) m.head |= 1u << k;
      prev = x;
    }
  }
}

__device__ __forceinline__ TrsSeg reduce_mine(const TrsMine& m) {
  TrsSeg s = trs_seg_identity();
#pragma unroll
  for (uint32_t k = 0; k < kTrsPer; ++k)
    if ((m.live >> k) & 1u) s = trs_seg_combine(s, trs_seg_element((int64_t)m.d[k], 0, ((m.head >> k) & 1u) != 0));
  return s;
}

__global__ __launch_bounds__(kTrsBS) void k_trs_seg_reduce(const unsigned long long* __restrict__ skey,
                                                           const uint32_t* __restrict__ spay,
                                                           const uint32_t* __restrict__ delta, uint64_t n,
                                                           TrsSeg* __restrict__ agg, unsigned long long* __restrict__ ctl) {
  __shared__ TrsSeg wagg[kTrsBS / 64];
  const uint64_t j0 = (uint64_t)blockIdx.x * TRISTREAM_TILE + (uint64_t)threadIdx.x * kTrsPer;
  TrsMine m;
  load_mine(skey, spay, delta, n, j0, m);
  TrsSeg total;
  (void)block_seg_excl<kTrsBS, TrsSegOps>(reduce_mine(m), wagg, &total);
  if (threadIdx.x == 0) {
    agg[blockIdx.x] = total;
    if (blockIdx.x > 0 && !(m.head & 1u)) atomicAdd(ctl + TRS_CROSSED, 1ull);
  }
}

__global__ __launch_bounds__(kTrsBS) void k_trs_seg_apply(const unsigned long long* __restrict__ skey,
                                                          const uint32_t* __restrict__ spay,
                                                          const uint32_t* __restrict__ delta, uint64_t n,
                                                          const TrsSeg* __restrict__ carry,
                                                          const int64_t* __restrict__ counter, uint64_t rank_cap,
                                                          int64_t* __restrict__ count, unsigned long long* __restrict__ ctl) {
  __shared__ TrsSeg wagg[kTrsBS / 64];
  const uint64_t j0 = (uint64_t)blockIdx.x * TRISTREAM_TILE + (uint64_t)threadIdx.x * kTrsPer;
  TrsMine m;
  load_mine(skey, spay, delta, n, j0, m);
  TrsSeg total;
  TrsSeg in = block_seg_excl<kTrsBS, TrsSegOps>(reduce_mine(m), wagg, &total);
  const TrsSeg cin = carry[blockIdx.x];
  bool bad = false;
#pragma unroll
  for (uint32_t k = 0; k < kTrsPer; ++k) {
    if (!((m.live >> k) & 1u)) continue;
    in = trs_seg_combine(in, trs_seg_element((int64_t)m.d[k], 0, ((m.head >> k) & 1u) != 0));
    if (m.idx[k] < rank_cap && m.pay[k] < n)
      count[m.pay[k]] = trs_seg_after(trs_seg_combine(cin, in), counter[m.idx[k]]);
    else
      bad = true;
  }
  if (bad) raise_err(ctl);
}

// the tail of every segment: its count is its vertex's counter from here on
__global__ __launch_bounds__(kTrsBS) void k_trs_commit(const unsigned long long* __restrict__ skey,
                                                       const uint32_t* __restrict__ spay, uint64_t n,
                                                       const int64_t* __restrict__ count, int64_t* __restrict__ counter,
                                                       uint64_t rank_cap) {
  const uint64_t j = (uint64_t)blockIdx.x * kTrsBS + threadIdx.x;
  if (j >= n) return;
  const unsigned long long x = skey[j];
  if (j + 1 < n && skey[j + 1] == x) return;
  const uint32_t idx = (uint32_t)x, p = spay[j];
  if (idx < rank_cap && p < n) counter[idx] = count[p];
}

// ---- the export
__device__ __forceinline__ uint32_t live_bits(const int64_t* __restrict__ rank, uint64_t n,
                                              const int64_t* __restrict__ counter, uint64_t rank_cap, uint64_t i0) {
  uint32_t bits = 0;
#pragma unroll
  for (uint32_t k = 0; k < kTrsPer; ++k) {
    if (i0 + k >= n) continue;
    const int64_t r = rank[i0 + k];
    if (r >= 0 && (uint64_t)r < rank_cap && counter[r] > 0) bits |= 1u << k;
  }
  return bits;
}

__global__ __launch_bounds__(kTrsBS) void k_trs_live_count(const int64_t* __restrict__ rank, uint64_t n,
                                                           const int64_t* __restrict__ counter, uint64_t rank_cap,
                                                           uint32_t* __restrict__ blk) {
  __shared__ uint32_t total;
  const uint64_t i0 = (uint64_t)blockIdx.x * TRISTREAM_TILE + (uint64_t)threadIdx.x * kTrsPer;
  block_count_to<kTrsBS>((uint32_t)__popc(live_bits(rank, n, counter, rank_cap, i0)), &total, blk + blockIdx.x);
}

__global__ __launch_bounds__(kTrsBS) void k_trs_live_write(const int64_t* __restrict__ v, const int64_t* __restrict__ rank,
                                                           uint64_t n, const int64_t* __restrict__ counter,
                                                           uint64_t rank_cap, const uint32_t* __restrict__ blk,
                                                           int64_t* __restrict__ ov, int64_t* __restrict__ oc,
                                                           uint64_t cap) {
  __shared__ uint32_t wsum[kTrsBS / 64];
  const uint64_t i0 = (uint64_t)blockIdx.x * TRISTREAM_TILE + (uint64_t)threadIdx.x * kTrsPer;
  const uint32_t bits = live_bits(rank, n, counter, rank_cap, i0);
  uint64_t pos = (uint64_t)blk[blockIdx.x] + block_excl_scan<kTrsBS>((uint32_t)__popc(bits), wsum);
#pragma unroll
  for (uint32_t k = 0; k < kTrsPer; ++k) {
    if (!(bits & (1u << k))) continue;
    if (pos < cap) {
      if (ov) ov[pos] = v[i0 + k];
      if (oc) oc[pos] = counter[rank[i0 + k]];
    }
    ++pos;
  }
}

inline uint32_t blocks_of(uint64_t n) { return (uint32_t)((n + kTrsBS - 1) / kTrsBS); }
inline uint32_t tiles_of(uint64_t n) { return (uint32_t)trs_tiles(n, TRISTREAM_TILE); }
inline uint32_t walk_blocks(uint64_t n) {
  return (uint32_t)((n + (uint64_t)kTrsWaveArrivals * (kTrsBS / 64) - 1) / ((uint64_t)kTrsWaveArrivals * (kTrsBS / 64)));
}

}  // namespace

void launch_trs_compact_new(const uint32_t* pay, const int64_t* lo, const int64_t* hi, uint64_t n, const uint8_t* flags,
                            const uint32_t* blk, uint64_t t0, int64_t* nx, int64_t* ny, uint32_t* nfirst,
                            uint8_t* is_new, uint64_t cap, hipStream_t st) {
  if (!n) return;
  hipLaunchKernelGGL(k_trs_compact_new, dim3((uint32_t)tri_blocks(n)), dim3(kTriBS), 0, st, pay, lo, hi, n, flags, blk,
                     t0, nx, ny, nfirst, is_new, cap);
}

void launch_trs_reverse(const uint32_t* pay, const int64_t* nx, const int64_t* ny, const uint32_t* nfirst, uint64_t m,
                        int64_t* rx, int64_t* ry, uint32_t* rfirst, hipStream_t st) {
  if (!m) return;
  hipLaunchKernelGGL(k_trs_reverse, dim3(blocks_of(m)), dim3(kTrsBS), 0, st, pay, nx, ny, nfirst, m, rx, ry, rfirst);
}

void launch_trs_merge(const TrsAdj& A, const int64_t* nx, const int64_t* ny, const uint32_t* nfirst, const int64_t* rx,
                      const int64_t* ry, const uint32_t* rfirst, uint64_t m, const TrsAdjOut& O, hipStream_t st) {
  const uint64_t total = A.n + 2 * m;
  if (!total) return;
  hipLaunchKernelGGL(k_trs_merge, dim3(blocks_of(total)), dim3(kTrsBS), 0, st, A, nx, ny, nfirst, rx, ry, rfirst, m, O);
}

void launch_trs_head_count(const int64_t* x, uint64_t n, uint32_t* blk, hipStream_t st) {
  if (!n) return;
  hipLaunchKernelGGL(k_trs_head_count, dim3(tiles_of(n)), dim3(kTrsBS), 0, st, x, n, blk);
}

void launch_trs_head_write(const int64_t* x, uint64_t n, const uint32_t* blk, int64_t* out, uint64_t cap, hipStream_t st) {
  if (!n) return;
  hipLaunchKernelGGL(k_trs_head_write, dim3(tiles_of(n)), dim3(kTrsBS), 0, st, x, n, blk, out, cap);
}

void launch_trs_rows(const TrsAdj& A, const int64_t* lo, const int64_t* hi, const uint8_t* is_new, uint64_t n,
                     TrsRowInfo* info, unsigned long long* ctl, hipStream_t st) {
  if (!n) return;
  hipLaunchKernelGGL(k_trs_rows, dim3(blocks_of(n)), dim3(kTrsBS), 0, st, A, lo, hi, is_new, n, info, ctl);
}

void launch_trs_count(const TrsAdj& A, const TrsRowInfo* info, uint64_t n, uint64_t t0, uint32_t* cnt,
                      unsigned long long* ctl, hipStream_t st) {
  if (!n) return;
  hipLaunchKernelGGL((k_trs_walk<false, TRISTREAM_LANES>), dim3(walk_blocks(n)), dim3(kTrsBS), 0, st, A, info,
                     (const int64_t*)nullptr, (const int64_t*)nullptr, n, t0, cnt, (const uint32_t*)nullptr,
                     (uint32_t*)nullptr, (int64_t*)nullptr, (uint32_t*)nullptr, (uint64_t)0, ctl);
  hipLaunchKernelGGL((k_trs_walk<false, 64>), dim3(walk_blocks(n)), dim3(kTrsBS), 0, st, A, info,
                     (const int64_t*)nullptr, (const int64_t*)nullptr, n, t0, cnt, (const uint32_t*)nullptr,
                     (uint32_t*)nullptr, (int64_t*)nullptr, (uint32_t*)nullptr, (uint64_t)0, ctl);
}

void launch_trs_arr_reduce(const uint32_t* cnt, uint64_t n, TrsSeg* agg, TrsSeg* carry, unsigned long long* ctl,
                           hipStream_t st) {
  if (!n) return;
  hipLaunchKernelGGL(k_trs_arr_reduce, dim3(tiles_of(n)), dim3(kTrsBS), 0, st, cnt, n, agg);
  hipLaunchKernelGGL(k_trs_carry, dim3(1), dim3(kTrsBS), 0, st, (const TrsSeg*)agg, carry, (uint64_t)tiles_of(n),
                     ctl + TRS_CLOSED);
}

void launch_trs_arr_apply(const uint32_t* cnt, uint64_t n, const TrsSeg* carry, int64_t total0, uint32_t* closed,
                          int64_t* total, uint32_t* roff, hipStream_t st) {
  if (!n) return;
  hipLaunchKernelGGL(k_trs_arr_apply, dim3(tiles_of(n)), dim3(kTrsBS), 0, st, cnt, n, carry, total0, closed, total, roff);
}

void launch_trs_write(const TrsAdj& A, const TrsRowInfo* info, const int64_t* lo, const int64_t* hi, const uint32_t* cnt,
                      const uint32_t* roff, uint64_t n, uint64_t t0, uint32_t* r_arr, int64_t* r_v, uint32_t* r_delta,
                      uint64_t cap, unsigned long long* ctl, hipStream_t st) {
  if (!n) return;
  hipLaunchKernelGGL((k_trs_walk<true, TRISTREAM_LANES>), dim3(walk_blocks(n)), dim3(kTrsBS), 0, st, A, info, lo, hi, n,
                     t0, const_cast<uint32_t*>(cnt), roff, r_arr, r_v, r_delta, cap, ctl);
  hipLaunchKernelGGL((k_trs_walk<true, 64>), dim3(walk_blocks(n)), dim3(kTrsBS), 0, st, A, info, lo, hi, n, t0,
                     const_cast<uint32_t*>(cnt), roff, r_arr, r_v, r_delta, cap, ctl);
}

void launch_trs_seg_pass(const unsigned long long* skey, const uint32_t* spay, const uint32_t* delta, uint64_t n,
                         int64_t* counter, uint64_t rank_cap, TrsSeg* agg, TrsSeg* carry, int64_t* count,
                         unsigned long long* ctl, hipStream_t st) {
  if (!n) return;
  const uint32_t tiles = tiles_of(n);
  hipLaunchKernelGGL(k_trs_seg_reduce, dim3(tiles), dim3(kTrsBS), 0, st, skey, spay, delta, n, agg, ctl);
  hipLaunchKernelGGL(k_trs_carry, dim3(1), dim3(kTrsBS), 0, st, (const TrsSeg*)agg, carry, (uint64_t)tiles,
                     (unsigned long long*)nullptr);
  hipLaunchKernelGGL(k_trs_seg_apply, dim3(tiles), dim3(kTrsBS), 0, st, skey, spay, delta, n, (const TrsSeg*)carry,
                     (const int64_t*)counter, rank_cap, count, ctl);
  hipLaunchKernelGGL(k_trs_commit, dim3(blocks_of(n)), dim3(kTrsBS), 0, st, skey, spay, n, (const int64_t*)count, counter,
                     rank_cap);
}

void launch_trs_live_count(const int64_t* rank, uint64_t n, const int64_t* counter, uint64_t rank_cap, uint32_t* blk,
                           hipStream_t st) {
  if (!n) return;
  hipLaunchKernelGGL(k_trs_live_count, dim3(tiles_of(n)), dim3(kTrsBS), 0, st, rank, n, counter, rank_cap, blk);
}

void launch_trs_live_write(const int64_t* v, const int64_t* rank, uint64_t n, const int64_t* counter, uint64_t rank_cap,
                           const uint32_t* blk, int64_t* ov, int64_t* oc, uint64_t cap, hipStream_t st) {
  if (!n) return;
  hipLaunchKernelGGL(k_trs_live_write, dim3(tiles_of(n)), dim3(kTrsBS), 0, st, v, rank, n, counter, rank_cap, blk, ov, oc,
                     cap);
}

}  // namespace gs
