// gs_degstream_k.hip -- kernels of the degree streams (gfx950).
//
//   k_ds_keys        : one occurrence per thread: its rank through the stored slot index, its
//                      sign from the deletion byte, its id
//   k_ds_seg_reduce  : the seeded segmented scan, step 1. A tile of DEGSTREAM_TILE sorted
//                      positions, kDsPer consecutive ones per thread, reduced to one DsSeg
//   k_ds_seg_carry   : step 2, one workgroup: the exclusive scan of the tile aggregates
//   k_ds_seg_apply   : step 3. Every position: carry-in, then the in-tile prefix, applied to
//                      the seed; (before, after) at its arrival position; the state at tails
//   k_ds_seg_commit  : step 4. The one deferred tail per tile
//   k_ds_rec_count / k_ds_rec_write   : the records of every occurrence, compacted in arrival order
//   k_ds_live_count / k_ds_live_write : the live entries of a state array, compacted in index order
// The maps, their composition, the segmented combine and the record rule are
// gs_degstream_seq.hpp's; the tile count, the rank inside a tile and the block-wide segmented
// scan are gs_scan.hpp's.
//
// Concurrency. No atomics carry data: the only atomics are the error flag, the maximum and the
// crossed-tile counter, read by the host after the fold. k_ds_seg_apply reads state[key] (the
// seed) at every position and writes state[key] at tails. Inside a workgroup every seed is
// loaded before the block scan's barrier and every tail is stored after it. A segment that
// reaches into another tile has its seed read by another workgroup, so its tail is not stored
// here: a tile has at most one such tail (the segment its first position continues), which goes
// to (late_idx, late_val)[tile] and is stored by the next launch. Nobody waits.
//
// What bounds every loop and index:
//   * per-element kernels handle one element per thread, its index tested against the count;
//   * tile kernels handle kDsPer positions per thread, each tested against the count; the
//     neighbours j - 1 and j + 1 of a position are read only inside [0, n);
//   * a stored slot index is tested against the table's slot count, a rank or degree against
//     the state array's capacity (DS_ERR is raised and the position reads seed 0 and stores
//     nothing), a sort payload against the position count, before any is used as an index;
//   * every output row is tested against the capacity of its array before the store;
//   * k_ds_seg_carry's loop runs ceil(tiles / kDsBS) times.
#include "gs_degstream.hpp"
#include "gs_scan.hpp"
#include "gs_sort.hpp"

namespace gs {
namespace {

__device__ __forceinline__ void raise_err(unsigned long long* ctl) { atomicOr(ctl + DS_ERR, 1ull); }

__global__ __launch_bounds__(kDsBS) void k_ds_keys(const int64_t* __restrict__ src, const int64_t* __restrict__ dst,
                                                  const uint8_t* __restrict__ del, uint64_t occs, uint64_t stride,
                                                  int dir, DistVTable vt, const uint32_t* __restrict__ vslot,
                                                  uint64_t rank_cap, int64_t* __restrict__ key,
                                                  int8_t* __restrict__ sgn, int64_t* __restrict__ vertex,
                                                  unsigned long long* __restrict__ ctl) {
  const uint64_t o = (uint64_t)blockIdx.x * kDsBS + threadIdx.x;
  if (o >= occs) return;
  const uint64_t e = ds_occ_edge(o, dir);
  const uint64_t entry = dir == kDsAll ? o : 2 * o;  // (IN / OUT: both entries of an edge are the collected endpoint)
  const uint32_t s = vslot[entry];
  uint32_t rank = 0;
  if (s <= vt.cap) {
    rank = vt.tab[s].rank;
    if (rank >= rank_cap) {
      raise_err(ctl);
      rank = 0;
    }
  } else {
    raise_err(ctl);
  }
  key[o] = (int64_t)rank;
  sgn[o] = (int8_t)ds_sign(del, e);
  vertex[o] = ds_occ_is_dst(o, dir) ? dst[e * stride] : src[e * stride];
}

// what a thread holds of its kDsPer positions
struct DsMine {
  uint32_t idx[kDsPer];   // the key's low 32 bits
  uint32_t pay[kDsPer];
  int c[kDsPer];
  uint32_t head, tail, live;  // bit k: position k is a segment head / a tail / below n
};

__device__ __forceinline__ void load_mine(const unsigned long long* __restrict__ skey, const uint32_t* __restrict__ spay,
                                          const int8_t* __restrict__ sgn, uint64_t n, uint64_t j0, DsMine& m) {
  m.head = m.tail = m.live = 0;
  unsigned long long prev = 0;
  if (j0 > 0 && j0 - 1 < n) prev = skey[j0 - 1];
#pragma unroll
  for (uint32_t k = 0; k < kDsPer; ++k) {
    const uint64_t j = j0 + k;
    m.idx[k] = 0;
    m.pay[k] = 0;
    m.c[k] = 0;
    if (j < n) {
      const unsigned long long x = skey[j];
      const uint32_t p = spay[j];
      m.live |= 1u << k;
      m.idx[k] = (uint32_t)x;
      m.pay[k] = p;
      m.c[k] = p < n ? (int)sgn[p] : 0;
      if (j == 0 || x != prev) m.head |= 1u << k;
      prev = x;
    }
  }
#pragma unroll
  for (uint32_t k = 0; k < kDsPer; ++k) {
    const uint64_t j = j0 + k;
    if (j < n) {
      bool t = j + 1 == n;
      if (!t) t = k + 1 < kDsPer ? ((m.head >> (k + 1)) & 1u) != 0 : skey[j + 1] != skey[j];
      if (t) m.tail |= 1u << k;
    }
  }
}

__device__ __forceinline__ DsSeg reduce_mine(const DsMine& m, bool clamp) {
  DsSeg s = ds_seg_identity();
#pragma unroll
  for (uint32_t k = 0; k < kDsPer; ++k)
    if ((m.live >> k) & 1u) s = ds_seg_combine(s, ds_seg_element(m.c[k], clamp, ((m.head >> k) & 1u) != 0));
  return s;
}

__global__ __launch_bounds__(kDsBS) void k_ds_seg_reduce(const unsigned long long* __restrict__ skey,
                                                        const uint32_t* __restrict__ spay,
                                                        const int8_t* __restrict__ sgn, uint64_t n, int clamp,
                                                        DsSeg* __restrict__ agg, unsigned long long* __restrict__ ctl) {
  __shared__ DsSeg wagg[kDsBS / 64];
  const uint64_t j0 = (uint64_t)blockIdx.x * DEGSTREAM_TILE + (uint64_t)threadIdx.x * kDsPer;
  DsMine m;
  load_mine(skey, spay, sgn, n, j0, m);
  DsSeg total;
  (void)block_seg_excl<kDsBS, DsSegOps>(reduce_mine(m, clamp != 0), wagg, &total);
  if (threadIdx.x == 0) {
    agg[blockIdx.x] = total;
    if (blockIdx.x > 0 && !(m.head & 1u)) atomicAdd(ctl + DS_CROSSED, 1ull);
  }
}

__global__ __launch_bounds__(kDsBS) void k_ds_seg_carry(const DsSeg* __restrict__ agg, DsSeg* __restrict__ carry,
                                                       uint64_t tiles) {
  __shared__ DsSeg wagg[kDsBS / 64];
  DsSeg run = ds_seg_identity();
  for (uint64_t t0 = 0; t0 < tiles; t0 += kDsBS) {
    const uint64_t t = t0 + threadIdx.x;
    const DsSeg mine = t < tiles ? agg[t] : ds_seg_identity();
    DsSeg total;
    const DsSeg excl = block_seg_excl<kDsBS, DsSegOps>(mine, wagg, &total);
    if (t < tiles) carry[t] = ds_seg_combine(run, excl);
    run = ds_seg_combine(run, total);
    __syncthreads();  // wagg is written again
  }
}

__global__ __launch_bounds__(kDsBS) void k_ds_seg_apply(const unsigned long long* __restrict__ skey,
                                                       const uint32_t* __restrict__ spay,
                                                       const int8_t* __restrict__ sgn, uint64_t n, int clamp,
                                                       const DsSeg* __restrict__ carry, uint32_t* state,
                                                       uint64_t state_cap, uint32_t* __restrict__ late_idx,
                                                       uint32_t* __restrict__ late_val, uint32_t* __restrict__ before,
                                                       uint32_t* __restrict__ after, unsigned long long* __restrict__ ctl,
                                                       unsigned long long* __restrict__ max_word) {
  __shared__ DsSeg wagg[kDsBS / 64];
  const uint64_t j0 = (uint64_t)blockIdx.x * DEGSTREAM_TILE + (uint64_t)threadIdx.x * kDsPer;
  DsMine m;
  load_mine(skey, spay, sgn, n, j0, m);
  int64_t seed[kDsPer];
  bool bad = false;
#pragma unroll
  for (uint32_t k = 0; k < kDsPer; ++k) {
    seed[k] = 0;
    if ((m.live >> k) & 1u) {
      if (m.idx[k] < state_cap && m.pay[k] < n)
        seed[k] = (int64_t)state[m.idx[k]];
      else
        bad = true;
    }
  }
  if (bad) raise_err(ctl);
  if (threadIdx.x == 0) late_idx[blockIdx.x] = kDsNoLate;
  DsSeg total;
  DsSeg in = block_seg_excl<kDsBS, DsSegOps>(reduce_mine(m, clamp != 0), wagg, &total);  // (barrier: seeds loaded, late_idx set)
  const DsSeg cin = carry[blockIdx.x];
  uint32_t top = 0;
#pragma unroll
  for (uint32_t k = 0; k < kDsPer; ++k) {
    if (!((m.live >> k) & 1u)) continue;
    const bool head = ((m.head >> k) & 1u) != 0;
    const DsSeg el = ds_seg_element(m.c[k], clamp != 0, head);
    const int64_t x = ds_seg_before(ds_seg_combine(cin, in), head, seed[k]);
    const int64_t y = ds_apply(DsPair{el.a, el.b}, x);
    in = ds_seg_combine(in, el);
    const bool ok = m.idx[k] < state_cap && m.pay[k] < n;
    if (ok) {
      if (before) before[m.pay[k]] = (uint32_t)x;
      after[m.pay[k]] = (uint32_t)y;
      top = (uint32_t)y > top ? (uint32_t)y : top;
      if ((m.tail >> k) & 1u) {
        if (in.head) {  // the whole segment lies in this tile
          state[m.idx[k]] = (uint32_t)y;
        } else {
          late_idx[blockIdx.x] = m.idx[k];
          late_val[blockIdx.x] = (uint32_t)y;
        }
      }
    }
  }
  if (max_word) {  // (every lane reaches this)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const uint32_t y = __shfl_xor(top, o, 64);
      top = y > top ? y : top;
    }
    if ((threadIdx.x & 63u) == 0 && top) atomicMax(max_word, (unsigned long long)top);
  }
}

__global__ __launch_bounds__(kDsBS) void k_ds_seg_commit(const uint32_t* __restrict__ late_idx,
                                                        const uint32_t* __restrict__ late_val, uint64_t tiles,
                                                        uint32_t* __restrict__ state, uint64_t state_cap) {
  const uint64_t t = (uint64_t)blockIdx.x * kDsBS + threadIdx.x;
  if (t >= tiles) return;
  const uint32_t i = late_idx[t];
  if (i != kDsNoLate && i < state_cap) state[i] = late_val[t];
}

// ---- records
__device__ __forceinline__ uint32_t rec_counts(const uint32_t* __restrict__ old_d, const uint32_t* __restrict__ new_d,
                                               const int8_t* __restrict__ sgn, uint64_t occs, uint64_t o0,
                                               uint32_t cnt[kDsPer]) {
  uint32_t sum = 0;
#pragma unroll
  for (uint32_t k = 0; k < kDsPer; ++k) {
    const uint64_t o = o0 + k;
    cnt[k] = o < occs ? ds_record_count(old_d[o], new_d[o], (int)sgn[o]) : 0u;
    sum += cnt[k];
  }
  return sum;
}

__global__ __launch_bounds__(kDsBS) void k_ds_rec_count(const uint32_t* __restrict__ old_d,
                                                       const uint32_t* __restrict__ new_d,
                                                       const int8_t* __restrict__ sgn, uint64_t occs,
                                                       uint32_t* __restrict__ blk) {
  __shared__ uint32_t total;
  uint32_t cnt[kDsPer];
  const uint64_t o0 = (uint64_t)blockIdx.x * DEGSTREAM_TILE + (uint64_t)threadIdx.x * kDsPer;
  block_count_to<kDsBS>(rec_counts(old_d, new_d, sgn, occs, o0, cnt), &total, blk + blockIdx.x);
}

__global__ __launch_bounds__(kDsBS) void k_ds_rec_write(const uint32_t* __restrict__ old_d,
                                                       const uint32_t* __restrict__ new_d,
                                                       const int8_t* __restrict__ sgn, uint64_t occs,
                                                       const uint32_t* __restrict__ blk, uint32_t* __restrict__ occ,
                                                       int64_t* __restrict__ key, uint32_t* __restrict__ degree,
                                                       int8_t* __restrict__ delta, uint64_t cap,
                                                       unsigned long long* __restrict__ ctl) {
  __shared__ uint32_t wsum[kDsBS / 64];
  uint32_t cnt[kDsPer];
  const uint64_t o0 = (uint64_t)blockIdx.x * DEGSTREAM_TILE + (uint64_t)threadIdx.x * kDsPer;
  const uint32_t mine = rec_counts(old_d, new_d, sgn, occs, o0, cnt);
  uint64_t row = (uint64_t)blk[blockIdx.x] + block_excl_scan<kDsBS>(mine, wsum);
  bool bad = false;
#pragma unroll
  for (uint32_t k = 0; k < kDsPer; ++k) {
    const uint64_t o = o0 + k;
    for (uint32_t r = 0; r < cnt[k]; ++r, ++row) {
      if (row >= cap) {
        bad = true;
        continue;
      }
      uint32_t d;
      int dl;
      ds_record(old_d[o], new_d[o], r, &d, &dl);
      occ[row] = (uint32_t)o;
      key[row] = (int64_t)d;
      degree[row] = d;
      delta[row] = (int8_t)dl;
    }
  }
  if (bad) raise_err(ctl);
}

// ---- the live entries of a state array
__global__ __launch_bounds__(kDsBS) void k_ds_live_count(const uint32_t* __restrict__ state, uint64_t n,
                                                        uint32_t* __restrict__ blk) {
  __shared__ uint32_t total;
  const uint64_t i0 = (uint64_t)blockIdx.x * DEGSTREAM_TILE + (uint64_t)threadIdx.x * kDsPer;
  uint32_t cnt = 0;
#pragma unroll
  for (uint32_t k = 0; k < kDsPer; ++k)
    if (i0 + k < n && state[i0 + k] > 0) ++cnt;
  block_count_to<kDsBS>(cnt, &total, blk + blockIdx.x);
}

__global__ __launch_bounds__(kDsBS) void k_ds_live_write(const uint32_t* __restrict__ state, uint64_t n,
                                                        const uint32_t* __restrict__ blk,
                                                        const int64_t* __restrict__ ids, int64_t* __restrict__ id_out,
                                                        int64_t* __restrict__ value_out, uint64_t cap) {
  __shared__ uint32_t wsum[kDsBS / 64];
  const uint64_t i0 = (uint64_t)blockIdx.x * DEGSTREAM_TILE + (uint64_t)threadIdx.x * kDsPer;
  uint32_t val[kDsPer], cnt = 0;
#pragma unroll
  for (uint32_t k = 0; k < kDsPer; ++k) {
    val[k] = i0 + k < n ? state[i0 + k] : 0u;
    cnt += val[k] > 0 ? 1u : 0u;
  }
  uint64_t row = (uint64_t)blk[blockIdx.x] + block_excl_scan<kDsBS>(cnt, wsum);
#pragma unroll
  for (uint32_t k = 0; k < kDsPer; ++k) {
    if (val[k] == 0) continue;
    if (row < cap) {
      if (id_out) id_out[row] = ids ? ids[i0 + k] : (int64_t)(i0 + k);
      if (value_out) value_out[row] = (int64_t)val[k];
    }
    ++row;
  }
}

inline uint32_t blocks_of(uint64_t n) { return (uint32_t)((n + kDsBS - 1) / kDsBS); }

}  // namespace

void launch_ds_keys(const int64_t* src, const int64_t* dst, const uint8_t* del, uint64_t n, uint64_t stride, int dir,
                    const DistVTable& vt, const uint32_t* vslot, uint64_t rank_cap, int64_t* key, int8_t* sgn,
                    int64_t* vertex, unsigned long long* ctl, hipStream_t st) {
  const uint64_t occs = ds_occurrences(n, dir);
  if (occs == 0) return;
  hipLaunchKernelGGL(k_ds_keys, dim3(blocks_of(occs)), dim3(kDsBS), 0, st, src, dst, del, occs, stride, dir, vt, vslot,
                     rank_cap, key, sgn, vertex, ctl);
}

void launch_ds_seg_pass(const unsigned long long* skey, const uint32_t* spay, const int8_t* sgn, uint64_t n, bool clamp,
                        uint32_t* state, uint64_t state_cap, DsSeg* agg, DsSeg* carry, uint32_t* late_idx,
                        uint32_t* late_val, uint32_t* before, uint32_t* after, unsigned long long* ctl,
                        unsigned long long* max_word, hipStream_t st) {
  if (n == 0) return;
  const uint64_t tiles = ds_tiles(n, DEGSTREAM_TILE);
  const int cl = clamp ? 1 : 0;
  hipLaunchKernelGGL(k_ds_seg_reduce, dim3((uint32_t)tiles), dim3(kDsBS), 0, st, skey, spay, sgn, n, cl, agg, ctl);
  hipLaunchKernelGGL(k_ds_seg_carry, dim3(1), dim3(kDsBS), 0, st, (const DsSeg*)agg, carry, tiles);
  hipLaunchKernelGGL(k_ds_seg_apply, dim3((uint32_t)tiles), dim3(kDsBS), 0, st, skey, spay, sgn, n, cl,
                     (const DsSeg*)carry, state, state_cap, late_idx, late_val, before, after, ctl, max_word);
  hipLaunchKernelGGL(k_ds_seg_commit, dim3(blocks_of(tiles)), dim3(kDsBS), 0, st, (const uint32_t*)late_idx,
                     (const uint32_t*)late_val, tiles, state, state_cap);
}

void launch_ds_rec_count(const uint32_t* old_d, const uint32_t* new_d, const int8_t* sgn, uint64_t occs, uint32_t* blk,
                         hipStream_t st) {
  if (occs == 0) return;
  hipLaunchKernelGGL(k_ds_rec_count, dim3((uint32_t)ds_tiles(occs, DEGSTREAM_TILE)), dim3(kDsBS), 0, st, old_d, new_d,
                     sgn, occs, blk);
}

void launch_ds_rec_write(const uint32_t* old_d, const uint32_t* new_d, const int8_t* sgn, uint64_t occs,
                         const uint32_t* blk, uint32_t* occ, int64_t* key, uint32_t* degree, int8_t* delta,
                         uint64_t cap, unsigned long long* ctl, hipStream_t st) {
  if (occs == 0) return;
  hipLaunchKernelGGL(k_ds_rec_write, dim3((uint32_t)ds_tiles(occs, DEGSTREAM_TILE)), dim3(kDsBS), 0, st, old_d, new_d,
                     sgn, occs, blk, occ, key, degree, delta, cap, ctl);
}

void launch_ds_live_count(const uint32_t* state, uint64_t n, uint32_t* blk, hipStream_t st) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_ds_live_count, dim3((uint32_t)ds_tiles(n, DEGSTREAM_TILE)), dim3(kDsBS), 0, st, state, n, blk);
}

void launch_ds_live_write(const uint32_t* state, uint64_t n, const uint32_t* blk, const int64_t* ids, int64_t* id_out,
                          int64_t* value_out, uint64_t cap, hipStream_t st) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_ds_live_write, dim3((uint32_t)ds_tiles(n, DEGSTREAM_TILE)), dim3(kDsBS), 0, st, state, n, blk,
                     ids, id_out, value_out, cap);
}

}  // namespace gs
