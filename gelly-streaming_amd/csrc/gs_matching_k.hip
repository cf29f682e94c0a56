// gs_matching_k.hip -- kernels of the weighted matching summary (gfx950).
//
//   k_mt_init     : state records to their initial value
//   k_mt_gather   : the ranks of every arrival's endpoints (through the slot indices the distinct
//                   streams' vertex phase left), its value, the first pending list
//   k_mt_reset / k_mt_seed / k_mt_pass / k_mt_lower / k_mt_remain / k_mt_commit :
//                   the phases of a round, one pending arrival per thread; each is one call of the
//                   phase function of the same name in gs_matching_seq.hpp
//   k_mt_tail     : one workgroup runs whole rounds with the same phase functions, a fence and a
//                   barrier where the grid has a kernel boundary
//   k_mt_event_count / k_mt_event_write : flag-scan-compact (gs_scan.hpp) over rows per arrival
//   k_mt_export / k_mt_decode / k_mt_mate : M by acceptance order, and the mate probe
//
// Concurrency. Inside a phase the only words that two threads both touch are T and Rd: they are
// lowered by atomic minimum and read by a load that bypasses the wave's cache (mt_lower,
// mt_peek); a pass that reads a value another thread lowers later is followed by another pass
// (the lowering thread reports a change). State records are written by the commit phase alone,
// and two arrivals that commit in one round have disjoint cells. Between phases: a kernel
// boundary, or in the tail __threadfence() + __syncthreads() of the one workgroup. Nobody waits
// for another workgroup.
//
// What bounds every loop and index:
//   * a thread handles one list position q < np (the tail: q strided below its count); the
//     arrival e = list[q] is tested against n before use (a bad one raises MT_ERR and is dropped);
//   * ranks are tested against the state's capacity once, by k_mt_gather, which stores 0 for a
//     bad one and raises MT_ERR; partners are only ever copies of those ranks;
//   * the fixpoint runs at most iter_cap passes, and every round retires its earliest pending
//     arrival, so the tail's loop ends after at most np rounds;
//   * every output row is tested against the capacity of its array before the store.
#include "gs_matching.hpp"
#include "gs_scan.hpp"
#include "gs_sort.hpp"

namespace gs {
namespace {

__device__ __forceinline__ int sharpen_now(int sharpen, const unsigned long long* ctl) {
  return (sharpen && __hip_atomic_load(ctl + MT_UNSAFE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) ? 1 : 0;
}

__global__ __launch_bounds__(kMtBS) void k_mt_init(MtVertex* st, uint64_t from, uint64_t to) {
  const uint64_t i = from + (uint64_t)blockIdx.x * kMtBS + threadIdx.x;
  if (i < to) st[i] = mt_vertex_init();
}

__global__ __launch_bounds__(kMtBS) void k_mt_gather(const uint32_t* __restrict__ vslot, const DistVSlot* tab,
                                                     uint64_t slots, uint64_t st_cap, const int64_t* __restrict__ val,
                                                     uint64_t stride, uint64_t n, uint32_t* __restrict__ ru,
                                                     uint32_t* __restrict__ rv, int64_t* __restrict__ w,
                                                     uint32_t* __restrict__ list, uint8_t* __restrict__ accepted,
                                                     unsigned long long* ctl) {
  const uint64_t i = (uint64_t)blockIdx.x * kMtBS + threadIdx.x;
  if (i >= n) return;
  uint32_t r[2];
  bool bad = false;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const uint32_t s = vslot[2 * i + k];
    r[k] = s < slots ? tab[s].rank : kDistNoRank;
    if (r[k] >= st_cap) {
      r[k] = 0;
      bad = true;
    }
  }
  const int64_t x = val[i * stride];
  ru[i] = r[0];
  rv[i] = r[1];
  w[i] = x;
  list[i] = (uint32_t)i;
  accepted[i] = 0;
  if (bad) atomicOr(ctl + MT_ERR, 1ull);
  if (!mt_weight_safe(x)) atomicOr(ctl + MT_UNSAFE, 1ull);
}

// the arrival of list position q, or kMtFar
__device__ __forceinline__ uint32_t pending_at(const uint32_t* list, uint64_t q, uint64_t np, uint32_t n,
                                               unsigned long long* ctl) {
  if (q >= np) return kMtFar;
  const uint32_t e = list[q];
  if (e >= n) {
    atomicOr(ctl + MT_ERR, 1ull);
    return kMtFar;
  }
  return e;
}

__global__ __launch_bounds__(kMtBS) void k_mt_reset(MtFold F, const uint32_t* list, uint64_t np, uint32_t n,
                                                    unsigned long long* ctl) {
  const uint64_t q = (uint64_t)blockIdx.x * kMtBS + threadIdx.x;
  if (q == 0) ctl[MT_NEXT] = 0;
  if (blockIdx.x == 0 && threadIdx.x <= kMatchingMaxIterCap) ctl[MT_CHG + threadIdx.x] = threadIdx.x == 0 ? 1 : 0;
  const uint32_t e = pending_at(list, q, np, n, ctl);
  if (e != kMtFar) mt_ph_reset(F, e);
}

__global__ __launch_bounds__(kMtBS) void k_mt_seed(MtFold F, const uint32_t* list, uint64_t np, uint32_t n,
                                                   unsigned long long* ctl) {
  const uint32_t e = pending_at(list, (uint64_t)blockIdx.x * kMtBS + threadIdx.x, np, n, ctl);
  if (e != kMtFar) mt_ph_seed(F, e);
}

// pass k >= 1 of the fixpoint: runs only if pass k - 1 (the seed: k = 1) marked an arrival
__global__ __launch_bounds__(kMtBS) void k_mt_pass(MtFold F, const uint32_t* list, uint64_t np, uint32_t n,
                                                   int sharpen, uint32_t k, unsigned long long* ctl) {
  if (ctl[MT_CHG + k - 1] == 0) return;  // (written by an earlier launch; uniform)
  F.sharpen = sharpen_now(sharpen, ctl);
  const uint64_t q = (uint64_t)blockIdx.x * kMtBS + threadIdx.x;
  if (q == 0) atomicAdd(ctl + MT_ITERS, 1ull);
  const uint32_t e = pending_at(list, q, np, n, ctl);
  const bool now = e != kMtFar && mt_ph_pass(F, e);
  if (__ballot(now) && (threadIdx.x & 63u) == 0) ctl[MT_CHG + k] = 1;
}

// the cap was hit before the fixpoint: plain reservations
__global__ __launch_bounds__(kMtBS) void k_mt_lower(MtFold F, const uint32_t* list, uint64_t np, uint32_t n,
                                                    uint32_t cap, unsigned long long* ctl) {
  if (ctl[MT_CHG + cap] == 0) return;
  const uint64_t q = (uint64_t)blockIdx.x * kMtBS + threadIdx.x;
  if (q == 0) atomicAdd(ctl + MT_FALLBACKS, 1ull);
  const uint32_t e = pending_at(list, q, np, n, ctl);
  if (e != kMtFar) mt_ph_lower(F, e);
}

__global__ __launch_bounds__(kMtBS) void k_mt_remain(MtFold F, const uint32_t* list, uint64_t np, uint32_t n,
                                                     int sharpen, unsigned long long* ctl) {
  F.sharpen = sharpen_now(sharpen, ctl);
  const uint32_t e = pending_at(list, (uint64_t)blockIdx.x * kMtBS + threadIdx.x, np, n, ctl);
  if (e != kMtFar) mt_ph_remain(F, e);
}

// the still pending arrivals to list_out: one atomic per wave
__global__ __launch_bounds__(kMtBS) void k_mt_commit(MtFold F, const uint32_t* list, uint64_t np, uint32_t n,
                                                     uint32_t* __restrict__ list_out, unsigned long long* ctl) {
  const uint32_t e = pending_at(list, (uint64_t)blockIdx.x * kMtBS + threadIdx.x, np, n, ctl);
  const bool stay = e != kMtFar && mt_ph_commit(F, e);
  const unsigned long long m = __ballot(stay);
  if (!m) return;  // wave-uniform
  const int lane = (int)(threadIdx.x & 63u);
  const int leader = __ffsll((long long)m) - 1;
  unsigned long long base = 0;
  if (lane == leader) base = atomicAdd(ctl + MT_NEXT, (unsigned long long)__popcll(m));
  base = __shfl(base, leader, 64);
  if (!stay) return;
  const uint64_t row = base + (uint64_t)__popcll(m & ((1ull << lane) - 1ull));
  if (row < np) list_out[row] = e;
}

// what one workgroup does where the grid has a kernel boundary: its stores are out and its
// later loads are fresh
__device__ __forceinline__ void tail_sync() {
  __threadfence();
  __syncthreads();
}

__global__ __launch_bounds__(kMtTailBS) void k_mt_tail(MtFold F, uint32_t* la, uint32_t* lb, uint32_t np, uint32_t n,
                                                       uint32_t iter_cap, int sharpen, unsigned long long* ctl) {
  __shared__ uint32_t s_next, s_chg;
  F.sharpen = sharpen_now(sharpen, ctl);
  uint32_t cnt = np, rounds = 0, iters = 0, fallbacks = 0;  // uniform over the workgroup
  while (cnt) {
    for (uint32_t q = threadIdx.x; q < cnt; q += kMtTailBS) {
      const uint32_t e = pending_at(la, q, cnt, n, ctl);
      if (e != kMtFar) mt_ph_reset(F, e);
    }
    if (threadIdx.x == 0) s_next = 0;
    tail_sync();
    for (uint32_t q = threadIdx.x; q < cnt; q += kMtTailBS) {
      const uint32_t e = pending_at(la, q, cnt, n, ctl);
      if (e != kMtFar) mt_ph_seed(F, e);
    }
    tail_sync();
    bool changed = true;
    for (uint32_t it = 0; it < iter_cap && changed; ++it) {
      if (threadIdx.x == 0) s_chg = 0;
      __syncthreads();
      bool now = false;
      for (uint32_t q = threadIdx.x; q < cnt; q += kMtTailBS) {
        const uint32_t e = pending_at(la, q, cnt, n, ctl);
        if (e != kMtFar && mt_ph_pass(F, e)) now = true;
      }
      if (now) s_chg = 1;
      tail_sync();
      changed = s_chg != 0;
      __syncthreads();  // (everyone has read s_chg before the next pass clears it)
      ++iters;
    }
    if (changed) {
      for (uint32_t q = threadIdx.x; q < cnt; q += kMtTailBS) {
        const uint32_t e = pending_at(la, q, cnt, n, ctl);
        if (e != kMtFar) mt_ph_lower(F, e);
      }
      ++fallbacks;
      tail_sync();
    }
    for (uint32_t q = threadIdx.x; q < cnt; q += kMtTailBS) {
      const uint32_t e = pending_at(la, q, cnt, n, ctl);
      if (e != kMtFar) mt_ph_remain(F, e);
    }
    tail_sync();
    for (uint32_t q = threadIdx.x; q < cnt; q += kMtTailBS) {
      const uint32_t e = pending_at(la, q, cnt, n, ctl);
      if (e != kMtFar && mt_ph_commit(F, e)) {
        const uint32_t row = atomicAdd(&s_next, 1u);
        if (row < cnt) lb[row] = e;
      }
    }
    tail_sync();
    const uint32_t left = s_next;
    __syncthreads();  // (everyone has read s_next before the next round clears it)
    // the earliest pending arrival always leaves; a count that does not fall is a broken state
    if (left >= cnt) {
      if (threadIdx.x == 0) atomicOr(ctl + MT_ERR, 2ull);
      break;
    }
    cnt = left;
    uint32_t* t = la;
    la = lb;
    lb = t;
    ++rounds;
  }
  if (threadIdx.x == 0) {
    atomicAdd(ctl + MT_TAIL_ROUNDS, (unsigned long long)rounds);
    atomicAdd(ctl + MT_ITERS, (unsigned long long)iters);
    atomicAdd(ctl + MT_FALLBACKS, (unsigned long long)fallbacks);
  }
}

// ---- events
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  return x;
}

__global__ __launch_bounds__(kMtBS) void k_mt_event_count(const uint8_t* __restrict__ accepted,
                                                          const MtRec* __restrict__ rec,
                                                          const int64_t* __restrict__ w, uint64_t n,
                                                          uint32_t* __restrict__ blk, unsigned long long* ctl) {
  __shared__ uint32_t total;
  const uint64_t i0 = (uint64_t)blockIdx.x * MATCHING_TILE + (uint64_t)threadIdx.x * kMtPer;
  uint32_t rows = 0;
  unsigned long long acc = 0, edges = 0, weight = 0;  // (wrapping)
#pragma unroll
  for (uint32_t k = 0; k < kMtPer; ++k) {
    const uint64_t i = i0 + k;
    if (i < n && accepted[i]) {
      const MtRec r = rec[i];
      const uint32_t c = mt_event_rows(1, r);
      rows += c;
      acc += 1;
      edges += 2ull - c;  // + 1 - removed
      weight += (unsigned long long)w[i];
      if (r.s0 != kMtNone) weight -= (unsigned long long)r.v0;
      if (r.s1 != kMtNone) weight -= (unsigned long long)r.v1;
    }
  }
  acc = wave_sum(acc);
  edges = wave_sum(edges);
  weight = wave_sum(weight);
  if ((threadIdx.x & 63u) == 0 && acc) {
    atomicAdd(ctl + MT_ACC, acc);
    atomicAdd(ctl + MT_EDGES, edges);
    atomicAdd(ctl + MT_WEIGHT, weight);
  }
  block_count_to<kMtBS>(rows, &total, blk + blockIdx.x);
}

__global__ __launch_bounds__(kMtBS) void k_mt_event_write(const uint8_t* __restrict__ accepted,
                                                          const MtRec* __restrict__ rec,
                                                          const uint32_t* __restrict__ ru,
                                                          const uint32_t* __restrict__ rv,
                                                          const int64_t* __restrict__ w, uint64_t n,
                                                          const uint32_t* __restrict__ blk,
                                                          const int64_t* __restrict__ vid, uint64_t nv,
                                                          uint32_t* __restrict__ arrival, uint8_t* __restrict__ type,
                                                          int64_t* __restrict__ src, int64_t* __restrict__ dst,
                                                          int64_t* __restrict__ val, uint64_t cap) {
  __shared__ uint32_t wsum[kMtBS / 64];
  const uint64_t i0 = (uint64_t)blockIdx.x * MATCHING_TILE + (uint64_t)threadIdx.x * kMtPer;
  uint32_t rows = 0;
#pragma unroll
  for (uint32_t k = 0; k < kMtPer; ++k)
    if (i0 + k < n && accepted[i0 + k]) rows += mt_event_rows(1, rec[i0 + k]);
  uint64_t row = (uint64_t)blk[blockIdx.x] + block_excl_scan<kMtBS>(rows, wsum);
  auto put = [&](uint64_t i, uint8_t t, uint32_t rs, uint32_t rd, int64_t x) {
    if (row < cap && rs < nv && rd < nv) {
      arrival[row] = (uint32_t)i;
      type[row] = t;
      src[row] = vid[rs];
      dst[row] = vid[rd];
      val[row] = x;
    }
    ++row;
  };
#pragma unroll
  for (uint32_t k = 0; k < kMtPer; ++k) {
    const uint64_t i = i0 + k;
    if (i < n && accepted[i]) {
      const MtRec r = rec[i];
      if (r.s0 != kMtNone) put(i, kMatchRemove, r.s0, r.d0, r.v0);
      if (r.s1 != kMtNone) put(i, kMatchRemove, r.s1, r.d1, r.v1);
      put(i, kMatchAdd, ru[i], rv[i], w[i]);
    }
  }
}

// ---- export and probes
__global__ __launch_bounds__(kMtBS) void k_mt_export(const MtVertex* __restrict__ st, uint64_t nv,
                                                     int64_t* __restrict__ stamp_out, uint32_t* __restrict__ rank_out,
                                                     uint64_t cap, unsigned long long* ctl) {
  const uint64_t r = (uint64_t)blockIdx.x * kMtBS + threadIdx.x;
  bool has = false;
  uint64_t stamp = 0;
  if (r < nv) {
    const MtVertex v = st[r];
    has = v.partner != kMtNone && v.is_src != 0;
    stamp = v.stamp;
  }
  const unsigned long long m = __ballot(has);
  if (!m) return;  // wave-uniform
  const int lane = (int)(threadIdx.x & 63u);
  const int leader = __ffsll((long long)m) - 1;
  unsigned long long base = 0;
  if (lane == leader) base = atomicAdd(ctl + MT_EXPORT, (unsigned long long)__popcll(m));
  base = __shfl(base, leader, 64);
  if (!has) return;
  const uint64_t row = base + (uint64_t)__popcll(m & ((1ull << lane) - 1ull));
  if (row < cap) {
    stamp_out[row] = (int64_t)stamp;
    rank_out[row] = (uint32_t)r;
  }
}

__global__ __launch_bounds__(kMtBS) void k_mt_decode(const unsigned long long* __restrict__ skey,
                                                     const uint32_t* __restrict__ pay,
                                                     const uint32_t* __restrict__ rank, uint64_t ne,
                                                     const MtVertex* __restrict__ st,
                                                     const int64_t* __restrict__ vid, uint64_t nv,
                                                     int64_t* __restrict__ src, int64_t* __restrict__ dst,
                                                     int64_t* __restrict__ val, unsigned long long* __restrict__ first) {
  const uint64_t i = (uint64_t)blockIdx.x * kMtBS + threadIdx.x;
  if (i >= ne) return;
  const uint32_t p = pay[i];
  if (p >= ne) return;
  const uint32_t r = rank[p];
  if (r >= nv) return;
  const MtVertex v = st[r];
  if (v.partner >= nv) return;
  if (src) src[i] = vid[r];
  if (dst) dst[i] = vid[v.partner];
  if (val) val[i] = v.value;
  if (first) first[i] = skey[i] ^ kSortSignBit;
}

__global__ __launch_bounds__(kMtBS) void k_mt_mate(const int64_t* __restrict__ rank, uint64_t n,
                                                   const MtVertex* __restrict__ st, const int64_t* __restrict__ vid,
                                                   uint64_t nv, int64_t* __restrict__ mate, int64_t* __restrict__ val,
                                                   uint8_t* __restrict__ found) {
  const uint64_t i = (uint64_t)blockIdx.x * kMtBS + threadIdx.x;
  if (i >= n) return;
  const int64_t r = rank[i];
  int64_t m = 0, x = 0;
  bool hit = false;
  if (r >= 0 && (uint64_t)r < nv) {
    const MtVertex v = st[r];
    if (v.partner != kMtNone && v.partner < nv) {
      hit = true;
      m = vid[v.partner];
      x = v.value;
    }
  }
  if (mate) mate[i] = m;
  if (val) val[i] = x;
  if (found) found[i] = hit ? 1 : 0;
}

uint32_t blocks_of(uint64_t n) { return (uint32_t)((n + kMtBS - 1) / kMtBS); }

}  // namespace

void launch_mt_init(MtVertex* st, uint64_t from, uint64_t to, hipStream_t st_) {
  if (to <= from) return;
  hipLaunchKernelGGL(k_mt_init, dim3(blocks_of(to - from)), dim3(kMtBS), 0, st_, st, from, to);
}

void launch_mt_gather(const uint32_t* vslot, const DistVTable& vt, uint64_t st_cap, const int64_t* val,
                      uint64_t stride, uint64_t n, uint32_t* ru, uint32_t* rv, int64_t* w, uint32_t* list,
                      uint8_t* accepted, unsigned long long* ctl, hipStream_t st) {
  hipLaunchKernelGGL(k_mt_gather, dim3(blocks_of(n)), dim3(kMtBS), 0, st, vslot, (const DistVSlot*)vt.tab,
                     (uint64_t)vt.cap + 1, st_cap, val, stride, n, ru, rv, w, list, accepted, ctl);
}

void launch_mt_round(const MtFold& F, const uint32_t* list, uint64_t np, uint32_t* list_out, uint32_t iter_cap,
                     int sharpen, unsigned long long* ctl, hipStream_t st) {
  const dim3 g(blocks_of(np)), b(kMtBS);
  hipLaunchKernelGGL(k_mt_reset, g, b, 0, st, F, list, np, F.n, ctl);
  hipLaunchKernelGGL(k_mt_seed, g, b, 0, st, F, list, np, F.n, ctl);
  for (uint32_t k = 1; k <= iter_cap; ++k) hipLaunchKernelGGL(k_mt_pass, g, b, 0, st, F, list, np, F.n, sharpen, k, ctl);
  hipLaunchKernelGGL(k_mt_lower, g, b, 0, st, F, list, np, F.n, iter_cap, ctl);
  hipLaunchKernelGGL(k_mt_remain, g, b, 0, st, F, list, np, F.n, sharpen, ctl);
  hipLaunchKernelGGL(k_mt_commit, g, b, 0, st, F, list, np, F.n, list_out, ctl);
}

void launch_mt_tail(const MtFold& F, uint32_t* la, uint32_t* lb, uint64_t np, uint32_t iter_cap, int sharpen,
                    unsigned long long* ctl, hipStream_t st) {
  hipLaunchKernelGGL(k_mt_tail, dim3(1), dim3(kMtTailBS), 0, st, F, la, lb, (uint32_t)np, F.n, iter_cap, sharpen, ctl);
}

void launch_mt_event_count(const uint8_t* accepted, const MtRec* rec, const int64_t* w, uint64_t n, uint32_t* blk,
                           unsigned long long* ctl, hipStream_t st) {
  hipLaunchKernelGGL(k_mt_event_count, dim3((uint32_t)mt_tiles(n)), dim3(kMtBS), 0, st, accepted, rec, w, n, blk, ctl);
}

void launch_mt_event_write(const uint8_t* accepted, const MtRec* rec, const uint32_t* ru, const uint32_t* rv,
                           const int64_t* w, uint64_t n, const uint32_t* blk, const int64_t* vid, uint64_t nv,
                           uint32_t* arrival, uint8_t* type, int64_t* src, int64_t* dst, int64_t* val, uint64_t cap,
                           hipStream_t st) {
  hipLaunchKernelGGL(k_mt_event_write, dim3((uint32_t)mt_tiles(n)), dim3(kMtBS), 0, st, accepted, rec, ru, rv, w, n,
                     blk, vid, nv, arrival, type, src, dst, val, cap);
}

void launch_mt_export(const MtVertex* st, uint64_t nv, int64_t* stamp, uint32_t* rank, uint64_t cap,
                      unsigned long long* ctl, hipStream_t st_) {
  hipLaunchKernelGGL(k_mt_export, dim3(blocks_of(nv)), dim3(kMtBS), 0, st_, st, nv, stamp, rank, cap, ctl);
}

void launch_mt_decode(const unsigned long long* skey, const uint32_t* pay, const uint32_t* rank, uint64_t ne,
                      const MtVertex* st, const int64_t* vid, uint64_t nv, int64_t* src, int64_t* dst, int64_t* val,
                      unsigned long long* first, hipStream_t st_) {
  hipLaunchKernelGGL(k_mt_decode, dim3(blocks_of(ne)), dim3(kMtBS), 0, st_, skey, pay, rank, ne, st, vid, nv, src, dst,
                     val, first);
}

void launch_mt_mate(const int64_t* rank, uint64_t n, const MtVertex* st, const int64_t* vid, uint64_t nv,
                    int64_t* mate, int64_t* val, uint8_t* found, hipStream_t st_) {
  hipLaunchKernelGGL(k_mt_mate, dim3(blocks_of(n)), dim3(kMtBS), 0, st_, rank, n, st, vid, nv, mate, val, found);
}

}  // namespace gs
