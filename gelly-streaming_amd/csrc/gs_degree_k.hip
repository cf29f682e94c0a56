// gs_degree_k.hip -- kernels of the degree summary (gfx950).
//
//   k_degree_fold   : a workgroup takes a tile of edges (DEGREE_TILE, 8 per thread), sums
//                     the tile's endpoint occurrences per id in an LDS hash keyed by id,
//                     then adds each distinct id's sum to its counter with ONE memory-side
//                     atomic. A hub of the stream costs one global add per tile instead of
//                     one per occurrence (same-address atomics serialise at the memory
//                     side, gs_device.hpp reserve_new_vertices).
//   k_degree_find   : batched read of counters
//   k_degree_export : table scan -> unordered (vertex, count) rows
//   k_degree_gather / k_degree_heads / k_degree_runs : tails of the sorted export and of
//                     the degree distribution (the sort itself is gs_sort_k.hip's)
//
// Concurrency: the relabel probe / insert is gs_device.hpp's (key CAS settles stale EMPTY
// reads); counters are only ever changed by atomicAdd on the slot's link word and never
// read inside the fold launch, so no load has to be fresh. Ids that do not fit the LDS
// hash (its bounded probe failed, or the id is INT64_MIN, the hash's empty marker) take
// the same global path directly, one atomic per occurrence. Every loop is bounded; no
// workgroup waits on another.
#include "gs_degree.hpp"

namespace gs {
namespace {

struct DegreeArgs {
  const int64_t* src;
  const int64_t* dst;
  const uint8_t* del;
  const int64_t* wt;
  uint32_t n;
  uint32_t stride;
  int dir;
  uint32_t shard0;
};

// Probe / insert up to two ids and add their weights to their counters. Both first probes
// go out back to back; a pair of EMPTY first probes inserts with paired key CASes (k_fold's
// insert path). New vertices are registered with one reservation atomic per wave. Call in
// wave-uniform control flow (lanes with nothing to do pass va = vb = false).
template <bool ADD>
__device__ __forceinline__ void global_add_pair(const Table& t, int shard, bool va, int64_t ka, int wa, bool vb,
                                                int64_t kb, int wb) {
  const uint32_t hu = hash_slot(ka, t.shift), hv = hash_slot(kb, t.shift);
  int64_t k0u = 0, k0v = 0;
  uint32_t l0u = 0, l0v = 0;
  if (va && ka != kEmpty) load_slot(t.tab + hu, k0u, l0u);
  if (vb && kb != kEmpty) load_slot(t.tab + hv, k0v, l0v);
  uint32_t su = kNoSlot, sv = kNoSlot, lu = 0, lv = 0;
  bool nu = false, nv = false;
  if (va && vb && k0u == kEmpty && k0v == kEmpty && hu != hv && ka != kb && ka != kEmpty && kb != kEmpty) {
    insert_pair<false, false>(t, ka, hu, kb, hv, su, lu, nu, sv, lv, nv);
  } else {
    if (va) su = lookup_resolve<false>(t, ka, hu, k0u, l0u, lu, nu);
    if (vb) sv = lookup_resolve<false>(t, kb, hv, k0v, l0v, lv, nv);
  }
  const NewVertices nvx = reserve_new_vertices(t, shard, nu, su, nv, sv);  // one atomic per wave
  // no-return adds: a table overflow (kNoSlot) raised the error flag, nothing is added
  if (ADD && va && su != kNoSlot && wa) atomicAdd(&t.tab[su].link, (uint32_t)wa);
  if (ADD && vb && sv != kNoSlot && wb) atomicAdd(&t.tab[sv].link, (uint32_t)wb);
  write_new_vertices(t, shard, nvx);
}

// One occurrence into the LDS hash: claim or find the id's slot within kDegreeLdsProbes
// linear probes and add w there. false: no slot (the caller adds it globally).
template <uint32_t LOGL>
__device__ __forceinline__ bool lds_add(unsigned long long* lkey, int* lcnt, int64_t key, int w) {
  constexpr uint32_t kMask = (1u << LOGL) - 1u;
  uint32_t h = (uint32_t)(((uint64_t)key * 0x9E3779B97F4A7C15ull) >> (64 - LOGL));
#pragma unroll
  for (uint32_t p = 0; p < kDegreeLdsProbes; ++p) {
    const unsigned long long old = atomicCAS(&lkey[h], (unsigned long long)kEmpty, (unsigned long long)key);
    if (old == (unsigned long long)kEmpty || old == (unsigned long long)key) {
      atomicAdd(&lcnt[h], w);
      return true;
    }
    h = (h + 1u) & kMask;
  }
  return false;
}

// One endpoint class of a wave's 64 edges into the LDS hash (every lane calls it; c: the lane
// holds an occurrence of `key` with weight w = +1 / -1). A wave whose occurrences all name one
// id -- a star's centre, repeated self-loops -- adds their sum once instead of 64 times to one
// LDS address. Returns whether the lane's occurrence is still to be added globally.
template <uint32_t LOGL>
__device__ __forceinline__ bool lds_add_wave(unsigned long long* lkey, int* lcnt, bool c, int64_t key, int w) {
  const unsigned long long m = __ballot(c);
  if (!m) return false;  // wave-uniform
  const int first = __ffsll((long long)m) - 1;
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)(uint64_t)key, first, 64);
  const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)((uint64_t)key >> 32), first, 64);
  const int64_t k0 = (int64_t)(((uint64_t)hi << 32) | lo);
  if (__popcll(m) >= 2 && __ballot(c && key != k0) == 0ull) {  // wave-uniform
    const int sum = __popcll(__ballot(c && w > 0)) - __popcll(__ballot(c && w < 0));
    int ok = 0;
    if ((int)(threadIdx.x & 63u) == first && k0 != kEmpty) ok = lds_add<LOGL>(lkey, lcnt, k0, sum) ? 1 : 0;
    ok = __shfl(ok, first, 64);
    return c && !ok;
  }
  return c && (key == kEmpty || !lds_add<LOGL>(lkey, lcnt, key, w));
}

// ITEMS edges per thread; COMBINE: the LDS hash of 2^LOGL slots (else every occurrence goes
// to global_add_pair directly: the row form, and the A/B of tools/degree_bench.py). ADD = false
// is the bench's diagnostic without the counter adds.
template <uint32_t ITEMS, uint32_t LOGL, bool COMBINE, bool ADD = true>
__global__ __launch_bounds__(kDegreeBS) void k_degree_fold(Table t, DegreeArgs a) {
  constexpr uint32_t L = COMBINE ? (1u << LOGL) : 1u;
  static_assert(!COMBINE || L >= 2 * kDegreeBS, "the flush handles two LDS slots per thread and iteration");
  __shared__ unsigned long long lkey[L];
  __shared__ int lcnt[L];
  const uint32_t tid = threadIdx.x;
  const uint32_t wave = tid >> 6;
  const uint32_t base = blockIdx.x * (kDegreeBS * ITEMS);
  if constexpr (COMBINE) {
    for (uint32_t s = tid; s < L; s += kDegreeBS) {
      lkey[s] = (unsigned long long)kEmpty;
      lcnt[s] = 0;
    }
    __syncthreads();
  }
  // vertex-list shard of a (call, wave): rotates so that a tile's new vertices spread over
  // the shards (reserve and write of one call use the same shard)
  uint32_t call = a.shard0 + blockIdx.x * (ITEMS + (COMBINE ? L / (2 * kDegreeBS) : 0u)) * 4u + wave;
  const bool rows = a.wt != nullptr;
#pragma unroll 2
  for (uint32_t j = 0; j < ITEMS; ++j, call += 4u) {
    const uint32_t i = base + j * kDegreeBS + tid;
    const bool valid = i < a.n;
    // the edge stream is read once: non-temporal loads leave the L2 to table lines
    const int64_t ks = valid ? __builtin_nontemporal_load(a.src + (size_t)i * a.stride) : 0;
    const int64_t kd = (valid && !rows) ? __builtin_nontemporal_load(a.dst + (size_t)i * a.stride) : 0;
    int w = 1;
    if (valid && rows) w = (int)a.wt[i];
    if (valid && a.del && (a.del[i] & 1u)) w = -1;
    bool fa = valid && (rows || a.dir != kDegreeIn);
    bool fb = valid && !rows && a.dir != kDegreeOut;
    if constexpr (COMBINE) {
      fa = lds_add_wave<LOGL>(lkey, lcnt, fa, ks, w);
      fb = lds_add_wave<LOGL>(lkey, lcnt, fb, kd, w);
    }
    if (__ballot(fa || fb) != 0ull)  // wave-uniform
      global_add_pair<ADD>(t, (int)(call & (uint32_t)(kShards - 1)), fa, ks, w, fb, kd, w);
  }
  if constexpr (COMBINE) {
    __syncthreads();
    for (uint32_t s = tid; s < L; s += 2 * kDegreeBS, call += 4u) {
      const int64_t ka = (int64_t)lkey[s], kb = (int64_t)lkey[s + kDegreeBS];
      const bool va = ka != kEmpty, vb = kb != kEmpty;
      if (__ballot(va || vb) != 0ull)  // wave-uniform
        global_add_pair<ADD>(t, (int)(call & (uint32_t)(kShards - 1)), va, ka, lcnt[s], vb, kb, lcnt[s + kDegreeBS]);
    }
  }
}

__device__ __forceinline__ int slot_degree(uint32_t s, uint32_t link) { return (int)(link - (s << 1)); }

__global__ __launch_bounds__(256) void k_degree_find(Table t, const int64_t* __restrict__ v, uint64_t n,
                                                     int64_t* __restrict__ degree, uint8_t* __restrict__ found) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  uint32_t link = 0;
  const uint32_t s = lookup_find(t, v[i], link);
  const int d = s == kNoSlot ? 0 : slot_degree(s, link);
  degree[i] = d > 0 ? (int64_t)d : 0;
  if (found) found[i] = d > 0 ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_degree_export(Table t, int64_t* __restrict__ ov, int64_t* __restrict__ od,
                                                       uint64_t cap_out, unsigned long long* __restrict__ count,
                                                       int all) {
  const uint64_t step = (uint64_t)gridDim.x * 256;
  for (uint64_t s0 = (uint64_t)blockIdx.x * 256; s0 <= (uint64_t)t.r0; s0 += step) {
    const uint64_t s = s0 + threadIdx.x;
    bool has = false;
    int64_t key = kEmpty;
    int d = 0;
    if (s <= (uint64_t)t.r0) {
      const uint4 x = *reinterpret_cast<const uint4*>(t.tab + s);
      key = (int64_t)(((uint64_t)x.y << 32) | x.x);
      d = slot_degree((uint32_t)s, x.z);
      const bool present = s == (uint64_t)t.r0 ? (x.w & kAuxPresent) != 0 : key != kEmpty;
      has = present && (all || d > 0);
    }
    // one append atomic per wave
    const unsigned long long m = __ballot(has);
    if (!m) continue;
    const int lane = (int)(threadIdx.x & 63u);
    const int leader = __ffsll((long long)m) - 1;
    unsigned long long b = 0;
    if (lane == leader) b = atomicAdd(count, (unsigned long long)__popcll(m));
    const uint32_t blo = (uint32_t)__shfl((int)(uint32_t)b, leader, 64);
    const uint32_t bhi = (uint32_t)__shfl((int)(uint32_t)(b >> 32), leader, 64);
    if (!has) continue;
    const uint64_t pos = (((uint64_t)bhi << 32) | blo) + (uint64_t)__popcll(m & ((1ull << lane) - 1ull));
    if (pos < cap_out) {
      ov[pos] = key;
      od[pos] = (int64_t)d;
    }
  }
}

__global__ __launch_bounds__(256) void k_degree_gather(const uint32_t* __restrict__ pay, const int64_t* __restrict__ v,
                                                       const int64_t* __restrict__ d, uint64_t n,
                                                       int64_t* __restrict__ ov, int64_t* __restrict__ od) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint64_t r = pay ? pay[i] : i;
  if (r >= n) return;  // (a payload is a row index)
  ov[i] = v[r];
  od[i] = d[r];
}

__global__ __launch_bounds__(256) void k_degree_heads(const unsigned long long* __restrict__ key, uint64_t n,
                                                      unsigned long long* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const bool head = i < n && (i == 0 || key[i] != key[i - 1]);
  const unsigned long long m = __ballot(head);
  if (m && (int)(threadIdx.x & 63u) == __ffsll((long long)m) - 1) atomicAdd(out, (unsigned long long)__popcll(m));
}

__global__ __launch_bounds__(256) void k_degree_runs(const int64_t* __restrict__ comp,
                                                     const unsigned long long* __restrict__ off, uint64_t nd,
                                                     int64_t* __restrict__ degree, int64_t* __restrict__ count) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nd) return;
  degree[i] = comp[i];
  count[i] = (int64_t)(off[i + 1] - off[i]);
}

uint32_t grid_of(uint64_t n) { return (uint32_t)((n + 255) / 256); }

}  // namespace

uint32_t degree_tile(int variant) {
  switch (variant) {
    case kDegreeTile1024: return 1024;
    default: return DEGREE_TILE;
  }
}

uint32_t degree_blocks(uint32_t n, int variant) {
  const uint32_t tile = degree_tile(variant);
  return (n + tile - 1) / tile;
}

void launch_degree_fold(const Table& t, const DegreeLaunch& f, int variant, hipStream_t st) {
  if (f.n == 0) return;
  if (f.wt) variant = kDegreeNoCombine;  // rows name distinct ids: nothing to combine
  const DegreeArgs a{f.src, f.dst, f.del, f.wt, f.n, f.stride, f.dir, f.shard0};
  const dim3 grid(degree_blocks(f.n, variant)), block(kDegreeBS);
  switch (variant) {
    case kDegreeNoCombine:
      hipLaunchKernelGGL((k_degree_fold<kDegreeItems, 1, false>), grid, block, 0, st, t, a);
      break;
    case kDegreeLds4096:
      hipLaunchKernelGGL((k_degree_fold<kDegreeItems, 12, true>), grid, block, 0, st, t, a);
      break;
    case kDegreeTile1024:
      hipLaunchKernelGGL((k_degree_fold<4, 11, true>), grid, block, 0, st, t, a);
      break;
    case kDegreeLds2048:
      hipLaunchKernelGGL((k_degree_fold<kDegreeItems, 11, true>), grid, block, 0, st, t, a);
      break;
    case kDegreeProbeOnly:
      hipLaunchKernelGGL((k_degree_fold<kDegreeItems, kDegreeLdsLog2, true, false>), grid, block, 0, st, t, a);
      break;
    default:
      hipLaunchKernelGGL((k_degree_fold<kDegreeItems, kDegreeLdsLog2, true>), grid, block, 0, st, t, a);
      break;
  }
}

void launch_degree_find(const Table& t, const int64_t* v, uint64_t n, int64_t* degree, uint8_t* found,
                        hipStream_t st) {
  if (!n) return;
  hipLaunchKernelGGL(k_degree_find, dim3(grid_of(n)), dim3(256), 0, st, t, v, n, degree, found);
}

void launch_degree_export(const Table& t, int64_t* ov, int64_t* od, uint64_t cap_out, unsigned long long* count,
                          bool all, hipStream_t st) {
  const uint64_t tiles = ((uint64_t)t.r0 + 256) / 256;
  const uint32_t grid = (uint32_t)(tiles < 8192 ? tiles : 8192);
  hipLaunchKernelGGL(k_degree_export, dim3(grid), dim3(256), 0, st, t, ov, od, cap_out, count, all ? 1 : 0);
}

void launch_degree_gather(const uint32_t* pay, const int64_t* v, const int64_t* d, uint64_t n, int64_t* ov,
                          int64_t* od, hipStream_t st) {
  if (!n) return;
  hipLaunchKernelGGL(k_degree_gather, dim3(grid_of(n)), dim3(256), 0, st, pay, v, d, n, ov, od);
}

void launch_degree_heads(const unsigned long long* key, uint64_t n, unsigned long long* out, hipStream_t st) {
  if (!n) return;
  hipLaunchKernelGGL(k_degree_heads, dim3(grid_of(n)), dim3(256), 0, st, key, n, out);
}

void launch_degree_runs(const int64_t* comp, const unsigned long long* off, uint64_t nd, int64_t* degree,
                        int64_t* count, hipStream_t st) {
  if (!nd) return;
  hipLaunchKernelGGL(k_degree_runs, dim3(grid_of(nd)), dim3(256), 0, st, comp, off, nd, degree, count);
}

}  // namespace gs
