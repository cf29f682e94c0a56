// gs_hot_k.hip -- building the hot index of the plain CC fold (HotEntry in gs_device.hpp; how
// the fold uses it: fold_block<..., HOT> in gs_kernels.hip; when it is built: hot_after_fold in
// gs_capi.cpp).
//
// A build reads the first n edges of one micro-batch, on the stream that has just folded it:
//   count  : endpoint occurrences into a one-row sketch (16 counters per index entry, addressed
//            by a hash of the id: no keys, no probing; a collision only overstates a count);
//   select : per index position the occurrence with the highest {count, tag} (64-bit max);
//   place  : the position's winner is looked up in the relabel table (read-only), its root found
//            (read-only find) and its entry {key, slot, root} written with one 16-B store. An id
//            the table does not hold yet stays out.
// Between builds a refresh (k_hot_refresh) renews the ancestors of the entries as they are.
// Equal ids of a wave are combined before any atomic: a hub's occurrences would otherwise queue
// same-address atomics at the memory side (11.4 ns each, profiles/r01_calib_atomic.log).
// Folds run beside a build and hook and split paths while it reads the table. Every link the
// find reads is an ancestor (the concurrency model in gs_device.hpp), so whatever root it
// reaches is a valid `anc`.
#include "gs_kernels.hpp"

namespace gs {

namespace {

constexpr int kHotSketchLog2 = 4;  // sketch counters per index entry (log2)
constexpr uint32_t kHotBS = 256;

__device__ __forceinline__ uint32_t sketch_pos(int64_t key, int log2_entries) {
  return (uint32_t)(((uint64_t)key * 0xC2B2AE3D27D4EB4Full) >> (64 - kHotSketchLog2 - log2_entries));
}
__device__ __forceinline__ unsigned long long hot_rank(uint32_t count, int64_t key) {
  return ((unsigned long long)count << 32) | (uint32_t)(((uint64_t)key * 0x9E3779B97F4A7C15ull) >> 32);
}

// Combine the equal ids of a wave: true in the lanes that go on (one per distinct id, bar the
// rare lane that lost its election slot to another id), cnt = the occurrences a lane stands
// for. elect[128] and dups[64] are the wave's LDS. Called by every thread of the block.
__device__ __forceinline__ bool wave_combine(int64_t key, bool has, uint32_t* elect, uint32_t* dups, uint32_t& cnt) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t e = (uint32_t)(((uint64_t)key * 0x9E3779B97F4A7C15ull) >> 57);
  __syncthreads();  // the previous call's reads are done
  dups[lane] = 0;
  if (has) elect[e] = lane;
  __syncthreads();
  const uint32_t w = has ? elect[e] : lane;  // a lane that wrote e this round
  const int64_t kw = __shfl(key, (int)w, 64);
  const bool dup = has && w != lane && kw == key;
  if (dup) atomicAdd(&dups[w], 1u);
  __syncthreads();
  cnt = 1u + dups[lane];
  return has && !dup;
}

struct HotSample {
  const int64_t* src;
  const int64_t* dst;
  uint32_t n, stride;
};

// endpoint j (0: src, 1: dst) of the thread's edge; false past the sample or for kEmpty
__device__ __forceinline__ bool sample_key(const HotSample& s, int j, int64_t& key) {
  const uint32_t i = blockIdx.x * kHotBS + threadIdx.x;
  key = 0;
  if (i >= s.n) return false;
  key = (j ? s.dst : s.src)[(size_t)i * s.stride];
  return key != kEmpty;
}

__global__ __launch_bounds__(kHotBS) void k_hot_count(HotSample s, uint32_t* sketch, int log2_entries) {
  __shared__ uint32_t elect[kHotBS / 64][128], dups[kHotBS / 64][64];
  const uint32_t wv = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    int64_t key;
    uint32_t cnt;
    const bool has = sample_key(s, j, key);
    if (wave_combine(key, has, elect[wv], dups[wv], cnt)) atomicAdd(&sketch[sketch_pos(key, log2_entries)], cnt);
  }
}

__global__ __launch_bounds__(kHotBS) void k_hot_select(HotSample s, const uint32_t* sketch, unsigned long long* best,
                                                       int log2_entries) {
  __shared__ uint32_t elect[kHotBS / 64][128], dups[kHotBS / 64][64];
  const uint32_t wv = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    int64_t key;
    uint32_t cnt;
    const bool has = sample_key(s, j, key);
    if (!wave_combine(key, has, elect[wv], dups[wv], cnt)) continue;
    const unsigned long long r = hot_rank(sketch[sketch_pos(key, log2_entries)], key);
    unsigned long long* b = best + hot_pos(key, 64 - log2_entries);
    if (*b < r) atomicMax(b, r);  // (a stale read only costs an atomic)
  }
}

__global__ __launch_bounds__(kHotBS) void k_hot_place(Table t, HotSample s, const uint32_t* sketch,
                                                      unsigned long long* best, HotEntry* out, int log2_entries) {
  __shared__ uint32_t elect[kHotBS / 64][128], dups[kHotBS / 64][64];
  const uint32_t wv = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    int64_t key;
    uint32_t cnt;
    const bool has = sample_key(s, j, key);
    if (!wave_combine(key, has, elect[wv], dups[wv], cnt)) continue;
    const unsigned long long r = hot_rank(sketch[sketch_pos(key, log2_entries)], key);  // >= 2^32: the id was counted
    const uint32_t p = hot_pos(key, 64 - log2_entries);
    // one occurrence of the winner claims the position (two ids of one rank: the first to claim)
    if (best[p] != r || atomicCAS(best + p, r, 0ull) != r) continue;
    uint32_t link = 0;
    const uint32_t slot = lookup_find(t, key, link);
    if (slot == kNoSlot) continue;
    int64_t kroot = key;
    uint32_t par = 0;
    const uint32_t root = find_ro(t, slot, link, kroot, par);
    *reinterpret_cast<uint4*>(out + p) = make_uint4((uint32_t)(uint64_t)key, (uint32_t)((uint64_t)key >> 32), slot, root);
  }
}

// Refresh: the live index's entries with their ancestors found again (from the old ancestor on:
// an ancestor's root is an ancestor), into the other buffer. After the component of most hot ids
// is hooked under a smaller id every entry names the old root, whose parent no other vertex
// keeps for long: the entries stop settling edges until their ancestors are renewed. One thread
// per entry and a chain of a link or two each: a few microseconds against a build's three passes.
__global__ __launch_bounds__(kHotBS) void k_hot_refresh(Table t, const HotEntry* in, HotEntry* out, uint32_t n) {
  const uint32_t i = blockIdx.x * kHotBS + threadIdx.x;
  if (i >= n) return;
  uint4 v = *reinterpret_cast<const uint4*>(in + i);
  if (v.z != kNoSlot) {
    int64_t k = 0;
    uint32_t l = 0, par = 0;
    load_slot(t.tab + v.w, k, l);
    v.w = find_ro(t, v.w, l, k, par);
  }
  *reinterpret_cast<uint4*>(out + i) = v;
}

}  // namespace

uint64_t hot_scratch_words(int log2_entries) {
  return (1ull << log2_entries) + ((1ull << (log2_entries + kHotSketchLog2)) >> 1);  // best (u64) + sketch (u32)
}

void launch_hot_build(const Table& t, const int64_t* src, const int64_t* dst, uint32_t n, uint32_t stride,
                      HotEntry* out, int log2_entries, unsigned long long* scratch, hipStream_t st) {
  const uint64_t entries = 1ull << log2_entries;
  unsigned long long* best = scratch;
  uint32_t* sketch = reinterpret_cast<uint32_t*>(scratch + entries);
  (void)hipMemsetAsync(scratch, 0, hot_scratch_words(log2_entries) * 8, st);
  (void)hipMemsetAsync(out, 0xFF, entries * sizeof(HotEntry), st);  // slot == kNoSlot: empty
  const HotSample s{src, dst, n, stride};
  const dim3 g((n + kHotBS - 1) / kHotBS), b(kHotBS);
  hipLaunchKernelGGL(k_hot_count, g, b, 0, st, s, sketch, log2_entries);
  hipLaunchKernelGGL(k_hot_select, g, b, 0, st, s, sketch, best, log2_entries);
  hipLaunchKernelGGL(k_hot_place, g, b, 0, st, t, s, sketch, best, out, log2_entries);
}

void launch_hot_refresh(const Table& t, const HotEntry* in, HotEntry* out, int log2_entries, hipStream_t st) {
  const uint32_t n = 1u << log2_entries;
  hipLaunchKernelGGL(k_hot_refresh, dim3((n + kHotBS - 1) / kHotBS), dim3(kHotBS), 0, st, t, in, out, n);
}

}  // namespace gs
