// gs_hot_k.hip -- building the hot index of the plain CC fold (HotBucket in gs_device.hpp; how
// the fold uses it: fold_block<..., HOT> in gs_kernels.hip; when it is built: hot_after_fold in
// gs_capi.cpp).
//
// A build reads the first n edges of one micro-batch, on the stream that has just folded it:
//   count  : endpoint occurrences into a sketch of one or two rows (per row 2^sketch_log2
//            counters per id the index can hold, addressed by a row's own hash of the id: no
//            keys, no probing; a collision only overstates a count, and an id's count is the
//            smaller of its rows' counters). The count passes of up to three earlier folds may
//            have added their occurrences to the same sketch (launch_hot_count behind each of
//            those folds; candidates still come from the build's own fold only);
//   select : per bucket the two highest ranks {count, tag} among its ids, in one pass: a 64-bit
//            max takes the winner, and whatever loses to it or is displaced by it goes into a
//            second max, which so ends as the highest rank below the winner's;
//   claim  : one occurrence of each of the two claims its place and looks its id up in the
//            relabel table (read-only). An id the table does not hold yet stays out;
//   root   : per place the root of the claimed slot (read-only find), and a vote among a sample
//            of the places for the root most of them reach: the build's ancestor G;
//   place  : per bucket one 16-B store of the keys whose root is G (kEmpty for the others), and
//            the header {G, G2 = G} behind the buckets (G was a root when a find ended there; a
//            fold may have hooked it since: G2 then lags until the first refresh, which only
//            costs one-hit settles).
// Ids under other roots stay out: one index serves one component, the one that dominates the
// sampled hot ids. Between builds a refresh (k_hot_refresh) finds G's root again into G2.
// Equal ids of a wave are combined before any atomic: a hub's occurrences would otherwise queue
// same-address atomics at the memory side (11.4 ns each, profiles/r01_calib_atomic.log).
// Folds run beside a build and hook and split paths while it reads the table. Every link the
// find reads is an ancestor (the concurrency model in gs_device.hpp), so a place whose find
// ended at G is under G for good, whatever G's own parent has become since.
#include "gs_kernels.hpp"

namespace gs {

namespace {

constexpr uint32_t kHotBS = 256;
constexpr uint32_t kVoteCells = 1024;  // hashed vote counters
// Every 8th block of k_hot_root votes: places are hash positions, so any blocks are a uniform
// sample of the claimed ids, and 1/8 of 2^17 places is ample for a majority. A grid of up to 64
// blocks (2^14 ids) votes whole: a sample of few places could be all unclaimed, and a build
// without votes holds no key.
constexpr uint32_t kVoteEvery = 8;
constexpr int kVoteRounds = 8;         // distinct roots a wave votes for at most

// The sketch: `rows` rows of 2^bits counters (bits = sketch_log2 + log2 ids <= 31).
struct HotSketch {
  uint32_t* c;
  int rows, bits;
};
__device__ __forceinline__ uint32_t sketch_pos(int64_t key, int row, int bits) {
  const uint64_t mul = row ? 0xA24BAED4963EE407ull : 0xC2B2AE3D27D4EB4Full;  // two odd constants: independent rows
  return ((uint32_t)row << bits) + (uint32_t)(((uint64_t)key * mul) >> (64 - bits));
}
__device__ __forceinline__ uint32_t sketch_count(const HotSketch& k, int64_t key) {
  uint32_t c = k.c[sketch_pos(key, 0, k.bits)];
  if (k.rows > 1) c = min(c, k.c[sketch_pos(key, 1, k.bits)]);
  return c;
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

// The build's scratch, in 64-bit words; everything up to `keys` is zeroed before a build.
struct HotScratch {
  unsigned long long* best1;  // [buckets] the highest rank of a bucket (0: none, or claimed)
  unsigned long long* best2;  // [buckets] the highest rank below it
  unsigned long long* vote;   // {votes << 32 | root} of the root with the most votes so far
  uint32_t* cells;            // [kVoteCells] votes by hashed root
  uint32_t* slot1;            // [ids] place 2 * bucket + {0, 1}: the claimed slot + 1 (0: none)
  HotSketch sketch;           // [rows << (sketch_log2 + log2 ids)]
  int64_t* keys;              // [ids] the place's key (where slot1 != 0)
  uint32_t* root;             // [ids] the place's root (where slot1 != 0)
};
inline uint64_t scratch_zeroed_words(int log2_ids, const HotTune& tune) {
  const uint64_t ids = 1ull << log2_ids;
  return ids /* best1, best2 */ + 1 + kVoteCells / 2 + (ids + 1) / 2 +
         (((uint64_t)tune.rows << (tune.sketch_log2 + log2_ids)) + 1) / 2;
}
inline HotScratch scratch_of(unsigned long long* w, int log2_ids, const HotTune& tune) {
  const uint64_t ids = 1ull << log2_ids, buckets = ids >> 1;
  HotScratch s;
  s.best1 = w;
  s.best2 = s.best1 + buckets;
  s.vote = s.best2 + buckets;
  s.cells = reinterpret_cast<uint32_t*>(s.vote + 1);
  s.slot1 = s.cells + kVoteCells;
  s.sketch = HotSketch{s.slot1 + ids, tune.rows, tune.sketch_log2 + log2_ids};
  s.keys = reinterpret_cast<int64_t*>(w + scratch_zeroed_words(log2_ids, tune));
  s.root = reinterpret_cast<uint32_t*>(s.keys + ids);
  return s;
}

// endpoint j (0: src, 1: dst) of the thread's edge; false past the sample or for kEmpty
__device__ __forceinline__ bool sample_key(const HotSample& s, int j, int64_t& key) {
  const uint32_t i = blockIdx.x * kHotBS + threadIdx.x;
  key = 0;
  if (i >= s.n) return false;
  key = (j ? s.dst : s.src)[(size_t)i * s.stride];
  return key != kEmpty;
}

__global__ __launch_bounds__(kHotBS) void k_hot_count(HotSample s, HotSketch sketch) {
  __shared__ uint32_t elect[kHotBS / 64][128], dups[kHotBS / 64][64];
  const uint32_t wv = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    int64_t key;
    uint32_t cnt;
    const bool has = sample_key(s, j, key);
    if (!wave_combine(key, has, elect[wv], dups[wv], cnt)) continue;
    for (int row = 0; row < sketch.rows; ++row) atomicAdd(&sketch.c[sketch_pos(key, row, sketch.bits)], cnt);
  }
}

__global__ __launch_bounds__(kHotBS) void k_hot_select(HotSample s, HotScratch x, int log2_ids) {
  __shared__ uint32_t elect[kHotBS / 64][128], dups[kHotBS / 64][64];
  const uint32_t wv = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    int64_t key;
    uint32_t cnt;
    const bool has = sample_key(s, j, key);
    if (!wave_combine(key, has, elect[wv], dups[wv], cnt)) continue;
    const unsigned long long r = hot_rank(sketch_count(x.sketch, key), key);
    const uint32_t p = hot_pos(key, 65 - log2_ids);
    // (the plain reads may be stale, that is lower: a stale read only costs an atomic)
    const unsigned long long seen = x.best1[p];
    if (seen == r) continue;  // another occurrence of this id brought its rank
    unsigned long long lower = r;  // the rank that did not stay in best1: r, or the one r displaced
    if (seen < r) {
      const unsigned long long old = atomicMax(x.best1 + p, r);
      if (old == r) continue;
      lower = old < r ? old : r;
    }
    if (lower && x.best2[p] < lower) atomicMax(x.best2 + p, lower);
  }
}

__global__ __launch_bounds__(kHotBS) void k_hot_claim(Table t, HotSample s, HotScratch x, int log2_ids) {
  __shared__ uint32_t elect[kHotBS / 64][128], dups[kHotBS / 64][64];
  const uint32_t wv = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    int64_t key;
    uint32_t cnt;
    const bool has = sample_key(s, j, key);
    if (!wave_combine(key, has, elect[wv], dups[wv], cnt)) continue;
    const unsigned long long r = hot_rank(sketch_count(x.sketch, key), key);  // >= 2^32: the id was counted
    const uint32_t p = hot_pos(key, 65 - log2_ids);
    const bool second = x.best1[p] != r;
    unsigned long long* b = (second ? x.best2 : x.best1) + p;
    // one occurrence of a ranked id claims its place (two ids of one rank: the first to claim)
    if (*b != r || atomicCAS(b, r, 0ull) != r) continue;
    uint32_t link = 0;
    const uint32_t slot = lookup_find(t, key, link);
    if (slot == kNoSlot) continue;
    x.keys[2 * p + second] = key;
    x.slot1[2 * p + second] = slot + 1;
  }
}

__global__ __launch_bounds__(kHotBS) void k_hot_root(Table t, HotScratch x, uint32_t ids) {
  const uint32_t i = blockIdx.x * kHotBS + threadIdx.x;
  uint32_t root = kNoSlot;
  if (i < ids && x.slot1[i]) {
    const uint32_t slot = x.slot1[i] - 1;
    int64_t k = 0;
    uint32_t l = 0, par = 0;
    load_slot(t.tab + slot, k, l);
    root = find_ro(t, slot, l, k, par);
    x.root[i] = root;
  }
  if (gridDim.x > 8 * kVoteEvery && blockIdx.x % kVoteEvery) return;
  // the wave's votes, one pair of atomics per distinct root: the root whose counter reaches the
  // highest value leaves {that value, root} in *vote
  const int lane = (int)(threadIdx.x & 63u);
  bool pend = root != kNoSlot;
  for (int round = 0; round < kVoteRounds; ++round) {
    const unsigned long long m = __ballot(pend);
    if (!m) break;
    const int leader = __ffsll((long long)m) - 1;
    const uint32_t r0 = (uint32_t)__shfl((int)root, leader, 64);
    const bool same = pend && root == r0;
    const uint32_t n = (uint32_t)__popcll(__ballot(same));
    if (lane == leader) {
      const uint32_t c = atomicAdd(&x.cells[(r0 * 0x9E3779B1u) >> 22], n) + n;
      atomicMax(x.vote, ((unsigned long long)c << 32) | r0);
    }
    if (same) pend = false;
  }
}

__global__ __launch_bounds__(kHotBS) void k_hot_place(HotScratch x, HotBucket* out, uint32_t buckets) {
  const uint32_t p = blockIdx.x * kHotBS + threadIdx.x;
  if (p >= buckets) return;
  const unsigned long long v = *x.vote;
  const uint32_t g = v ? (uint32_t)v : kNoSlot;
  const bool h0 = x.slot1[2 * p] && x.root[2 * p] == g, h1 = x.slot1[2 * p + 1] && x.root[2 * p + 1] == g;
  const uint64_t k0 = (uint64_t)(h0 ? x.keys[2 * p] : kEmpty), k1 = (uint64_t)(h1 ? x.keys[2 * p + 1] : kEmpty);
  *reinterpret_cast<uint4*>(out + p) =
      make_uint4((uint32_t)k0, (uint32_t)(k0 >> 32), (uint32_t)k1, (uint32_t)(k1 >> 32));
  if (p == 0) *reinterpret_cast<uint4*>(out + buckets) = make_uint4(g, g, 0u, 0u);  // HotHeader {g, g2}
}

// Refresh: the root found again from G, into the live header's G2. After the index's component
// is hooked under a smaller id, a cold vertex of it hangs under the new root, not under G: the
// one-hit edges stop settling until G2 names the new root (the both-hit edges never stop). One
// lane and a chain of a link or two. The folds read the header meanwhile: whichever value of
// G2 they see was a root above G. The address is uniform, so the compiler walks the chain with
// scalar loads, through the scalar cache: a link it reads may be older than what the L2 holds.
// That is as good -- a stale link is still an ancestor, so the slot found is one of G's
// ancestors, at worst not yet its root -- and the reads need not be made fresh.
__global__ __launch_bounds__(64) void k_hot_refresh(Table t, HotHeader* h) {
  if (threadIdx.x) return;
  const uint32_t g = h->g;
  if (g == kNoSlot) return;
  int64_t k = 0;
  uint32_t l = 0, par = 0;
  load_slot(t.tab + g, k, l);
  h->g2 = find_ro(t, g, l, k, par);
}

}  // namespace

uint64_t hot_scratch_words(int log2_ids, const HotTune& tune) {
  const uint64_t ids = 1ull << log2_ids;
  return scratch_zeroed_words(log2_ids, tune) + ids + (ids + 1) / 2;  // + keys, root
}

void launch_hot_zero(int log2_ids, const HotTune& tune, unsigned long long* scratch, hipStream_t st) {
  (void)hipMemsetAsync(scratch, 0, scratch_zeroed_words(log2_ids, tune) * 8, st);
}

void launch_hot_count(const int64_t* src, const int64_t* dst, uint32_t n, uint32_t stride, int log2_ids,
                      const HotTune& tune, unsigned long long* scratch, hipStream_t st) {
  if (!n) return;
  const HotScratch x = scratch_of(scratch, log2_ids, tune);
  const HotSample s{src, dst, n, stride};
  hipLaunchKernelGGL(k_hot_count, dim3((n + kHotBS - 1) / kHotBS), dim3(kHotBS), 0, st, s, x.sketch);
}

void launch_hot_build(const Table& t, const int64_t* src, const int64_t* dst, uint32_t n, uint32_t stride,
                      HotBucket* out, int log2_ids, const HotTune& tune, unsigned long long* scratch, hipStream_t st) {
  const uint32_t ids = 1u << log2_ids, buckets = (uint32_t)hot_buckets(log2_ids);
  const HotScratch x = scratch_of(scratch, log2_ids, tune);
  const HotSample s{src, dst, n, stride};
  const dim3 g((n + kHotBS - 1) / kHotBS), b(kHotBS);
  hipLaunchKernelGGL(k_hot_count, g, b, 0, st, s, x.sketch);
  hipLaunchKernelGGL(k_hot_select, g, b, 0, st, s, x, log2_ids);
  hipLaunchKernelGGL(k_hot_claim, g, b, 0, st, t, s, x, log2_ids);
  hipLaunchKernelGGL(k_hot_root, dim3((ids + kHotBS - 1) / kHotBS), b, 0, st, t, x, ids);
  hipLaunchKernelGGL(k_hot_place, dim3((buckets + kHotBS - 1) / kHotBS), b, 0, st, x, out, buckets);  // every bucket
}

void launch_hot_refresh(const Table& t, HotBucket* live, int log2_ids, hipStream_t st) {
  hipLaunchKernelGGL(k_hot_refresh, dim3(1), dim3(64), 0, st, t, reinterpret_cast<HotHeader*>(live + hot_buckets(log2_ids)));
}

}  // namespace gs
