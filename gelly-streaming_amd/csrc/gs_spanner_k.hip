// gs_spanner_k.hip -- kernels of the k-spanner summary (gfx950); launchers in gs_spanner.hpp.
//
//   sp_search          : the bounded two-sided search, run by one workgroup (a single wave with
//                        its sets in LDS, or 256 threads with stamp arrays in a global arena). A
//                        ball grows from each endpoint; each of the k steps expands the side with
//                        the smaller frontier (gs_spanner_seq.hpp: sp_pick_side) and ends the
//                        search when a vertex it reaches is in the other side's set.
//   k_sp_query         : within queries and the filter pass (G0 only)
//   k_sp_round         : one round over the undecided pending edges (upper, then lower search)
//   k_sp_tail          : the serial tail, one workgroup
//   k_sp_flag / k_sp_pending / k_sp_compact_pairs : flag, scan (gs_sort.hpp's launch_tile_scan)
//                        and compact: the pending edges, the accepted entries, the export
//   k_sp_gather / k_sp_mark / k_sp_merge / k_sp_count_rows : the passes between them
//
// What bounds every loop:
//   * every binary search halves an index interval inside its array (gs_triangle_rows.hpp);
//   * a row walk runs over [b, e) of the adjacency and [pb, pe) of the pending entries, both
//     from tri_row on the same arrays; a status byte is read only for a pending index j < i,
//     and i is below the number of pending edges;
//   * a probe of an LDS set visits at most `slots` slots; a list position is tested against
//     the list's capacity before the store (an overflow ends the search with verdict 2);
//   * a frontier is a range of list positions below the list's count;
//   * a search makes at most k <= 16 steps; list-driven loops run to the list length the host
//     read back, and every list element is tested against the element count;
//   * every output position of a compaction is tested against the capacity of its array.
// A search reads statuses the launch before wrote (the tail: its own workgroup wrote, behind a
// barrier); sets and frontier lists are private to the workgroup.
#include "gs_scan.hpp"
#include "gs_spanner.hpp"
#include "gs_triangle_rows.hpp"

namespace gs {
namespace {

constexpr int64_t kSpEmptyKey = INT64_MIN;  // empty slot of an LDS set; the id itself has a flag bit instead
constexpr uint64_t kSpNoHandle = ~0ull;
constexpr uint32_t kSpSlotsMax = 2 * kSpannerLdsSet;  // sp_set_slots(kSpannerLdsSet)

__device__ __forceinline__ uint8_t sp_status(const uint8_t* st, uint32_t j) {
  return __hip_atomic_load(st + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// verdicts of a visit
enum : int { kVisOld = 0, kVisNew = 1, kVisFull = 2, kVisMet = 3 };

// Both sets of a wave in LDS: keys[side][slots] open addressing, list[side][cap] in discovery
// order, cnt[side] the list lengths, cnt[2] the presence bits of INT64_MIN.
struct LdsSets {
  int64_t* keys;
  int64_t* list;
  uint32_t* cnt;
  uint32_t slots, cap;

  __device__ void reset() {
    for (uint32_t q = threadIdx.x; q < 2 * slots; q += blockDim.x) keys[q] = kSpEmptyKey;
    if (threadIdx.x < 3) cnt[threadIdx.x] = 0;
    __syncthreads();
  }
  __device__ int append(int side, int64_t v) {
    const uint32_t idx = atomicAdd(&cnt[side], 1u);
    if (idx >= cap) return kVisFull;
    list[side * cap + idx] = v;
    return kVisNew;
  }
  // v joins the set of `side` unless the other side holds it
  __device__ int visit(const SpGraph&, int side, int64_t v) {
    const int other = side ^ 1;
    if (v == kSpEmptyKey) {
      if ((*(volatile uint32_t*)&cnt[2] >> other) & 1u) return kVisMet;
      const uint32_t old = atomicOr(&cnt[2], 1u << side);
      return ((old >> side) & 1u) ? kVisOld : append(side, v);
    }
    const uint32_t h = sp_hash(v, slots), mask = slots - 1;
    const volatile int64_t* ko = keys + other * slots;
    for (uint32_t p = 0; p < slots; ++p) {
      const int64_t key = ko[(h + p) & mask];
      if (key == v) return kVisMet;
      if (key == kSpEmptyKey) break;
    }
    int64_t* km = keys + side * slots;
    for (uint32_t p = 0; p < slots; ++p) {
      const uint32_t s = (h + p) & mask;
      int64_t key = *(volatile int64_t*)&km[s];
      if (key == kSpEmptyKey) {
        key = (int64_t)atomicCAS(reinterpret_cast<unsigned long long*>(&km[s]), (unsigned long long)kSpEmptyKey,
                                 (unsigned long long)v);
        if (key == kSpEmptyKey) return append(side, v);
      }
      if (key == v) return kVisOld;
    }
    return kVisFull;
  }
  __device__ bool seed(const SpGraph& g, int side, int64_t v) { return visit(g, side, v) == kVisNew; }
  __device__ int64_t at(int side, uint32_t idx) const { return list[side * cap + idx]; }
  __device__ uint32_t count(int side) const { return cnt[side] < cap ? cnt[side] : cap; }
};

// Both sets of a heavy search in one arena: stamp[H] by dense vertex number, list[side][H].
struct StampSets {
  uint32_t* stamp;
  int64_t* list;
  uint64_t H;
  uint32_t* cnt;  // LDS
  uint32_t gen;

  __device__ void reset() {
    if (threadIdx.x < 2) cnt[threadIdx.x] = 0;
    __syncthreads();
  }
  __device__ static uint64_t handle(const SpGraph& g, int64_t v) {
    const uint64_t p = tri_lower(g.ax, 0, g.n0, v);
    if (p < g.n0 && g.ax[p] == v) return p;
    const uint64_t q = tri_lower(g.px, 0, g.np, v);
    if (q < g.np && g.px[q] == v) return g.n0 + q;
    return kSpNoHandle;
  }
  __device__ int visit(const SpGraph& g, int side, int64_t v) {
    const uint64_t h = handle(g, v);
    if (h >= H) return kVisFull;
    const uint32_t mine = sp_stamp(gen, side), theirs = sp_stamp(gen, side ^ 1);
    if (__hip_atomic_load(stamp + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == theirs) return kVisMet;
    if (atomicExch(stamp + h, mine) == mine) return kVisOld;
    const uint32_t idx = atomicAdd(&cnt[side], 1u);
    if (idx >= H) return kVisFull;
    __hip_atomic_store(list + side * H + idx, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return kVisNew;
  }
  __device__ bool seed(const SpGraph& g, int side, int64_t v) { return visit(g, side, v) == kVisNew; }
  __device__ int64_t at(int side, uint32_t idx) const {
    return __hip_atomic_load(list + side * H + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ uint32_t count(int side) const { return cnt[side]; }
};

// within(s, t, k) on g in `view` for pending edge i: 0 no, 1 yes, 2 the sets overflowed. Every
// thread of the workgroup calls it with the same arguments and gets the same answer. sh: two
// words of LDS; *rowmax: the longest row expanded so far (uniform).
template <class Sets>
__device__ int sp_search(const SpGraph& g, int view, uint32_t i, int64_t s, int64_t t, int k, Sets& S, uint32_t* sh,
                         uint32_t* rowmax) {
  const uint32_t tid = threadIdx.x, nt = blockDim.x;
  if (tid == 0) sh[0] = 0;
  if (s == t) {  // only the loop itself
    __syncthreads();
    if (tid == 0 && tri_has_pair(g.ax, g.ay, g.n0, s, s)) atomicOr(&sh[0], 1u);
    uint64_t pb, pe;
    tri_row(g.px, g.np, s, &pb, &pe);
    for (uint64_t q = pb + tid; q < pe; q += nt) {
      const uint32_t j = g.pj[q];
      if (g.py[q] == s && j < i && sp_traversable(view, j, i, sp_status(g.status, j))) atomicOr(&sh[0], 1u);
    }
    __syncthreads();
    const int r = (int)(sh[0] & 1u);
    __syncthreads();
    return r;
  }
  S.reset();
  if (tid == 0 && !(S.seed(g, 0, s) && S.seed(g, 1, t))) sh[0] = 4;  // an endpoint is no vertex
  __syncthreads();
  if (sh[0] & 4u) {
    __syncthreads();
    return 0;
  }
  uint32_t fb[2] = {0, 0}, fe[2] = {1, 1};
  for (int step = 0; step < k; ++step) {
    const int side = sp_pick_side(fe[0] - fb[0], fe[1] - fb[1]);
    if (fe[side] == fb[side]) return 0;  // the ball is complete
    for (uint32_t f = fb[side]; f < fe[side]; ++f) {
      const int64_t u = S.at(side, f);
      uint64_t b, e, pb, pe;
      tri_row(g.ax, g.n0, u, &b, &e);
      tri_row(g.px, g.np, u, &pb, &pe);
      const uint64_t la = e - b, len = la + (pe - pb);
      if (len > *rowmax) *rowmax = len > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)len;
      for (uint64_t q = tid; q < len; q += nt) {
        int64_t y;
        if (q < la) {
          y = g.ay[b + q];
        } else {
          const uint64_t p = pb + (q - la);
          const uint32_t j = g.pj[p];
          if (j >= i || !sp_traversable(view, j, i, sp_status(g.status, j))) continue;
          y = g.py[p];
        }
        const int r = S.visit(g, side, y);
        if (r == kVisMet) atomicOr(&sh[0], 1u);
        else if (r == kVisFull) atomicOr(&sh[0], 2u);
      }
    }
    __syncthreads();
    const uint32_t flag = sh[0], cnt = S.count(side);
    __syncthreads();
    if (flag & 1u) return 1;
    if (flag & 2u) return 2;
    fb[side] = fe[side];
    fe[side] = cnt;
  }
  return 0;
}

__device__ __forceinline__ void sp_note_row(unsigned long long* ctl, uint32_t rowmax) {
  if (threadIdx.x == 0 && rowmax > ctl[SP_ROWMAX]) atomicMax(ctl + SP_ROWMAX, (unsigned long long)rowmax);
}

// the LDS of an on-chip search: both key tables, both lists
struct SpLds {
  int64_t words[2 * (kSpSlotsMax + kSpannerLdsSet)];
};
static_assert(sizeof(SpLds) == 12288, "12 KiB per wave: 13 waves per CU (gs_spanner_seq.hpp)");

__device__ __forceinline__ LdsSets sp_lds_sets(SpLds* lds, uint32_t* cnt, uint32_t lds_set) {
  LdsSets S;
  S.cap = lds_set < kSpannerLdsSet ? (lds_set ? lds_set : 1u) : kSpannerLdsSet;
  S.slots = sp_set_slots(S.cap);
  S.keys = lds->words;
  S.list = lds->words + 2 * S.slots;
  S.cnt = cnt;
  return S;
}

__device__ __forceinline__ StampSets sp_stamp_sets(const SpArenas& ar, uint32_t* cnt, uint32_t q) {
  StampSets S;
  S.stamp = ar.stamp + (uint64_t)blockIdx.x * ar.H;
  S.list = ar.list + 2ull * blockIdx.x * ar.H;
  S.H = ar.H;
  S.cnt = cnt;
  S.gen = ar.gen0 + q;
  return S;
}

__device__ __forceinline__ void sp_push(uint32_t* list, unsigned long long* len, uint32_t v, uint64_t cap) {
  const unsigned long long p = atomicAdd(len, 1ull);
  if (p < cap) list[p] = v;
}

__global__ __launch_bounds__(kSpWave) void k_sp_query(SpGraph g, const int64_t* __restrict__ src,
                                                      const int64_t* __restrict__ dst, uint64_t n, uint64_t stride,
                                                      int k, uint8_t* __restrict__ out, uint32_t* __restrict__ heavy,
                                                      unsigned long long* __restrict__ ctl, uint32_t lds_set) {
  __shared__ SpLds lds;
  __shared__ uint32_t cnt[4], sh[2];
  const uint64_t i = blockIdx.x;
  if (i >= n) return;
  LdsSets S = sp_lds_sets(&lds, cnt, lds_set);
  uint32_t rowmax = 0;
  const int r = sp_search(g, kSpBase, 0, src[i * stride], dst[i * stride], k, S, sh, &rowmax);
  if (threadIdx.x == 0) {
    if (r == 2) sp_push(heavy, ctl + SP_HEAVY, (uint32_t)i, n);
    else out[i] = (uint8_t)r;
  }
  sp_note_row(ctl, rowmax);
}

__global__ __launch_bounds__(kSpBS) void k_sp_query_heavy(SpGraph g, const int64_t* __restrict__ src,
                                                          const int64_t* __restrict__ dst, uint64_t n,
                                                          uint64_t stride, int k, uint8_t* __restrict__ out,
                                                          const uint32_t* __restrict__ heavy, uint64_t nheavy,
                                                          unsigned long long* __restrict__ ctl, SpArenas ar) {
  __shared__ uint32_t cnt[4], sh[2];
  uint32_t rowmax = 0, q = 0;
  for (uint64_t it = blockIdx.x; it < nheavy; it += gridDim.x, ++q) {
    const uint64_t i = heavy[it];
    if (i >= n) continue;
    StampSets S = sp_stamp_sets(ar, cnt, q);
    const int r = sp_search(g, kSpBase, 0, src[i * stride], dst[i * stride], k, S, sh, &rowmax);
    if (threadIdx.x == 0) {
      if (r == 2) atomicAdd(ctl + SP_ERR, 1ull);
      out[i] = r == 1 ? 1 : 0;
    }
  }
  sp_note_row(ctl, rowmax);
}

// the verdict of pending edge j in a round (gs_spanner_seq.hpp: sp_round_verdict), or -1 when a
// search overflowed its sets
template <class Sets>
__device__ int sp_decide(const SpGraph& g, uint32_t j, int64_t s, int64_t t, int k, Sets& S, uint32_t* sh,
                         uint32_t* rowmax) {
  const int up = sp_search(g, kSpUpper, j, s, t, k, S, sh, rowmax);
  if (up == 2) return -1;
  if (up == 0) return sp_round_verdict(false, false);
  const int lo = sp_search(g, kSpLower, j, s, t, k, S, sh, rowmax);
  if (lo == 2) return -1;
  return sp_round_verdict(true, lo == 1);
}

__global__ __launch_bounds__(kSpWave) void k_sp_round(SpGraph g, const int64_t* __restrict__ ps,
                                                      const int64_t* __restrict__ pt,
                                                      const uint32_t* __restrict__ list, uint64_t nlist, int k,
                                                      uint8_t* __restrict__ st_out, uint32_t* __restrict__ list_out,
                                                      uint32_t* __restrict__ heavy,
                                                      unsigned long long* __restrict__ ctl, uint32_t lds_set,
                                                      uint64_t npend) {
  __shared__ SpLds lds;
  __shared__ uint32_t cnt[4], sh[2];
  if (blockIdx.x >= nlist) return;
  const uint32_t j = list[blockIdx.x];
  if (j >= npend) return;
  LdsSets S = sp_lds_sets(&lds, cnt, lds_set);
  uint32_t rowmax = 0;
  const int v = sp_decide(g, j, ps[j], pt[j], k, S, sh, &rowmax);
  if (threadIdx.x == 0) {
    if (v < 0) {
      sp_push(heavy, ctl + SP_HEAVY, j, npend);
    } else {
      st_out[j] = (uint8_t)v;
      if (v == kSpUndecided) sp_push(list_out, ctl + SP_UND, j, npend);
    }
  }
  sp_note_row(ctl, rowmax);
}

__global__ __launch_bounds__(kSpBS) void k_sp_round_heavy(SpGraph g, const int64_t* __restrict__ ps,
                                                          const int64_t* __restrict__ pt,
                                                          const uint32_t* __restrict__ heavy, uint64_t nheavy, int k,
                                                          uint8_t* __restrict__ st_out,
                                                          uint32_t* __restrict__ list_out,
                                                          unsigned long long* __restrict__ ctl, SpArenas ar,
                                                          uint64_t npend) {
  __shared__ uint32_t cnt[4], sh[2];
  uint32_t rowmax = 0, q = 0;
  for (uint64_t it = blockIdx.x; it < nheavy; it += gridDim.x, q += 2) {
    const uint32_t j = heavy[it];
    if (j >= npend) continue;
    const int64_t s = ps[j], t = pt[j];
    StampSets S = sp_stamp_sets(ar, cnt, q);
    int v = kSpAccepted;
    const int up = sp_search(g, kSpUpper, j, s, t, k, S, sh, &rowmax);
    int lo = 0;
    if (up == 1) {
      S.gen += 1;
      lo = sp_search(g, kSpLower, j, s, t, k, S, sh, &rowmax);
      v = sp_round_verdict(true, lo == 1);
    }
    if (threadIdx.x == 0) {
      if (up == 2 || lo == 2) atomicAdd(ctl + SP_ERR, 1ull);
      st_out[j] = (uint8_t)v;
      if (v == kSpUndecided) sp_push(list_out, ctl + SP_UND, j, npend);
    }
  }
  sp_note_row(ctl, rowmax);
}

__global__ __launch_bounds__(kSpBS) void k_sp_tail(SpGraph g, const int64_t* __restrict__ ps,
                                                   const int64_t* __restrict__ pt, uint64_t npend, int k,
                                                   uint8_t* status, unsigned long long* __restrict__ ctl,
                                                   SpArenas ar) {
  __shared__ uint32_t cnt[4], sh[2];
  __shared__ uint8_t und[kSpBS];
  uint32_t rowmax = 0, q = 0;
  // kSpBS statuses at a time: an undecided byte changes only when this loop reaches it
  for (uint64_t j0 = 0; j0 < npend; j0 += kSpBS) {
    const uint64_t jt = j0 + threadIdx.x;
    und[threadIdx.x] = jt < npend && status[jt] == kSpUndecided;
    __syncthreads();
    for (uint32_t o = 0; o < kSpBS; ++o) {
      if (!und[o]) continue;
      const uint64_t j = j0 + o;
      StampSets S = sp_stamp_sets(ar, cnt, q++);
      const int r = sp_search(g, kSpLower, (uint32_t)j, ps[j], pt[j], k, S, sh, &rowmax);
      if (threadIdx.x == 0) {
        if (r == 2) atomicAdd(ctl + SP_ERR, 1ull);
        __hip_atomic_store(status + j, (uint8_t)(r == 1 ? kSpDropped : kSpAccepted), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
      }
      __syncthreads();
    }
    __syncthreads();
  }
  sp_note_row(ctl, rowmax);
}

enum : int { kFlagPending = 0, kFlagAccepted = 1, kFlagEdges = 2 };

// mode kFlagPending: a = the filter's results; kFlagAccepted: a = statuses, pj; kFlagEdges: x, y
__global__ __launch_bounds__(kSpBS) void k_sp_flag(int mode, const uint8_t* __restrict__ a,
                                                   const uint32_t* __restrict__ pj, const int64_t* __restrict__ x,
                                                   const int64_t* __restrict__ y, uint64_t n,
                                                   uint8_t* __restrict__ flags, uint32_t* __restrict__ blk) {
  __shared__ uint32_t total;
  const uint64_t i0 = (uint64_t)blockIdx.x * SPANNER_TILE + threadIdx.x * kSpPer;
  uint32_t c = 0;
#pragma unroll
  for (uint32_t q = 0; q < kSpPer; ++q) {
    const uint64_t i = i0 + q;
    if (i >= n) continue;
    bool keep;
    if (mode == kFlagPending) {
      keep = a[i] == 0;
    } else if (mode == kFlagAccepted) {
      const uint32_t j = pj[i];
      keep = j != kSpDead && a[j] == kSpAccepted;
    } else {
      keep = x[i] <= y[i];
    }
    flags[i] = keep ? 1 : 0;
    c += keep ? 1u : 0u;
  }
  block_count_to<kSpBS>(c, &total, blk + blockIdx.x);
}

__global__ __launch_bounds__(kSpBS) void k_sp_pending(const int64_t* __restrict__ src, const int64_t* __restrict__ dst,
                                                      uint64_t n, uint64_t stride, const uint8_t* __restrict__ flags,
                                                      const uint32_t* __restrict__ blk, uint32_t* __restrict__ pidx,
                                                      int64_t* __restrict__ ps, int64_t* __restrict__ pt,
                                                      int64_t* __restrict__ ex, int64_t* __restrict__ ey,
                                                      uint32_t* __restrict__ list, uint64_t cap) {
  __shared__ uint32_t wsum[kSpBS / 64];
  const uint64_t i0 = (uint64_t)blockIdx.x * SPANNER_TILE + threadIdx.x * kSpPer;
  uint32_t bits = 0;
#pragma unroll
  for (uint32_t q = 0; q < kSpPer; ++q)
    if (i0 + q < n && flags[i0 + q]) bits |= 1u << q;
  uint64_t pos = (uint64_t)blk[blockIdx.x] + block_excl_scan<kSpBS>((uint32_t)__popc(bits), wsum);
#pragma unroll
  for (uint32_t q = 0; q < kSpPer; ++q) {
    if (!(bits & (1u << q))) continue;
    if (pos < cap) {
      const int64_t s = src[(i0 + q) * stride], t = dst[(i0 + q) * stride];
      pidx[pos] = (uint32_t)(i0 + q);
      ps[pos] = s;
      pt[pos] = t;
      ex[2 * pos] = s;
      ey[2 * pos] = t;
      ex[2 * pos + 1] = t;
      ey[2 * pos + 1] = s;
      list[pos] = (uint32_t)pos;
    }
    ++pos;
  }
}

__global__ __launch_bounds__(kSpBS) void k_sp_compact_pairs(const int64_t* __restrict__ x, const int64_t* __restrict__ y,
                                                            uint64_t n, const uint8_t* __restrict__ flags,
                                                            const uint32_t* __restrict__ blk, int64_t* __restrict__ ox,
                                                            int64_t* __restrict__ oy, uint64_t cap) {
  __shared__ uint32_t wsum[kSpBS / 64];
  const uint64_t i0 = (uint64_t)blockIdx.x * SPANNER_TILE + threadIdx.x * kSpPer;
  uint32_t bits = 0;
#pragma unroll
  for (uint32_t q = 0; q < kSpPer; ++q)
    if (i0 + q < n && flags[i0 + q]) bits |= 1u << q;
  uint64_t pos = (uint64_t)blk[blockIdx.x] + block_excl_scan<kSpBS>((uint32_t)__popc(bits), wsum);
#pragma unroll
  for (uint32_t q = 0; q < kSpPer; ++q) {
    if (!(bits & (1u << q))) continue;
    if (pos < cap) {
      ox[pos] = x[i0 + q];
      oy[pos] = y[i0 + q];
    }
    ++pos;
  }
}

__global__ __launch_bounds__(kSpBS) void k_sp_gather(const uint32_t* __restrict__ pay, const int64_t* __restrict__ ex,
                                                     const int64_t* __restrict__ ey, uint64_t ne,
                                                     int64_t* __restrict__ px, int64_t* __restrict__ py,
                                                     uint32_t* __restrict__ pj) {
  const uint64_t e = (uint64_t)blockIdx.x * kSpBS + threadIdx.x;
  if (e >= ne) return;
  const uint64_t r = pay ? pay[e] : e;
  if (r >= ne) return;
  const int64_t x = ex[r], y = ey[r];
  px[e] = x;
  py[e] = y;
  pj[e] = ((r & 1) && x == y) ? kSpDead : (uint32_t)(r >> 1);
}

__global__ __launch_bounds__(kSpBS) void k_sp_mark(const uint8_t* __restrict__ status,
                                                   const uint32_t* __restrict__ pidx, uint64_t npend,
                                                   uint8_t* __restrict__ accepted,
                                                   unsigned long long* __restrict__ ctl) {
  const uint64_t j = (uint64_t)blockIdx.x * kSpBS + threadIdx.x;
  const bool acc = j < npend && status[j] == kSpAccepted;
  if (acc) accepted[pidx[j]] = 1;
  const unsigned long long wave = __ballot(acc);
  if ((threadIdx.x & 63u) == 0 && wave) atomicAdd(ctl + SP_ACC, (unsigned long long)__popcll(wave));
}

__global__ __launch_bounds__(kSpBS) void k_sp_merge(const int64_t* __restrict__ ax, const int64_t* __restrict__ ay,
                                                    uint64_t n0, const int64_t* __restrict__ dx,
                                                    const int64_t* __restrict__ dy, uint64_t nd,
                                                    int64_t* __restrict__ ox, int64_t* __restrict__ oy, uint64_t cap) {
  const uint64_t i = (uint64_t)blockIdx.x * kSpBS + threadIdx.x;
  if (i >= n0 + nd) return;
  int64_t kx, ky;
  uint64_t pos;
  if (i < n0) {
    kx = ax[i];
    ky = ay[i];
    pos = i + tri_pair_lower(dx, dy, nd, kx, ky);
  } else {
    kx = dx[i - n0];
    ky = dy[i - n0];
    pos = (i - n0) + tri_pair_lower(ax, ay, n0, kx, ky);
  }
  if (pos < cap) {
    ox[pos] = kx;
    oy[pos] = ky;
  }
}

__global__ __launch_bounds__(kSpBS) void k_sp_count_rows(const int64_t* __restrict__ x, uint64_t n,
                                                         unsigned long long* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * kSpBS + threadIdx.x;
  const bool head = i < n && (i == 0 || x[i - 1] != x[i]);
  const unsigned long long wave = __ballot(head);
  if ((threadIdx.x & 63u) == 0 && wave) atomicAdd(out, (unsigned long long)__popcll(wave));
}

uint32_t grid_of(uint64_t n) { return (uint32_t)((n + kSpBS - 1) / kSpBS); }

}  // namespace

void launch_sp_query(const SpGraph& g, const int64_t* src, const int64_t* dst, uint64_t n, uint64_t stride, int k,
                     uint8_t* out, uint32_t* heavy, unsigned long long* ctl, uint32_t lds_set, hipStream_t st) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_sp_query, dim3((uint32_t)n), dim3(kSpWave), 0, st, g, src, dst, n, stride, k, out, heavy, ctl,
                     lds_set);
}

void launch_sp_query_heavy(const SpGraph& g, const int64_t* src, const int64_t* dst, uint64_t n, uint64_t stride,
                           int k, uint8_t* out, const uint32_t* heavy, uint64_t nheavy, unsigned long long* ctl,
                           const SpArenas& ar, hipStream_t st) {
  if (nheavy == 0 || ar.count == 0) return;
  const uint32_t grid = (uint32_t)(nheavy < ar.count ? nheavy : ar.count);
  hipLaunchKernelGGL(k_sp_query_heavy, dim3(grid), dim3(kSpBS), 0, st, g, src, dst, n, stride, k, out, heavy, nheavy,
                     ctl, ar);
}

void launch_sp_round(const SpGraph& g, const int64_t* ps, const int64_t* pt, const uint32_t* list, uint64_t nlist,
                     int k, uint8_t* st_out, uint32_t* list_out, uint32_t* heavy, unsigned long long* ctl,
                     uint32_t lds_set, hipStream_t st) {
  if (nlist == 0) return;
  hipLaunchKernelGGL(k_sp_round, dim3((uint32_t)nlist), dim3(kSpWave), 0, st, g, ps, pt, list, nlist, k, st_out,
                     list_out, heavy, ctl, lds_set, g.np / 2);
}

void launch_sp_round_heavy(const SpGraph& g, const int64_t* ps, const int64_t* pt, const uint32_t* heavy,
                           uint64_t nheavy, int k, uint8_t* st_out, uint32_t* list_out, unsigned long long* ctl,
                           const SpArenas& ar, hipStream_t st) {
  if (nheavy == 0 || ar.count == 0) return;
  const uint32_t grid = (uint32_t)(nheavy < ar.count ? nheavy : ar.count);
  hipLaunchKernelGGL(k_sp_round_heavy, dim3(grid), dim3(kSpBS), 0, st, g, ps, pt, heavy, nheavy, k, st_out, list_out,
                     ctl, ar, g.np / 2);
}

void launch_sp_tail(const SpGraph& g, const int64_t* ps, const int64_t* pt, uint64_t npend, int k, uint8_t* status,
                    unsigned long long* ctl, const SpArenas& ar, hipStream_t st) {
  if (npend == 0 || ar.count == 0) return;
  hipLaunchKernelGGL(k_sp_tail, dim3(1), dim3(kSpBS), 0, st, g, ps, pt, npend, k, status, ctl, ar);
}

void launch_sp_flag_pending(const uint8_t* res, uint64_t n, uint8_t* flags, uint32_t* blk, hipStream_t st) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_sp_flag, dim3((uint32_t)sp_blocks(n)), dim3(kSpBS), 0, st, (int)kFlagPending, res,
                     (const uint32_t*)nullptr, (const int64_t*)nullptr, (const int64_t*)nullptr, n, flags, blk);
}

void launch_sp_pending(const int64_t* src, const int64_t* dst, uint64_t n, uint64_t stride, const uint8_t* flags,
                       const uint32_t* blk, uint32_t* pidx, int64_t* ps, int64_t* pt, int64_t* ex, int64_t* ey,
                       uint32_t* list, uint64_t cap, hipStream_t st) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_sp_pending, dim3((uint32_t)sp_blocks(n)), dim3(kSpBS), 0, st, src, dst, n, stride, flags, blk,
                     pidx, ps, pt, ex, ey, list, cap);
}

void launch_sp_gather(const uint32_t* pay, const int64_t* ex, const int64_t* ey, uint64_t ne, int64_t* px,
                      int64_t* py, uint32_t* pj, hipStream_t st) {
  if (ne == 0) return;
  hipLaunchKernelGGL(k_sp_gather, dim3(grid_of(ne)), dim3(kSpBS), 0, st, pay, ex, ey, ne, px, py, pj);
}

void launch_sp_mark(const uint8_t* status, const uint32_t* pidx, uint64_t npend, uint8_t* accepted,
                    unsigned long long* ctl, hipStream_t st) {
  if (npend == 0) return;
  hipLaunchKernelGGL(k_sp_mark, dim3(grid_of(npend)), dim3(kSpBS), 0, st, status, pidx, npend, accepted, ctl);
}

void launch_sp_flag_accepted(const uint32_t* pj, const uint8_t* status, uint64_t ne, uint8_t* flags, uint32_t* blk,
                             hipStream_t st) {
  if (ne == 0) return;
  hipLaunchKernelGGL(k_sp_flag, dim3((uint32_t)sp_blocks(ne)), dim3(kSpBS), 0, st, (int)kFlagAccepted, status, pj,
                     (const int64_t*)nullptr, (const int64_t*)nullptr, ne, flags, blk);
}

void launch_sp_flag_edges(const int64_t* x, const int64_t* y, uint64_t n, uint8_t* flags, uint32_t* blk,
                          hipStream_t st) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_sp_flag, dim3((uint32_t)sp_blocks(n)), dim3(kSpBS), 0, st, (int)kFlagEdges,
                     (const uint8_t*)nullptr, (const uint32_t*)nullptr, x, y, n, flags, blk);
}

void launch_sp_compact_pairs(const int64_t* x, const int64_t* y, uint64_t n, const uint8_t* flags,
                             const uint32_t* blk, int64_t* ox, int64_t* oy, uint64_t cap, hipStream_t st) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_sp_compact_pairs, dim3((uint32_t)sp_blocks(n)), dim3(kSpBS), 0, st, x, y, n, flags, blk, ox, oy,
                     cap);
}

void launch_sp_merge(const int64_t* ax, const int64_t* ay, uint64_t n0, const int64_t* dx, const int64_t* dy,
                     uint64_t nd, int64_t* ox, int64_t* oy, uint64_t cap, hipStream_t st) {
  if (n0 + nd == 0) return;
  hipLaunchKernelGGL(k_sp_merge, dim3(grid_of(n0 + nd)), dim3(kSpBS), 0, st, ax, ay, n0, dx, dy, nd, ox, oy, cap);
}

void launch_sp_count_rows(const int64_t* x, uint64_t n, unsigned long long* out, hipStream_t st) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_sp_count_rows, dim3(grid_of(n)), dim3(kSpBS), 0, st, x, n, out);
}

}  // namespace gs
