// gs_trisample_k.hip -- kernels of the sampling triangle estimate (gfx950). The per-lane bodies
// are the functions of gs_trisample_seq.hpp, which the host restatement ts_fold_parts calls too;
// here is what a lane is, what a workgroup stages, and how the lists are appended and compacted.
//
//   k_ts_coin      lane = instance, workgroup = 256 instances x one chunk of arrivals: the 64
//                  lanes of a wave share t. One jump (uniform: the affine map is the same for
//                  every instance), two LCG steps per arrival, the integer rejection on the high
//                  26 bits, the double product for survivors only. Successes are rare after the
//                  first arrivals; a wave holds its successes in LDS and appends them with one
//                  atomic per kTsCoinHold - 64 of them.
//   k_ts_search    lane = instance, workgroup = 256 instances x one tile of arrivals, staged in
//                  LDS: every lane reads the same address (a broadcast). A lane leaves its loop
//                  body early unless the arrival touches its third vertex.
//   k_ts_rows      one workgroup walks the changed arrivals in steps of 1024 with a carried
//                  row count (the shape of k_tile_scan).
#include "gs_scan.hpp"
#include "gs_trisample.hpp"

namespace gs {
namespace {

__global__ __launch_bounds__(kTsBS) void k_ts_init(uint64_t* __restrict__ lcg, TsState* __restrict__ st, uint32_t S,
                                                   int64_t seed) {
  const uint32_t i = blockIdx.x * kTsBS + threadIdx.x;
  if (i >= S) return;
  lcg[i] = ts_instance_state(seed, i);
  st[i] = ts_state_init();
}

__global__ __launch_bounds__(kTsBS) void k_ts_coin(const uint64_t* __restrict__ lcg_in, uint64_t* __restrict__ lcg_out,
                                                   uint32_t S, uint32_t gx, uint32_t t0, uint32_t n, uint32_t chunk,
                                                   int64_t* __restrict__ keys, uint64_t cap,
                                                   unsigned long long* __restrict__ ctl) {
  // a wave's successes wait here for one append: at the first arrivals of a stream every wave
  // has some at every arrival, and one global atomic each would queue on a single address
  __shared__ uint64_t held[kTsBS / 64][kTsCoinHold];
  const uint32_t c = blockIdx.x / gx, inst = (blockIdx.x % gx) * kTsBS + threadIdx.x;
  const uint32_t c0 = c * chunk, len = min(chunk, n - c0), lane = threadIdx.x & 63u;
  const bool valid = inst < S;
  uint64_t* const mine = held[threadIdx.x >> 6];
  uint32_t cnt = 0;  // (wave-uniform)
  const auto flush = [&]() {
    if (!cnt) return;
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(&ctl[TS_COINS], (unsigned long long)cnt);
    const uint32_t blo = (uint32_t)__shfl((int)(uint32_t)base, 0, 64);
    const uint32_t bhi = (uint32_t)__shfl((int)(uint32_t)(base >> 32), 0, 64);
    const uint64_t at = ((uint64_t)bhi << 32) | blo;
    __builtin_amdgcn_wave_barrier();
    for (uint32_t k = lane; k < cnt; k += 64)
      if (at + k < cap) keys[at + k] = (int64_t)(mine[k] | (1ull << 63));
    __builtin_amdgcn_wave_barrier();
    cnt = 0;
  };
  const TsAffine to_chunk = ts_jump(2ull * c0);  // (uniform)
  const uint64_t s = valid ? ts_apply(to_chunk, lcg_in[inst]) : 0;
  const uint64_t after = ts_coin_lane(s, t0 + c0 + 1, len, [&](uint32_t k, bool ok) {
    ok = ok && valid;
    const unsigned long long m = __ballot(ok);
    if (!m) return;  // wave-uniform
    if (ok) mine[cnt + (uint32_t)__popcll(m & ((1ull << lane) - 1))] = ts_key(inst, c0 + k);
    cnt += (uint32_t)__popcll(m);
    if (cnt > kTsCoinHold - 64) flush();
  });
  flush();
  if (valid && c0 + len == n) lcg_out[inst] = after;
}

__global__ __launch_bounds__(kTsBS) void k_ts_carried(const TsState* __restrict__ st, TsSeg* __restrict__ seg, uint32_t S,
                                                      uint32_t n) {
  const uint32_t i = blockIdx.x * kTsBS + threadIdx.x;
  if (i < S) seg[i] = ts_seg_carried(st[i], n);
}

__global__ __launch_bounds__(kTsBS) void k_ts_segments(const unsigned long long* __restrict__ keys, uint64_t K, uint32_t S,
                                                       uint32_t n, const int64_t* __restrict__ src,
                                                       const int64_t* __restrict__ dst, uint64_t stride, uint32_t t0,
                                                       uint64_t third_seed, int64_t vertices, TsSeg* __restrict__ seg,
                                                       unsigned long long* __restrict__ ctl) {
  const uint64_t j = (uint64_t)blockIdx.x * kTsBS + threadIdx.x;
  uint32_t attempts = 0;
  if (j < K) {
    const uint64_t* k64 = reinterpret_cast<const uint64_t*>(keys);
    const uint32_t inst = ts_key_instance(k64[j]), pos = ts_key_position(k64[j]);
    if (inst < S && pos < n) {
      seg[S + j] = ts_seg_sampled(k64, K, j, n, src[(uint64_t)pos * stride], dst[(uint64_t)pos * stride], t0,
                                  third_seed, vertices, &attempts);
      if (ts_key_first_of_instance(k64, j)) seg[inst].end = pos;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) attempts = max(attempts, (uint32_t)__shfl_xor((int)attempts, o, 64));
  if ((threadIdx.x & 63u) == 0 && attempts) atomicMax(&ctl[TS_ATTEMPTS], (unsigned long long)attempts);
}

__global__ __launch_bounds__(kTsBS) void k_ts_search(TsSeg* __restrict__ seg, const unsigned long long* __restrict__ keys,
                                                     uint64_t K, uint32_t S, uint32_t gx,
                                                     const int64_t* __restrict__ src, const int64_t* __restrict__ dst,
                                                     uint64_t stride, uint32_t n, uint32_t tile) {
  __shared__ TsEdge e[kTsTile];
  const uint32_t lo = (blockIdx.x / gx) * tile, hi = min(n, lo + tile);
  const uint32_t inst = (blockIdx.x % gx) * kTsBS + threadIdx.x;
  for (uint32_t k = threadIdx.x; k < hi - lo; k += kTsBS) {
    e[k].a = src[(uint64_t)(lo + k) * stride];
    e[k].b = dst[(uint64_t)(lo + k) * stride];
  }
  __syncthreads();
  if (inst < S)
    ts_search_lane(seg, reinterpret_cast<const uint64_t*>(keys), K, S, inst, lo, hi,
                   [&](uint32_t pos) { return e[pos - lo]; });
}

__global__ __launch_bounds__(kTsBS) void k_ts_finish(const TsSeg* __restrict__ seg,
                                                     const unsigned long long* __restrict__ keys, uint64_t K, uint32_t S,
                                                     uint32_t n, int32_t* __restrict__ delta, TsState* __restrict__ st) {
  const uint64_t g = (uint64_t)blockIdx.x * kTsBS + threadIdx.x;
  if (g >= S + K) return;
  const TsSeg sg = seg[g];
  const TsOutcome o = ts_outcome(sg, n);
  if (o.plus != kTsNever && o.plus < n) atomicAdd(&delta[o.plus], 1);
  if (o.minus != kTsNever && o.minus < n) atomicAdd(&delta[o.minus], -1);
  if (sg.end == n) {
    const uint32_t inst = g < S ? (uint32_t)g : ts_key_instance(keys[g - S]);
    if (inst < S) st[inst] = ts_state_of(sg, o.flags);
  }
}

// thread q of a tile owns the kTsRowPer consecutive arrivals at tile + q * kTsRowPer
__device__ __forceinline__ void load_deltas(const int32_t* __restrict__ delta, uint32_t n, int32_t (&d)[kTsRowPer],
                                            uint32_t& sum, uint32_t& cnt) {
  const uint32_t p0 = blockIdx.x * kTsRowTile + threadIdx.x * kTsRowPer;
  sum = cnt = 0;
#pragma unroll
  for (uint32_t q = 0; q < kTsRowPer; ++q) {
    d[q] = p0 + q < n ? delta[p0 + q] : 0;
    sum += (uint32_t)d[q];
    cnt += d[q] != 0;
  }
}

__global__ __launch_bounds__(kTsBS) void k_ts_delta_tiles(const int32_t* __restrict__ delta, uint32_t n,
                                                          uint32_t* __restrict__ tsum, uint32_t* __restrict__ tcnt) {
  __shared__ uint32_t tot[2];
  int32_t d[kTsRowPer];
  uint32_t sum, cnt;
  load_deltas(delta, n, d, sum, cnt);
  block_count_to<kTsBS>(sum, &tot[0], &tsum[blockIdx.x]);
  block_count_to<kTsBS>(cnt, &tot[1], &tcnt[blockIdx.x]);
}

__global__ __launch_bounds__(kTsBS) void k_ts_changes(const int32_t* __restrict__ delta, uint32_t n,
                                                      const uint32_t* __restrict__ tsum, const uint32_t* __restrict__ tcnt,
                                                      int32_t beta0, uint32_t t0, double inv_s, int32_t vertices,
                                                      int32_t* __restrict__ chg_t, int32_t* __restrict__ chg_beta,
                                                      int32_t* __restrict__ chg_est) {
  __shared__ uint32_t ws[2][kTsBS / 64];
  int32_t d[kTsRowPer];
  uint32_t sum, cnt;
  load_deltas(delta, n, d, sum, cnt);
  uint32_t run = (uint32_t)beta0 + tsum[blockIdx.x] + block_excl_scan<kTsBS>(sum, ws[0]);
  uint32_t r = tcnt[blockIdx.x] + block_excl_scan<kTsBS>(cnt, ws[1]);
  const uint32_t p0 = blockIdx.x * kTsRowTile + threadIdx.x * kTsRowPer;
#pragma unroll
  for (uint32_t q = 0; q < kTsRowPer; ++q) {
    run += (uint32_t)d[q];
    if (d[q] != 0 && r < n) {
      const int32_t t = (int32_t)(t0 + p0 + q + 1);
      chg_t[r] = t;
      chg_beta[r] = (int32_t)run;
      chg_est[r] = ts_estimate(inv_s, (int32_t)run, t, vertices);
      ++r;
    }
  }
}

__global__ __launch_bounds__(kTsRowsBS) void k_ts_rows(const int32_t* __restrict__ chg_t,
                                                       const int32_t* __restrict__ chg_beta,
                                                       const int32_t* __restrict__ chg_est, int32_t beta0, int32_t est0,
                                                       int32_t* __restrict__ row_t, int32_t* __restrict__ row_est,
                                                       int32_t* __restrict__ row_beta, uint64_t cap,
                                                       unsigned long long* __restrict__ ctl) {
  __shared__ uint32_t ws[kTsRowsBS / 64];
  const uint64_t M = ctl[TS_CHANGES];
  uint32_t carry = 0;
  for (uint64_t c0 = 0; c0 < M; c0 += kTsRowsBS) {  // block-uniform
    const uint64_t k = c0 + threadIdx.x;
    const bool row = k < M && chg_est[k] != (k ? chg_est[k - 1] : est0);
    const uint32_t before = block_excl_scan<kTsRowsBS>(row ? 1u : 0u, ws);
    uint32_t total = 0;
#pragma unroll
    for (uint32_t q = 0; q < kTsRowsBS / 64; ++q) total += ws[q];
    const uint64_t at = (uint64_t)carry + before;
    if (row && at < cap) {
      row_t[at] = chg_t[k];
      row_est[at] = chg_est[k];
      row_beta[at] = chg_beta[k];
    }
    carry += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    ctl[TS_ROWS] = carry;
    ctl[TS_BETA] = (unsigned long long)(uint32_t)(M ? chg_beta[M - 1] : beta0);
    ctl[TS_EST] = (unsigned long long)(uint32_t)(M ? chg_est[M - 1] : est0);
  }
}

__global__ __launch_bounds__(kTsBS) void k_ts_states(const TsState* __restrict__ st, uint32_t S, int64_t* __restrict__ src,
                                                     int64_t* __restrict__ trg, int64_t* __restrict__ third,
                                                     uint8_t* __restrict__ flags, int32_t* __restrict__ sampled_at) {
  const uint32_t i = blockIdx.x * kTsBS + threadIdx.x;
  if (i >= S) return;
  const TsState s = st[i];
  if (src) src[i] = s.src;
  if (trg) trg[i] = s.trg;
  if (third) third[i] = s.third;
  if (flags) flags[i] = (uint8_t)s.flags;
  if (sampled_at) sampled_at[i] = s.sampled_at;
}

inline uint32_t blocks_of(uint64_t n) { return (uint32_t)((n + kTsBS - 1) / kTsBS); }

}  // namespace

void launch_ts_init(uint64_t* lcg, TsState* st, uint32_t S, int64_t seed, hipStream_t st_) {
  hipLaunchKernelGGL(k_ts_init, dim3(blocks_of(S)), dim3(kTsBS), 0, st_, lcg, st, S, seed);
}

void launch_ts_coin(const uint64_t* lcg_in, uint64_t* lcg_out, uint32_t S, uint32_t t0, uint32_t n, uint32_t chunk,
                    int64_t* keys, uint64_t cap, unsigned long long* ctl, hipStream_t st) {
  const uint32_t gx = blocks_of(S);
  hipLaunchKernelGGL(k_ts_coin, dim3((uint32_t)(gx * ts_parts(n, chunk))), dim3(kTsBS), 0, st, lcg_in, lcg_out, S, gx, t0,
                     n, chunk, keys, cap, ctl);
}

void launch_ts_carried(const TsState* st, TsSeg* seg, uint32_t S, uint32_t n, hipStream_t st_) {
  hipLaunchKernelGGL(k_ts_carried, dim3(blocks_of(S)), dim3(kTsBS), 0, st_, st, seg, S, n);
}

void launch_ts_segments(const unsigned long long* keys, uint64_t K, uint32_t S, uint32_t n, const int64_t* src,
                        const int64_t* dst, uint64_t stride, uint32_t t0, uint64_t third_seed, int64_t vertices,
                        TsSeg* seg, unsigned long long* ctl, hipStream_t st) {
  hipLaunchKernelGGL(k_ts_segments, dim3(blocks_of(K)), dim3(kTsBS), 0, st, keys, K, S, n, src, dst, stride, t0,
                     third_seed, vertices, seg, ctl);
}

void launch_ts_search(TsSeg* seg, const unsigned long long* keys, uint64_t K, uint32_t S, const int64_t* src,
                      const int64_t* dst, uint64_t stride, uint32_t n, uint32_t tile, hipStream_t st) {
  const uint32_t gx = blocks_of(S);
  if (tile > kTsTile) tile = kTsTile;  // (the LDS stage holds kTsTile arrivals)
  hipLaunchKernelGGL(k_ts_search, dim3((uint32_t)(gx * ts_parts(n, tile))), dim3(kTsBS), 0, st, seg, keys, K, S, gx, src,
                     dst, stride, n, tile);
}

void launch_ts_finish(const TsSeg* seg, const unsigned long long* keys, uint64_t K, uint32_t S, uint32_t n,
                      int32_t* delta, TsState* st, hipStream_t st_) {
  hipLaunchKernelGGL(k_ts_finish, dim3(blocks_of(S + K)), dim3(kTsBS), 0, st_, seg, keys, K, S, n, delta, st);
}

void launch_ts_delta_tiles(const int32_t* delta, uint32_t n, uint32_t* tsum, uint32_t* tcnt, hipStream_t st) {
  hipLaunchKernelGGL(k_ts_delta_tiles, dim3((uint32_t)ts_row_tiles(n)), dim3(kTsBS), 0, st, delta, n, tsum, tcnt);
}

void launch_ts_changes(const int32_t* delta, uint32_t n, const uint32_t* tsum, const uint32_t* tcnt, int32_t beta0,
                       uint32_t t0, double inv_s, int32_t vertices, int32_t* chg_t, int32_t* chg_beta,
                       int32_t* chg_est, hipStream_t st) {
  hipLaunchKernelGGL(k_ts_changes, dim3((uint32_t)ts_row_tiles(n)), dim3(kTsBS), 0, st, delta, n, tsum, tcnt, beta0, t0,
                     inv_s, vertices, chg_t, chg_beta, chg_est);
}

void launch_ts_rows(const int32_t* chg_t, const int32_t* chg_beta, const int32_t* chg_est, int32_t beta0, int32_t est0,
                    int32_t* row_t, int32_t* row_est, int32_t* row_beta, uint64_t cap, unsigned long long* ctl,
                    hipStream_t st) {
  hipLaunchKernelGGL(k_ts_rows, dim3(1), dim3(kTsRowsBS), 0, st, chg_t, chg_beta, chg_est, beta0, est0, row_t, row_est,
                     row_beta, cap, ctl);
}

void launch_ts_states(const TsState* st, uint32_t S, int64_t* src, int64_t* trg, int64_t* third, uint8_t* flags,
                      int32_t* sampled_at, hipStream_t st_) {
  hipLaunchKernelGGL(k_ts_states, dim3(blocks_of(S)), dim3(kTsBS), 0, st_, st, S, src, trg, third, flags, sampled_at);
}

}  // namespace gs
