// gs_trisample.cpp -- the sampling triangle estimate behind include/gs_summary.h's gs_trisample_*
// section: example/BroadcastTriangleCount.java at parallelism 1 with the seeded coin of
// example/IncidenceSamplingTriangleCount.java. The rules and the decomposition are in
// gs_trisample_seq.hpp (executable: ts_fold_seq, ts_fold_parts), the kernels in
// gs_trisample_k.hip, the argument in DESIGN.md section 6h.
//
// A fold of n arrivals: the coin pass appends the resample keys (the host reads their count: the
// fold's first wait; a list too small for them is grown and the pass, which only reads the
// stored LCG states, runs again); the shared radix sort orders them; segments, search and
// outcomes follow; the deltas of betaSum are scanned, the changed arrivals compacted, the rows
// written; the host reads the control words (the fold's last wait).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "gs_internal.hpp"
#include "gs_trisample.hpp"

using namespace gsi;

struct gs_trisample_s : StreamOwner {
  uint32_t S = 0;
  int32_t vertices = 0;
  int64_t seed = 0;
  uint64_t third_seed = 0;
  DevBuf<unsigned long long> ctl;  // gs::TsCtl words
  DevBuf<uint64_t> lcg[2];         // [S] the Random states: a fold reads lcg[cur] and writes the other
  int cur = 0;
  DevBuf<gs::TsState> st;          // [S]
  // fold scratch for n_cap arrivals
  uint64_t n_cap = 0;
  DevBuf<int32_t> delta, chg_t, chg_beta, chg_est, row_t, row_est, row_beta;
  DevBuf<uint32_t> tsum, tcnt;     // [row tiles + 1]
  // the resample keys and the segments, for k_cap keys
  uint64_t k_cap = 0;
  DevBuf<int64_t> keys;
  DevBuf<gs::TsSeg> seg;           // [S + k_cap]
  SortScratch sort;
  // device staging of a host fold, of the host form of the states
  FoldStage stage;                 // (src, dst)
  uint64_t o_cap = 0;
  DevBuf<int64_t> o_src, o_trg, o_third;
  DevBuf<uint8_t> o_flags;
  DevBuf<int32_t> o_at;
  // host-known totals
  uint64_t folded = 0;
  int32_t beta_sum = 0, last_est = 0;
  uint64_t rows = 0;
  bool rows_kept = true;  // false after a fold the library cut into pieces
  // gs_testing_trisample_tune (< 0: product) and gs_testing_trisample_stats
  int64_t tune[5] = {-1, -1, -1, -1, -1};
  uint64_t stats[4] = {0, 0, 0, 0};
  uint64_t phase_us[4] = {0, 0, 0, 0};  // of the last profiled fold: coin, sort and segments, search, outcomes and rows
};

namespace {

constexpr const char* kWhat = "trisample";  // check_handle: "null trisample handle"

// the arrivals of one device piece of a fold (gs_testing_trisample_tune, what = 4)
uint64_t piece_of(const gs_trisample_s* h) {
  return h->tune[4] > 0 ? (uint64_t)std::min<int64_t>(h->tune[4], (int64_t)gs::kTsMaxFold) : gs::kTsMaxFold;
}

int ensure_scratch(gs_trisample_s* h, uint64_t n) {
  GS_HIP(grow_group(h->stream, h->n_cap, n, std::min(piece_of(h), n + n / 4), [&](uint64_t c) {
    hipError_t e = alloc_each(c, h->delta, h->chg_t, h->chg_beta, h->chg_est, h->row_t, h->row_est, h->row_beta);
    if (e == hipSuccess) e = alloc_each(gs::ts_row_tiles(c) + 1, h->tsum, h->tcnt);
    return e;
  }));
  return GS_OK;
}

int ensure_keys(gs_trisample_s* h, uint64_t keys) {
  GS_HIP(grow_group(h->stream, h->k_cap, keys, keys + keys / 4, [&](uint64_t c) {
    const hipError_t e = h->keys.alloc(c);
    return e != hipSuccess ? e : h->seg.alloc((uint64_t)h->S + c);
  }));
  return GS_OK;
}

// the keys a fold at edge counts t0 + 1 .. t0 + n is expected to append, S (H(t0 + n) - H(t0)),
// with eight deviations of headroom
uint64_t expected_keys(uint32_t S, uint64_t t0, uint64_t n) {
  const double mean = (double)S * ((t0 ? 0.0 : 1.0) + std::log((double)(t0 + n) / (double)std::max<uint64_t>(t0, 1)));
  const double cap = mean + 8.0 * std::sqrt(mean) + 64.0;
  return (uint64_t)std::min(cap, (double)S * (double)n);
}

int fold_guard(gs_trisample_s* h, const void* src, const void* dst, size_t n) {
  if (n && (!src || !dst)) return fail(GS_ERR_INVALID, "null edge arrays");
  if (n > gs::kTsMaxArrivals || h->folded + n > gs::kTsMaxArrivals)
    return fail(GS_ERR_INVALID, "trisample fold: more than 2^31 - 1 arrivals in total");
  return GS_OK;
}

// 0 < n <= piece_of(h) device arrivals on h->stream
int fold_piece(gs_trisample_s* h, const int64_t* src, const int64_t* dst, uint64_t n, uint64_t stride) {
  hipStream_t st = h->stream;
  const uint32_t S = h->S, t0 = (uint32_t)h->folded, n32 = (uint32_t)n;
  const uint32_t chunk = h->tune[0] > 0 ? (uint32_t)std::min<int64_t>(h->tune[0], 1 << 30) : gs::kTsChunk;
  const uint32_t tile = h->tune[1] > 0 ? (uint32_t)std::min<int64_t>(h->tune[1], gs::kTsTile) : gs::kTsTile;
  if (int rc = ensure_scratch(h, n)) return rc;
  const uint64_t expect = expected_keys(S, t0, n);
  if (int rc = ensure_keys(h, h->tune[3] > 0 ? std::min<uint64_t>(expect, (uint64_t)h->tune[3]) : expect)) return rc;
  uint64_t us[4] = {0, 0, 0, 0};
  PhaseTimer timer(st, h->tune[2] > 0, us, 4);
  timer.mark(0);
  // coin
  uint64_t K = 0;
  for (int attempt = 0;; ++attempt) {
    GS_HIP(hipMemsetAsync(h->ctl, 0, gs::TS_CTL_WORDS * 8, st));
    GS_LAUNCH(gs::launch_ts_coin(h->lcg[h->cur], h->lcg[h->cur ^ 1], S, t0, n32, chunk, h->keys, h->k_cap, h->ctl, st));
    unsigned long long k = 0;
    GS_HIP(hipMemcpyAsync(&k, h->ctl + gs::TS_COINS, 8, hipMemcpyDeviceToHost, st));
    GS_HIP(hipStreamSynchronize(st));
    K = k;
    if (K <= h->k_cap) break;
    if (K > (1ull << 31) || attempt) return fail(GS_ERR_CAPACITY, "trisample fold: too many resamples for one fold");
    if (int rc = ensure_keys(h, K)) return rc;
  }
  timer.mark(1);
  // segments
  GS_LAUNCH(gs::launch_ts_carried(h->st, h->seg, S, n32, st));
  GS_HIP(hipMemsetAsync(h->delta, 0, n * 4, st));
  const unsigned long long* sorted = nullptr;
  if (K) {
    if (int rc = sort_scratch_ensure(h->sort, K, st)) return rc;
    // the sort's key is id ^ 2^63 = instance << 32 | position: the digits above n's and S's bits are zero in all
    bool skip[gs::kSortPasses];
    for (int p = 0; p < 4; ++p) skip[p] = p > 0 && ((uint64_t)(n - 1) >> (8 * p)) == 0;
    for (int p = 4; p < (int)gs::kSortPasses; ++p) skip[p] = ((uint64_t)(S - 1) >> (8 * (p - 4))) == 0;
    gs::SortSrc cur;
    if (int rc = sort_by_key(h->sort, h->keys, K, skip, &cur, st, "trisample fold")) return rc;
    sorted = cur.key;
    GS_LAUNCH(gs::launch_ts_segments(sorted, K, S, n32, src, dst, stride, t0, h->third_seed, h->vertices, h->seg, h->ctl,
                                     st));
  }
  timer.mark(2);
  // search, outcomes
  GS_LAUNCH(gs::launch_ts_search(h->seg, sorted, K, S, src, dst, stride, n32, tile, st));
  timer.mark(3);
  GS_LAUNCH(gs::launch_ts_finish(h->seg, sorted, K, S, n32, h->delta, h->st, st));
  // rows
  const uint64_t nt = gs::ts_row_tiles(n);
  GS_LAUNCH(gs::launch_ts_delta_tiles(h->delta, n32, h->tsum, h->tcnt, st));
  GS_LAUNCH(gs::launch_tile_scan(h->tsum, nt, h->ctl + gs::TS_DSUM, st));
  GS_LAUNCH(gs::launch_tile_scan(h->tcnt, nt, h->ctl + gs::TS_CHANGES, st));
  GS_LAUNCH(gs::launch_ts_changes(h->delta, n32, h->tsum, h->tcnt, h->beta_sum, t0, 1.0 / (double)S, h->vertices,
                                  h->chg_t, h->chg_beta, h->chg_est, st));
  GS_LAUNCH(gs::launch_ts_rows(h->chg_t, h->chg_beta, h->chg_est, h->beta_sum, h->last_est, h->row_t, h->row_est,
                               h->row_beta, h->n_cap, h->ctl, st));
  unsigned long long c[gs::TS_CTL_WORDS];
  GS_HIP(hipMemcpyAsync(c, h->ctl, sizeof(c), hipMemcpyDeviceToHost, st));
  GS_HIP(hipStreamSynchronize(st));
  timer.mark(4);
  timer.finish();
  for (int i = 0; i < 4; ++i) h->phase_us[i] += us[i];
  if (c[gs::TS_COINS] != K || c[gs::TS_CHANGES] > n || c[gs::TS_ROWS] > c[gs::TS_CHANGES] ||
      (uint32_t)c[gs::TS_BETA] > S)
    return fail(GS_ERR_HIP, "trisample fold: counts out of range (the handle's state is undefined)");
  h->cur ^= 1;
  h->folded += n;
  h->beta_sum = (int32_t)(uint32_t)c[gs::TS_BETA];
  h->last_est = (int32_t)(uint32_t)c[gs::TS_EST];
  h->rows = c[gs::TS_ROWS];
  h->stats[0] = K;
  h->stats[1] = (uint64_t)S + K;
  h->stats[2] = c[gs::TS_ATTEMPTS];
  h->stats[3] = c[gs::TS_ROWS];
  return GS_OK;
}

void forget_last(gs_trisample_s* h) {
  std::fill(h->stats, h->stats + 4, 0);
  std::fill(h->phase_us, h->phase_us + 4, 0);
  h->rows = 0;
  h->rows_kept = true;
}

// the whole fold, cut into pieces of at most piece_of(h) arrivals; host: the arrays are HOST arrays
int fold_all(gs_trisample_s* h, const int64_t* src, const int64_t* dst, size_t n, uint64_t stride, bool host,
             size_t* rows) {
  forget_last(h);
  if (rows) *rows = 0;
  if (n == 0) return GS_OK;
  DeviceGuard g(h->device);
  uint64_t sum[4] = {0, 0, 0, 0};
  const uint64_t piece = piece_of(h);
  for (uint64_t at = 0; at < n; at += piece) {
    const uint64_t len = std::min<uint64_t>(piece, n - at);
    const int64_t* col[2] = {src + at * stride, dst + at * stride};
    if (host) GS_HIP(h->stage.put(h->stream, len, piece, col));  // (fold_piece ends with a wait)
    if (int rc = fold_piece(h, col[0], col[1], len, host ? 1 : stride)) return rc;
    sum[0] += h->stats[0];
    sum[1] += h->stats[1];
    sum[2] = std::max(sum[2], h->stats[2]);
    sum[3] += h->stats[3];
  }
  if (n > piece) {
    std::copy(sum, sum + 4, h->stats);
    h->rows = 0;
    h->rows_kept = false;
  }
  if (rows) *rows = sum[3];
  return GS_OK;
}

int rows_impl(gs_trisample_s* h, int32_t* edges, int32_t* estimate, int32_t* beta_sum, size_t cap, size_t* n,
              bool to_host) {
  if (int rc = check_handle(h, kWhat)) return rc;
  if (!n) return fail(GS_ERR_INVALID, "n is null");
  DeviceGuard g(h->device);
  if (!h->rows_kept) return fail(GS_ERR_INVALID, "trisample rows: the last fold was cut into pieces, its rows were not kept");
  const uint64_t rows = h->rows;
  *n = rows;
  if (cap < rows) return truncated(cap, rows);
  if (rows == 0) return GS_OK;
  const ColumnCopy copy(h->stream, to_host);
  GS_HIP(copy.col(edges, h->row_t.get(), rows));
  GS_HIP(copy.col(estimate, h->row_est.get(), rows));
  GS_HIP(copy.col(beta_sum, h->row_beta.get(), rows));
  GS_HIP(copy.done());
  return GS_OK;
}

int states_impl(gs_trisample_s* h, int64_t* src, int64_t* trg, int64_t* third, uint8_t* flags, int32_t* sampled_at,
                bool to_host) {
  if (int rc = check_handle(h, kWhat)) return rc;
  DeviceGuard g(h->device);
  const uint32_t S = h->S;
  if (!to_host) {
    GS_LAUNCH(gs::launch_ts_states(h->st, S, src, trg, third, flags, sampled_at, h->stream));
    return GS_OK;
  }
  GS_HIP(grow_group(h->stream, h->o_cap, S, S, [&](uint64_t c) {
    return alloc_each(c, h->o_src, h->o_trg, h->o_third, h->o_flags, h->o_at);
  }));
  GS_LAUNCH(gs::launch_ts_states(h->st, S, h->o_src, h->o_trg, h->o_third, h->o_flags, h->o_at, h->stream));
  const ColumnCopy copy(h->stream, true);
  GS_HIP(copy.col(src, h->o_src.get(), S));
  GS_HIP(copy.col(trg, h->o_trg.get(), S));
  GS_HIP(copy.col(third, h->o_third.get(), S));
  GS_HIP(copy.col(flags, h->o_flags.get(), S));
  GS_HIP(copy.col(sampled_at, h->o_at.get(), S));
  GS_HIP(copy.done());
  return GS_OK;
}

int init_state(gs_trisample_s* h) {
  GS_LAUNCH(gs::launch_ts_init(h->lcg[h->cur], h->st, h->S, h->seed, h->stream));
  GS_HIP(hipMemsetAsync(h->ctl, 0, gs::TS_CTL_WORDS * 8, h->stream));
  h->folded = 0;
  h->beta_sum = h->last_est = 0;
  forget_last(h);
  return GS_OK;
}

}  // namespace

extern "C" {

int gs_trisample_destroy(gs_trisample t) { return owner_destroy(t); }

int gs_trisample_create(gs_trisample* out, int device, uint64_t samples, int64_t vertices, int64_t seed,
                        uint64_t third_seed) {
  if (!out) return fail(GS_ERR_INVALID, "out is null");
  *out = nullptr;
  if (samples < 1 || samples > gs::kTsMaxSamples) return fail(GS_ERR_INVALID, "trisample create: samples must be in 1 .. 2^20");
  if (vertices < gs::kTsMinVertices || vertices > gs::kTsMaxVertices)
    return fail(GS_ERR_INVALID, "trisample create: vertices must be in 3 .. 2^31 - 1");
  if (int rc = check_device_index(device)) return rc;
  return owner_create(out, device, [&](gs_trisample_s* h) -> int {
    h->S = (uint32_t)samples;
    h->vertices = (int32_t)vertices;
    h->seed = seed;
    h->third_seed = third_seed;
    GS_HIP(h->ctl.alloc(gs::TS_CTL_WORDS));
    GS_HIP(alloc_each(samples, h->lcg[0], h->lcg[1], h->st));
    return init_state(h);
  });
}

int gs_trisample_reset(gs_trisample t) {
  if (int rc = check_handle(t, kWhat)) return rc;
  DeviceGuard g(t->device);
  return init_state(t);
}

int gs_trisample_fold_device(gs_trisample t, const int64_t* src, const int64_t* dst, size_t n, size_t stride,
                             size_t* rows) {
  if (int rc = check_handle(t, kWhat)) return rc;
  if (stride == 0 || stride > 0xFFFFFFFFull) return fail(GS_ERR_INVALID, "stride must be >= 1");
  if (int rc = fold_guard(t, src, dst, n)) return rc;
  return fold_all(t, src, dst, n, stride, false, rows);
}

int gs_trisample_fold(gs_trisample t, const int64_t* src, const int64_t* dst, size_t n, size_t* rows) {
  if (int rc = check_handle(t, kWhat)) return rc;
  if (int rc = fold_guard(t, src, dst, n)) return rc;
  return fold_all(t, src, dst, n, 1, true, rows);
}

int gs_trisample_rows_device(gs_trisample t, int32_t* edges, int32_t* estimate, int32_t* beta_sum, size_t cap,
                             size_t* n) {
  return rows_impl(t, edges, estimate, beta_sum, cap, n, false);
}

int gs_trisample_rows(gs_trisample t, int32_t* edges, int32_t* estimate, int32_t* beta_sum, size_t cap, size_t* n) {
  return rows_impl(t, edges, estimate, beta_sum, cap, n, true);
}

int gs_trisample_estimate(gs_trisample t, uint64_t* arrivals, int32_t* beta_sum, int32_t* estimate) {
  if (int rc = check_handle(t, kWhat)) return rc;
  if (!arrivals || !beta_sum || !estimate) return fail(GS_ERR_INVALID, "null estimate pointers");
  *arrivals = t->folded;
  *beta_sum = t->beta_sum;
  *estimate = t->last_est;
  return GS_OK;
}

int gs_trisample_states_device(gs_trisample t, int64_t* src, int64_t* trg, int64_t* third, uint8_t* flags,
                               int32_t* sampled_at) {
  return states_impl(t, src, trg, third, flags, sampled_at, false);
}

int gs_trisample_states(gs_trisample t, int64_t* src, int64_t* trg, int64_t* third, uint8_t* flags,
                        int32_t* sampled_at) {
  return states_impl(t, src, trg, third, flags, sampled_at, true);
}

int gs_trisample_sync(gs_trisample t) { return owner_sync(t, kWhat); }
int gs_trisample_get_stream(gs_trisample t, void** stream) { return owner_get_stream(t, kWhat, stream); }
int gs_trisample_wait_stream(gs_trisample t, void* stream) { return owner_wait_stream(t, kWhat, stream); }

// gs_testing.h: the last fold. No device call.
int gs_testing_trisample_stats(void* handle, uint64_t* out) {
  gs_trisample t = static_cast<gs_trisample>(handle);
  if (int rc = check_handle(t, kWhat)) return rc;
  if (!out) return fail(GS_ERR_INVALID, "out is null");
  for (int i = 0; i < 4; ++i) out[i] = t->stats[i];
  for (int i = 0; i < 4; ++i) out[4 + i] = t->phase_us[i];
  return GS_OK;
}

int gs_testing_trisample_tune(void* handle, int what, int64_t value) {
  gs_trisample t = static_cast<gs_trisample>(handle);
  // (the arguments first: they are checked without a handle, and so without a device)
  if (what < 0 || what > 5) return fail(GS_ERR_INVALID, "trisample tune: unknown control");
  if (what == 5 && (value < 0 || value > (int64_t)gs::kTsMaxArrivals))
    return fail(GS_ERR_INVALID, "trisample tune: edge_count must be in 0 .. 2^31 - 1");
  if (int rc = check_handle(t, kWhat)) return rc;
  if (what == 5) {  // an action: the arrival count alone
    t->folded = (uint64_t)value;
    return GS_OK;
  }
  t->tune[what] = value <= 0 ? -1 : value;
  return GS_OK;
}

}  // extern "C"
