// gs_trisample.hpp -- host-side launchers of the sampling triangle estimate's kernels
// (gs_trisample_k.hip): the coin pass over (instance, chunk of arrivals), the segments behind the
// sorted resample keys, the search pass over (instance, tile of arrivals), the outcomes, and the
// rows by a scan of betaSum's changes. Every launch is queued on the given stream; kernel
// boundaries carry all ordering between workgroups (no workgroup waits on another inside a launch).
//
// State: per instance its java.util.Random state (48 bits in a uint64) and
// its candidate record TsState (gs_trisample_seq.hpp). Per fold: the resample keys
// (instance << 32 | position), one TsSeg per instance and per key, one int32 delta of betaSum per
// arrival, the changed arrivals, the rows.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define GS_TRISAMPLE_SEQ_RULES_ONLY  // not the host restatements (TsSeq, ts_fold_seq, ts_fold_parts)
#include "gs_trisample_seq.hpp"

namespace gs {

constexpr uint32_t kTsBS = 256;         // threads of every workgroup but the rows' one
constexpr uint32_t kTsCoinHold = 256;   // successes a wave of the coin pass holds in LDS between two appends
constexpr uint32_t kTsRowTile = 1024;   // arrivals per workgroup of the delta kernels
constexpr uint32_t kTsRowPer = kTsRowTile / kTsBS;
static_assert(kTsRowTile == kTsBS * kTsRowPer, "tile = threads x arrivals per thread");
constexpr uint32_t kTsRowsBS = 1024;    // threads of the rows' one workgroup

// control words (uint64) of a handle
enum TsCtl : int {
  TS_COINS = 0,     // coin successes of the current fold (the append position of the keys)
  TS_ATTEMPTS = 1,  // the longest third-vertex draw of the current fold, in attempts
  TS_DSUM = 2,      // betaSum after - before the current fold (32 bits, wrapping)
  TS_CHANGES = 3,   // arrivals of the current fold at which betaSum changed
  TS_ROWS = 4,      // rows of the current fold
  TS_BETA = 5,      // betaSum after the fold
  TS_EST = 6,       // the estimate at the last change (or the one carried in)
  TS_CTL_WORDS = 8
};

__host__ __device__ constexpr uint64_t ts_row_tiles(uint64_t n) { return (n + kTsRowTile - 1) / kTsRowTile; }
__host__ __device__ constexpr uint64_t ts_parts(uint64_t n, uint32_t part) { return (n + part - 1) / part; }

// lcg[i] = the Random state instance i starts from, st[i] = the initial candidate, i < S
void launch_ts_init(uint64_t* lcg, TsState* st, uint32_t S, int64_t seed, hipStream_t st_);
// The coin pass: n arrivals at edge counts t0 + 1 .. t0 + n in chunks of `chunk`; a success of
// instance i at position p appends (i << 32 | p) with bit 63 set -- as an int64 id of the sort
// driver, whose key is id ^ 2^63, so that the sorted keys are the plain ones -- at
// ctl[TS_COINS]++ while that is below cap (the count goes on). lcg_out[i] = the state after the
// fold (lcg_in is only read).
void launch_ts_coin(const uint64_t* lcg_in, uint64_t* lcg_out, uint32_t S, uint32_t t0, uint32_t n, uint32_t chunk,
                    int64_t* keys, uint64_t cap, unsigned long long* ctl, hipStream_t st);
// seg[i] = instance i's carried-in segment over the whole fold, i < S
void launch_ts_carried(const TsState* st, TsSeg* seg, uint32_t S, uint32_t n, hipStream_t st_);
// keys sorted: seg[S + j] = the segment of key j, its third vertex drawn; the carried-in segment
// of the key's instance ends at the instance's first key; ctl[TS_ATTEMPTS] = max attempts
void launch_ts_segments(const unsigned long long* keys, uint64_t K, uint32_t S, uint32_t n, const int64_t* src,
                        const int64_t* dst, uint64_t stride, uint32_t t0, uint64_t third_seed, int64_t vertices,
                        TsSeg* seg, unsigned long long* ctl, hipStream_t st);
// The search pass in tiles of `tile` <= kTsTile arrivals, staged in LDS once per workgroup.
void launch_ts_search(TsSeg* seg, const unsigned long long* keys, uint64_t K, uint32_t S, const int64_t* src,
                      const int64_t* dst, uint64_t stride, uint32_t n, uint32_t tile, hipStream_t st);
// Outcomes of the S + K segments: delta[p] (zero before) += 1 / -= 1, st[i] = the state behind
// instance i's last segment.
void launch_ts_finish(const TsSeg* seg, const unsigned long long* keys, uint64_t K, uint32_t S, uint32_t n,
                      int32_t* delta, TsState* st, hipStream_t st_);
// Rows, step 1: tsum[b] = the sum of tile b's deltas, tcnt[b] = its nonzero deltas ...
void launch_ts_delta_tiles(const int32_t* delta, uint32_t n, uint32_t* tsum, uint32_t* tcnt, hipStream_t st);
// ... step 2, both after launch_tile_scan: the changed arrivals in order, (edge count, betaSum,
// estimate) each ...
void launch_ts_changes(const int32_t* delta, uint32_t n, const uint32_t* tsum, const uint32_t* tcnt, int32_t beta0,
                       uint32_t t0, double inv_s, int32_t vertices, int32_t* chg_t, int32_t* chg_beta,
                       int32_t* chg_est, hipStream_t st);
// ... step 3, one workgroup: change k is a row iff its estimate differs from change k - 1's
// (est0 for k = 0); at most cap rows; ctl[TS_ROWS], ctl[TS_BETA], ctl[TS_EST].
void launch_ts_rows(const int32_t* chg_t, const int32_t* chg_beta, const int32_t* chg_est, int32_t beta0, int32_t est0,
                    int32_t* row_t, int32_t* row_est, int32_t* row_beta, uint64_t cap, unsigned long long* ctl,
                    hipStream_t st);
// the candidates as columns (any may be null)
void launch_ts_states(const TsState* st, uint32_t S, int64_t* src, int64_t* trg, int64_t* third, uint8_t* flags,
                      int32_t* sampled_at, hipStream_t st_);

}  // namespace gs
