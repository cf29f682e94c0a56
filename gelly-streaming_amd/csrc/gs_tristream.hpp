// gs_tristream.hpp -- host-side launchers of the triangle streams' kernels (gs_tristream_k.hip):
// every record of example/ExactTriangleCount.java's continuous stream, exact in arrival order.
// Every launch is queued on the given stream; kernel boundaries carry all ordering between
// workgroups (no workgroup waits on another inside a launch).
//
// State. The adjacency of section 6c -- directed entries (x, y) sorted by
// (x, y), two buffers, merged and never re-sorted -- with a 32-bit `first` stamp per entry (the
// number of the arrival that added the pair) in place of the fold number; the distinct streams'
// vertex table (gs_vtable.hpp) and beside its vertex list an int64 counter t per rank. Per fold:
// canonical pairs, the new pairs and their reverses, per arrival its rows in the merged
// adjacency, c, the row (closed, total) and the record offset; per record its arrival, vertex,
// delta, rank key and count. The rules are gs_tristream_seq.hpp's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gs_distinct.hpp"
#include "gs_triangle.hpp"

#define GS_TRISTREAM_SEQ_RULES_ONLY  // not the host restatements (trs_fold_seq, trs_fold_parts)
#include "gs_tristream_seq.hpp"

namespace gs {

// Positions per workgroup of the scan and compaction kernels (gsamd.TRISTREAM_TILE).
constexpr uint32_t TRISTREAM_TILE = 2048;
constexpr uint32_t kTrsBS = 256;                        // threads of every workgroup
constexpr uint32_t kTrsPer = TRISTREAM_TILE / kTrsBS;   // consecutive positions per thread
static_assert(TRISTREAM_TILE == kTrsBS * kTrsPer, "tile = threads x positions per thread");
constexpr uint32_t kTrsWaveArrivals = 64;               // arrivals a wave of the walk kernels owns, one per lane
// Lanes that share one arrival's walked row while it is short (gsamd.TRISTREAM_LANES), and the
// longest walked row that counts as short (gsamd.TRISTREAM_SHORT_ROW): longer ones take a wave.
constexpr uint32_t TRISTREAM_LANES = 8;
constexpr uint32_t kTrsShortRow = 4 * TRISTREAM_LANES;

// control words (uint64) of a handle
enum TrsCtl : int {
  TRS_ERR = 0,      // an index was out of range, or the write pass met another count than the count pass
  TRS_NEW = 1,      // new pairs of the fold
  TRS_HEADS = 2,    // row heads of the merged adjacency: the vertices of G after the fold
  TRS_CLOSED = 3,   // } sum of c over the fold, and its records:
  TRS_RECORDS = 4,  // } adjacent words, written together
  TRS_CROSSED = 5,  // tiles of the record scan that began inside a segment
  TRS_STEPS = 6,    // sum over the fold's arrivals of the walked row's length
  TRS_HOT = 7,      // the longest row an arrival of the fold met
  TRS_LIVE = 8,     // rows of a state export
  TRS_CTL_WORDS = 16
};
static_assert(TRS_RECORDS == TRS_CLOSED + 1, "k_trs_carry stores the two sums side by side");

struct TrsAdj {
  const int64_t* x = nullptr;
  const int64_t* y = nullptr;
  const uint32_t* first = nullptr;
  uint64_t n = 0;
};
struct TrsAdjOut {
  int64_t* x = nullptr;
  int64_t* y = nullptr;
  uint32_t* first = nullptr;
  uint64_t cap = 0;
};
// per arrival: the walked (shorter) row [sb, se) and the searched row [lb, le) of its endpoints in
// the merged adjacency; all zero for a loop and, under `ignore`, for a repeat
struct TrsRowInfo {
  uint32_t sb, se, lb, le;
};

// After launch_tri_flag_new over the arrivals sorted stably by (lo, hi) and launch_tile_scan: the
// flagged positions in order are the new pairs (nx, ny) with nfirst = the number of their arrival,
// at most cap of them; is_new[arrival] = its position was flagged.
void launch_trs_compact_new(const uint32_t* pay, const int64_t* lo, const int64_t* hi, uint64_t n, const uint8_t* flags,
                            const uint32_t* blk, uint64_t t0, int64_t* nx, int64_t* ny, uint32_t* nfirst,
                            uint8_t* is_new, uint64_t cap, hipStream_t st);
// (rx, ry, rfirst)[j] = (ny, nx, nfirst)[pay[j]] for j < m (pay: the new pairs ordered by (hi, lo))
void launch_trs_reverse(const uint32_t* pay, const int64_t* nx, const int64_t* ny, const uint32_t* nfirst, uint64_t m,
                        int64_t* rx, int64_t* ry, uint32_t* rfirst, hipStream_t st);
// O = merge of A, the forward and the reverse entries, m each, all sorted by (x, y) and disjoint,
// every entry with its stamp
void launch_trs_merge(const TrsAdj& A, const int64_t* nx, const int64_t* ny, const uint32_t* nfirst, const int64_t* rx,
                      const int64_t* ry, const uint32_t* rfirst, uint64_t m, const TrsAdjOut& O, hipStream_t st);
// blk[b] = entries of tile b that head their row (x differs from the entry before) ...
void launch_trs_head_count(const int64_t* x, uint64_t n, uint32_t* blk, hipStream_t st);
// ... and, blk after launch_tile_scan, their x in order, at most cap
void launch_trs_head_write(const int64_t* x, uint64_t n, const uint32_t* blk, int64_t* out, uint64_t cap, hipStream_t st);
// info[a] of every arrival (is_new null: repeats are intersected); TRS_STEPS and TRS_HOT
void launch_trs_rows(const TrsAdj& A, const int64_t* lo, const int64_t* hi, const uint8_t* is_new, uint64_t n,
                     TrsRowInfo* info, unsigned long long* ctl, hipStream_t st);
// cnt[a] = c of arrival a: the entries of its walked row found in its searched row, both stamps
// below the arrival's number t0 + 1 + a
void launch_trs_count(const TrsAdj& A, const TrsRowInfo* info, uint64_t n, uint64_t t0, uint32_t* cnt,
                      unsigned long long* ctl, hipStream_t st);
// The scan over the arrivals in three launches. Before the host's check of the record count:
// every tile reduced, the aggregates scanned, ctl[TRS_CLOSED] = sum of c, ctl[TRS_RECORDS] = records.
void launch_trs_arr_reduce(const uint32_t* cnt, uint64_t n, TrsSeg* agg, TrsSeg* carry, unsigned long long* ctl,
                           hipStream_t st);
// After it: closed[a] = c, total[a] = total0 + the inclusive sum of c, roff[a] = the records before a
void launch_trs_arr_apply(const uint32_t* cnt, uint64_t n, const TrsSeg* carry, int64_t total0, uint32_t* closed,
                          int64_t* total, uint32_t* roff, hipStream_t st);
// The ordered write: per arrival with c > 0 its records at roff[a]: every hit w of the walked row
// in the row's (ascending) order with delta 1, then lo[a] and hi[a] with delta c; at most cap rows.
void launch_trs_write(const TrsAdj& A, const TrsRowInfo* info, const int64_t* lo, const int64_t* hi, const uint32_t* cnt,
                      const uint32_t* roff, uint64_t n, uint64_t t0, uint32_t* r_arr, int64_t* r_v, uint32_t* r_delta,
                      uint64_t cap, unsigned long long* ctl, hipStream_t st);
// The seeded segmented sum over n records sorted stably by rank (skey[j] = rank ^ sign bit, spay[j]
// = the record's arrival-order row): count[spay[j]] = counter[rank] + the deltas of its segment up
// to and including j. Four launches: tiles reduced; aggregates scanned; every position applied
// (counter is only read); the segment tails stored as the new counters.
void launch_trs_seg_pass(const unsigned long long* skey, const uint32_t* spay, const uint32_t* delta, uint64_t n,
                         int64_t* counter, uint64_t rank_cap, TrsSeg* agg, TrsSeg* carry, int64_t* count,
                         unsigned long long* ctl, hipStream_t st);
// The export: blk[b] = rows k of tile b with counter[rank[k]] > 0, then (v[k], counter) of those rows
void launch_trs_live_count(const int64_t* rank, uint64_t n, const int64_t* counter, uint64_t rank_cap, uint32_t* blk,
                           hipStream_t st);
void launch_trs_live_write(const int64_t* v, const int64_t* rank, uint64_t n, const int64_t* counter, uint64_t rank_cap,
                           const uint32_t* blk, int64_t* ov, int64_t* oc, uint64_t cap, hipStream_t st);

}  // namespace gs
