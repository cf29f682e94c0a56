// gs_degstream.hpp -- host-side launchers of the degree streams' kernels (gs_degstream_k.hip):
// every running degree and every distribution record of an edge stream, exact in arrival order
// (SimpleEdgeStream.getDegrees, example/DegreeDistribution.java). Every launch is queued on the
// given stream; kernel boundaries carry all ordering between workgroups (no workgroup waits on
// another inside a launch).
//
// State. Ids get a dense rank from the distinct streams' vertex table
// (gs_distinct.hpp: DistVTable, launch_dist_vertices; vid[rank] beside it); beside the vertex
// list uint32 degree[rank], and a dense uint32 count[degree]. Per fold: key, sign and vertex of
// every occurrence, its (old, new) row, the records compacted in arrival order and their counts.
// The rules are gs_degstream_seq.hpp's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gs_distinct.hpp"

#define GS_DEGSTREAM_SEQ_RULES_ONLY  // not the host restatements (ds_fold_seq, ds_fold_parts)
#include "gs_degstream_seq.hpp"

namespace gs {

// Positions per workgroup of the scan and compaction kernels (gsamd.DEGSTREAM_TILE).
constexpr uint32_t DEGSTREAM_TILE = 2048;
constexpr uint32_t kDsBS = 256;                        // threads of every workgroup
constexpr uint32_t kDsPer = DEGSTREAM_TILE / kDsBS;    // consecutive positions per thread
static_assert(DEGSTREAM_TILE == kDsBS * kDsPer, "tile = threads x positions per thread");
constexpr uint32_t kDsNoLate = 0xFFFFFFFFu;            // a tile without a deferred tail
constexpr uint64_t kDsMinCounts = 1024;                // the count array's first capacity (gsamd.DEGSTREAM_MIN_COUNTS)

// control words (uint64) of a handle
enum DsCtl : int {
  DS_ERR = 0,      // a slot, rank, degree or row index was out of range
  DS_MAX = 1,      // the largest new degree of the fold
  DS_CROSSED = 2,  // tiles of the fold's two scans that began inside a segment
  DS_RECORDS = 3,  // records of the fold
  DS_LIVE = 4,     // rows of a state export
  DS_CTL_WORDS = 8
};

// After launch_dist_vertices over the fold's collected endpoints (entry e of edge e >> 1; IN and
// OUT pass the one collected array twice): per occurrence o its rank as key[o], its sign as
// sgn[o] and its id as vertex[o]. A slot or rank out of range raises DS_ERR.
void launch_ds_keys(const int64_t* src, const int64_t* dst, const uint8_t* del, uint64_t n, uint64_t stride, int dir,
                    const DistVTable& vt, const uint32_t* vslot, uint64_t rank_cap, int64_t* key, int8_t* sgn,
                    int64_t* vertex, unsigned long long* ctl, hipStream_t st);

// The seeded segmented scan of maps x -> max(x + a, b) over n positions sorted stably by key
// (skey[j] = key ^ sign bit, spay[j] = the arrival position; the key's low 32 bits index state).
// Position j's map is (sgn[spay[j]], clamp ? 0 : -inf); its segment's seed is state[key].
// Four launches: every tile reduced to one DsSeg; the tile aggregates scanned by one workgroup;
// every position's value before and after it written at its arrival position (before may be
// null), state[key] written at the tails of segments that lie inside one tile and the one tail
// per tile whose segment began in an earlier tile -- other workgroups of the launch read its
// seed -- deferred to (late_idx, late_val); the deferred tails committed. agg and carry hold
// ds_tiles(n) DsSeg each, late_idx / late_val as many words. max_word (may be null): an atomic
// maximum of the values after.
void launch_ds_seg_pass(const unsigned long long* skey, const uint32_t* spay, const int8_t* sgn, uint64_t n, bool clamp,
                        uint32_t* state, uint64_t state_cap, DsSeg* agg, DsSeg* carry, uint32_t* late_idx,
                        uint32_t* late_val, uint32_t* before, uint32_t* after, unsigned long long* ctl,
                        unsigned long long* max_word, hipStream_t st);

// Records, flag-scan-compact over 0, 1 or 2 rows per occurrence in arrival order: blk[b] = rows
// of tile b ...
void launch_ds_rec_count(const uint32_t* old_d, const uint32_t* new_d, const int8_t* sgn, uint64_t occs, uint32_t* blk,
                         hipStream_t st);
// ... and, blk after launch_tile_scan, the rows: occurrence, degree (as the sort's key and as
// 32 bits) and delta, at most cap of them
void launch_ds_rec_write(const uint32_t* old_d, const uint32_t* new_d, const int8_t* sgn, uint64_t occs,
                         const uint32_t* blk, uint32_t* occ, int64_t* key, uint32_t* degree, int8_t* delta,
                         uint64_t cap, unsigned long long* ctl, hipStream_t st);

// The live entries of a state array in index order, flag-scan-compact: blk[b] = entries > 0 of
// tile b; then (ids ? ids[i] : i, state[i]) per live entry, at most cap rows.
void launch_ds_live_count(const uint32_t* state, uint64_t n, uint32_t* blk, hipStream_t st);
void launch_ds_live_write(const uint32_t* state, uint64_t n, const uint32_t* blk, const int64_t* ids, int64_t* id_out,
                          int64_t* value_out, uint64_t cap, hipStream_t st);

}  // namespace gs
