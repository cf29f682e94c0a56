// gs_matching.hpp -- host-side launchers of the weighted matching summary's kernels
// (gs_matching_k.hip): the rank gather behind the distinct streams' vertex phase, the phases of
// a round over the pending arrivals, the one-workgroup tail, the event compaction, and the
// export and mate probes. Every launch is queued on the given stream; kernel boundaries carry all
// ordering between workgroups (no workgroup waits on another inside a launch).
//
// State. Ids get a dense rank from the distinct streams' vertex table
// (gs_distinct.hpp: DistVTable, launch_dist_vertices; vid[rank] beside it); a rank survives a
// table rebuild, so the state is one MtVertex record per rank (gs_matching_seq.hpp): partner
// rank, source bit, value, acceptance stamp and the two batch-local words T and Rd. Per fold:
// the ranks and value of every arrival, a mark byte, the accepted byte, the record of what an
// accepted arrival removed, and two pending lists that the rounds ping-pong between.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gs_distinct.hpp"

#define GS_MATCHING_SEQ_RULES_ONLY  // not the host restatements (MatchingSeq, MatchingRounds)
#include "gs_matching_seq.hpp"

namespace gs {

constexpr uint32_t MATCHING_TILE = 1024;  // arrivals per workgroup of the event compaction
constexpr uint32_t kMtBS = 256;           // threads of every workgroup but the tail's
constexpr uint32_t kMtPer = MATCHING_TILE / kMtBS;
static_assert(MATCHING_TILE == kMtBS * kMtPer, "tile = threads x arrivals per thread");
constexpr uint32_t kMtTailBS = 1024;      // threads of the tail's one workgroup

// control words (uint64) of a handle
enum MtCtl : int {
  MT_NEXT = 0,         // arrivals the current round left pending   } read together, once per round
  MT_ERR = 1,          // a rank or list index was out of range      }
  MT_UNSAFE = 2,       // a value outside [0, 2^61) was folded since the last reset
  MT_ITERS = 3,        // fixpoint passes run by the current fold
  MT_FALLBACKS = 4,    // rounds of the current fold that fell back to plain reservations
  MT_TAIL_ROUNDS = 5,  // rounds the tail ran
  MT_ROWS = 6,         // event rows of the current fold
  MT_ACC = 7,          // accepted arrivals of the current fold
  MT_EDGES = 8,        // |M| after - before the current fold (wrapping)
  MT_WEIGHT = 9,       // weight(M) after - before (wrapping)
  MT_EXPORT = 10,      // append position of the export
  MT_CHG = 16,         // MT_CHG + k: fixpoint pass k of the current round marked an arrival (k = 0: set)
  MT_CTL_WORDS = MT_CHG + kMatchingMaxIterCap + 1
};
constexpr int kMtFoldWords = 10;  // MT_NEXT .. MT_WEIGHT: read at the end of a fold

__host__ __device__ constexpr uint64_t mt_tiles(uint64_t n) { return (n + MATCHING_TILE - 1) / MATCHING_TILE; }

// st[i] = the initial record for from <= i < to
void launch_mt_init(MtVertex* st, uint64_t from, uint64_t to, hipStream_t st_);
// After launch_dist_vertices: ru / rv[i] = the ranks of arrival i's endpoints (through vslot),
// w[i] = val[i * stride], list[i] = i, accepted[i] = 0; a rank >= st_cap raises MT_ERR, a value
// that is not weight-safe MT_UNSAFE.
void launch_mt_gather(const uint32_t* vslot, const DistVTable& vt, uint64_t st_cap, const int64_t* val,
                      uint64_t stride, uint64_t n, uint32_t* ru, uint32_t* rv, int64_t* w, uint32_t* list,
                      uint8_t* accepted, unsigned long long* ctl, hipStream_t st);
// One round over the np pending arrivals list[0 .. np): reset, seed, iter_cap gated fixpoint
// passes (pass k runs only if pass k - 1 marked something), the gated lowering to plain
// reservations, remain, commit; the still pending go to list_out in any order (ctl[MT_NEXT]).
// sharpen: sharpening is on (it applies while ctl[MT_UNSAFE] is zero).
void launch_mt_round(const MtFold& F, const uint32_t* list, uint64_t np, uint32_t* list_out, uint32_t iter_cap,
                     int sharpen, unsigned long long* ctl, hipStream_t st);
// The tail, one workgroup: all remaining rounds with the same phase functions and block barriers;
// la holds the np pending arrivals, lb is the other list.
void launch_mt_tail(const MtFold& F, uint32_t* la, uint32_t* lb, uint64_t np, uint32_t iter_cap, int sharpen,
                    unsigned long long* ctl, hipStream_t st);
// Events, flag-scan-compact over rows per arrival: blk[b] = rows of tile b, and ctl[MT_ACC],
// ctl[MT_EDGES], ctl[MT_WEIGHT] += the fold's accepted arrivals and its change of M ...
void launch_mt_event_count(const uint8_t* accepted, const MtRec* rec, const int64_t* w, uint64_t n, uint32_t* blk,
                           unsigned long long* ctl, hipStream_t st);
// ... and, blk after launch_tile_scan, the rows in arrival order (REMOVE at the source endpoint,
// REMOVE at the target endpoint, ADD), at most cap of them
void launch_mt_event_write(const uint8_t* accepted, const MtRec* rec, const uint32_t* ru, const uint32_t* rv,
                           const int64_t* w, uint64_t n, const uint32_t* blk, const int64_t* vid, uint64_t nv,
                           uint32_t* arrival, uint8_t* type, int64_t* src, int64_t* dst, int64_t* val, uint64_t cap,
                           hipStream_t st);
// the source vertices of M's edges appended to (stamp[], rank[]) in any order, at most cap rows
void launch_mt_export(const MtVertex* st, uint64_t nv, int64_t* stamp, uint32_t* rank, uint64_t cap,
                      unsigned long long* ctl, hipStream_t st_);
// rows sorted by stamp: skey[i] = stamp ^ sign bit, pay[i] = its row in rank[]; outputs may be null
void launch_mt_decode(const unsigned long long* skey, const uint32_t* pay, const uint32_t* rank, uint64_t ne,
                      const MtVertex* st, const int64_t* vid, uint64_t nv, int64_t* src, int64_t* dst, int64_t* val,
                      unsigned long long* first, hipStream_t st_);
// rank[i] (launch_dist_rank: -1 absent) -> mate[i], val[i], found[i]; absent or unmatched: 0, 0, 0
void launch_mt_mate(const int64_t* rank, uint64_t n, const MtVertex* st, const int64_t* vid, uint64_t nv,
                    int64_t* mate, int64_t* val, uint8_t* found, hipStream_t st_);

}  // namespace gs
