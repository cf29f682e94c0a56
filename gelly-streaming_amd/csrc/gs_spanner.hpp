// gs_spanner.hpp -- host-side launchers of the k-spanner summary's kernels (gs_spanner_k.hip):
// the bounded two-sided search in its three uses (within queries and the filter pass, the rounds
// over the pending edges, the serial tail), the flag / compact passes around them and the merge
// of the accepted edges into the sorted adjacency. Every launch is queued on the given stream;
// kernel boundaries carry all ordering between workgroups (no workgroup waits on another inside
// a launch, no load has to be fresh).
//
// State. The adjacency A holds every edge {u, v} of G as the two directed
// entries (u, v) and (v, u), a loop {u, u} as the one entry (u, u): two parallel arrays x, y (the
// 64-bit ids themselves) sorted by (x, y) in signed order, as the triangle summary keeps them
// (gs_triangle_rows.hpp has the row arithmetic). The dense number of a vertex, where one is
// needed (the stamp arrays of the heavy search), is the index of the first entry of its row:
// below A.n for a vertex of G0, A.n + the index of its first pending entry for a vertex that only
// the fold's pending edges touch. No table is kept beside the rows.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define GS_SPANNER_SEQ_RULES_ONLY  // not the host restatement (SpannerSeq)
#include "gs_spanner_seq.hpp"

namespace gs {

constexpr uint32_t SPANNER_TILE = 1024;  // elements per workgroup of the flag / compact passes
constexpr uint32_t kSpBS = 256;          // threads of those workgroups and of a heavy search
constexpr uint32_t kSpPer = SPANNER_TILE / kSpBS;
static_assert(SPANNER_TILE == kSpBS * kSpPer, "tile = threads x elements per thread");
constexpr uint32_t kSpWave = 64;         // threads of an on-chip search: one wave per edge
constexpr uint32_t kSpannerArenas = 32;  // product size of the heavy search's arena pool
constexpr uint32_t kSpannerRoundCap = 16;

// control words (uint64) of a handle
enum SpCtl : int {
  SP_HEAVY = 0,   // edges on the heavy list of the current launch   } read together
  SP_UND = 1,     // edges the current round left undecided           }
  SP_PEND = 2,    // pending edges of the current fold (the filter pass's survivors)
  SP_ENT = 3,     // adjacency entries of the fold's accepted edges   } read together
  SP_ACC = 4,     // accepted edges of the fold                       }
  SP_VERT = 5,    // vertices of G
  SP_ROWMAX = 6,  // diagnostics: the longest row a search of the last fold expanded
  SP_ROWS = 7,    // edges of the current export
  SP_ERR = 8,     // a heavy search ran out of its arena (cannot happen with a sized arena)
  SP_CTL_WORDS = 16
};

// what a search walks: G0 = (ax, ay)[n0] and the pending entries (px, py, pj)[np] sorted by
// (px, py), with the status byte of pending edge pj (gs_spanner_seq.hpp: sp_traversable)
struct SpGraph {
  const int64_t* ax = nullptr;
  const int64_t* ay = nullptr;
  uint64_t n0 = 0;
  const int64_t* px = nullptr;
  const int64_t* py = nullptr;
  const uint32_t* pj = nullptr;
  uint64_t np = 0;
  const uint8_t* status = nullptr;
};

// The heavy search's pool: arena b has the stamps stamp[b * H .. ) of H dense vertex numbers and
// the two discovery lists list[(2 b + side) * H .. ). A search of generation g stamps with
// sp_stamp(g, side); the q-th search of an arena in a launch has generation gen0 + q.
struct SpArenas {
  uint32_t* stamp = nullptr;
  int64_t* list = nullptr;
  uint64_t H = 0;
  uint32_t count = 0;
  uint32_t gen0 = 0;
};

__host__ __device__ constexpr uint64_t sp_blocks(uint64_t n) { return (n + SPANNER_TILE - 1) / SPANNER_TILE; }

// out[i] = within(src[i * stride], dst[i * stride], k) on g (view kSpBase) for i < n, one wave
// each with on-chip sets of lds_set entries per side; a search that overflows them appends i to
// heavy (ctl[SP_HEAVY] counts) and leaves out[i] unwritten.
void launch_sp_query(const SpGraph& g, const int64_t* src, const int64_t* dst, uint64_t n, uint64_t stride, int k,
                     uint8_t* out, uint32_t* heavy, unsigned long long* ctl, uint32_t lds_set, hipStream_t st);
// the same for the nheavy elements of the heavy list, one workgroup per arena
void launch_sp_query_heavy(const SpGraph& g, const int64_t* src, const int64_t* dst, uint64_t n, uint64_t stride,
                           int k, uint8_t* out, const uint32_t* heavy, uint64_t nheavy, unsigned long long* ctl,
                           const SpArenas& ar, hipStream_t st);
// One round: for the nlist undecided pending edges j = list[q] (endpoints ps[j], pt[j]) the upper
// and, when needed, the lower search on g, whose status bytes are the round before's;
// st_out[j] = the verdict, the still undecided appended to list_out (ctl[SP_UND]), overflows to
// heavy (ctl[SP_HEAVY]).
void launch_sp_round(const SpGraph& g, const int64_t* ps, const int64_t* pt, const uint32_t* list, uint64_t nlist,
                     int k, uint8_t* st_out, uint32_t* list_out, uint32_t* heavy, unsigned long long* ctl,
                     uint32_t lds_set, hipStream_t st);
// (two generations per element)
void launch_sp_round_heavy(const SpGraph& g, const int64_t* ps, const int64_t* pt, const uint32_t* heavy,
                           uint64_t nheavy, int k, uint8_t* st_out, uint32_t* list_out, unsigned long long* ctl,
                           const SpArenas& ar, hipStream_t st);
// The serial tail, one workgroup on arena 0: the undecided pending edges in arrival order, each
// searched on G0 + the accepted edges before it; `status` (g.status, written in place) ends
// without an undecided byte. One generation per undecided edge.
void launch_sp_tail(const SpGraph& g, const int64_t* ps, const int64_t* pt, uint64_t npend, int k, uint8_t* status,
                    unsigned long long* ctl, const SpArenas& ar, hipStream_t st);

// flags[i] = res[i] == 0 for i < n; blk[b] = flagged elements of tile b
void launch_sp_flag_pending(const uint8_t* res, uint64_t n, uint8_t* flags, uint32_t* blk, hipStream_t st);
// The flagged arrivals in order become the pending edges j = 0 ..: pidx[j] = arrival index,
// (ps, pt)[j] its endpoints, entries 2j = (s, t) and 2j + 1 = (t, s) in (ex, ey), list[j] = j.
// blk after launch_tile_scan; at most cap pending edges.
void launch_sp_pending(const int64_t* src, const int64_t* dst, uint64_t n, uint64_t stride, const uint8_t* flags,
                       const uint32_t* blk, uint32_t* pidx, int64_t* ps, int64_t* pt, int64_t* ex, int64_t* ey,
                       uint32_t* list, uint64_t cap, hipStream_t st);
// the ne entries in sorted order: px[e] = ex[pay[e]], py[e] = ey[pay[e]], pj[e] = pay[e] / 2, or
// kSpDead for the second entry of a loop
void launch_sp_gather(const uint32_t* pay, const int64_t* ex, const int64_t* ey, uint64_t ne, int64_t* px,
                      int64_t* py, uint32_t* pj, hipStream_t st);
// accepted[pidx[j]] = status[j] == accepted for j < npend; ctl[SP_ACC] += the accepted
void launch_sp_mark(const uint8_t* status, const uint32_t* pidx, uint64_t npend, uint8_t* accepted,
                    unsigned long long* ctl, hipStream_t st);
// flags[e] = entry e belongs to an accepted edge (and is not dead), e < ne
void launch_sp_flag_accepted(const uint32_t* pj, const uint8_t* status, uint64_t ne, uint8_t* flags, uint32_t* blk,
                             hipStream_t st);
// flags[i] = x[i] <= y[i]: each undirected edge once (the export)
void launch_sp_flag_edges(const int64_t* x, const int64_t* y, uint64_t n, uint8_t* flags, uint32_t* blk,
                          hipStream_t st);
// the flagged pairs (x, y)[i] in order into (ox, oy), at most cap of them
void launch_sp_compact_pairs(const int64_t* x, const int64_t* y, uint64_t n, const uint8_t* flags,
                             const uint32_t* blk, int64_t* ox, int64_t* oy, uint64_t cap, hipStream_t st);
// (ox, oy) = merge of A = (ax, ay)[n0] and D = (dx, dy)[nd], both sorted by (x, y), disjoint
void launch_sp_merge(const int64_t* ax, const int64_t* ay, uint64_t n0, const int64_t* dx, const int64_t* dy,
                     uint64_t nd, int64_t* ox, int64_t* oy, uint64_t cap, hipStream_t st);
// *out += rows of the sorted column x[n] (the vertices of G)
void launch_sp_count_rows(const int64_t* x, uint64_t n, unsigned long long* out, hipStream_t st);

}  // namespace gs
