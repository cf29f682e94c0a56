// gs_triangle.hpp -- host-side launchers of the triangle summary's kernels (gs_triangle_k.hip):
// canonise, the flag / scan / compact passes of the dedup and of the exports, the three-way
// merge into the sorted adjacency, the per-edge row pass and the intersection (count) kernels.
// Every launch is queued on the given stream; kernel boundaries carry all ordering between
// workgroups (no workgroup waits on another inside a launch, no load has to be fresh).
//
// State. The adjacency A holds every edge {u, v} of G as the two
// directed entries (u, v) and (v, u): three parallel arrays x, y (the 64-bit ids themselves)
// and seq (the number of the fold that added the edge), sorted by (x, y) in signed order. The
// row of a vertex is the contiguous range of its x value (gs_triangle_rows.hpp). The counter
// t(v) is the 64-bit word {link, aux} of v's slot in a relabel table of the existing layout
// (gs_device.hpp):
//   t(slot s) = (aux << 32 | link) - (s << 1)
// so the table's initial state (link = s << 1, aux = 0) reads as zero. INT64_MIN, the table's
// empty marker, keeps its presence flag and counter in two control words instead (the
// reserved slot's aux bit would sit inside a 64-bit counter).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gs_device.hpp"

namespace gs {

// Lanes that share one edge's shorter row in the product (gsamd.TRIANGLE_LANES): the lane
// group of the binned count kernel's short bin.
constexpr uint32_t TRIANGLE_LANES = 8;
// Edges per workgroup of the per-edge passes (gsamd.TRIANGLE_TILE): canonise, flag, compact.
constexpr uint32_t TRIANGLE_TILE = 1024;
constexpr uint32_t kTriBS = 256;                       // threads of every workgroup
constexpr uint32_t kTriPer = TRIANGLE_TILE / kTriBS;   // consecutive elements per thread
static_assert(TRIANGLE_TILE == kTriBS * kTriPer, "tile = threads x elements per thread");
constexpr uint32_t kTriShortRow = 4 * TRIANGLE_LANES;  // binned: shorter rows up to here take a lane group
constexpr uint32_t kTriWaveRow = 64;                   // binned: shorter rows above here may take a workgroup ...
constexpr uint32_t kTriLdsRow = 4096;                  // ... when the longer row has at least this many entries
constexpr uint32_t kTriSamples = 1024;                 // samples of the longer row staged in LDS (8 KiB)

// Work assignment of the count step (GS_TESTING_TRIANGLE_VARIANT; tools/triangle_bench.py)
enum TriangleVariant : int {
  kTriangleBinned = 0,  // product: lane group of 8 / wave / workgroup with LDS samples, by row length
  kTriangleWave = 1,    // one wave per new edge, 64 lanes striding the shorter row
  kTriangleVariants = 2,
  kTriangleProduct = kTriangleBinned
};

// control words (uint64) of a handle
enum TriCtl : int {
  TRI_T = 0,      // triangles of G        } the three words of
  TRI_E = 1,      // edges of G            } gs_triangle_count_device,
  TRI_NV = 2,     // vertices of G         } in this order
  TRI_NEW = 3,    // new edges of the current fold
  TRI_MINP = 4,   // INT64_MIN is a vertex
  TRI_MINC = 5,   // t(INT64_MIN)
  TRI_ROWS = 6,   // rows of the current export
  TRI_BIN1 = 7,   // binned count: edges in the wave list
  TRI_BIN2 = 8,   //               edges in the workgroup list
  TRI_STEPS = 9,  // diagnostics: sum over new edges of the shorter row length, since reset
  TRI_HOT = 10,   // diagnostics: the longest row a new edge met, since reset
  // the last removal (gs_triangle_remove / _expire), zeroed when one begins
  TRI_RNEW = 11,    // D, its dying edges
  TRI_RBIN1 = 12,   // binned count: dying edges in the removal's wave list
  TRI_RBIN2 = 13,   //               dying edges in the removal's workgroup list
  TRI_RSTEPS = 14,  // sum over the dying edges of the shorter row length
  TRI_RTRI = 15,    // triangles destroyed
  TRI_RVAN = 16,    // vertices whose every entry dies
  TRI_RLIVE = 17,   // surviving entries of A
  TRI_CTL_WORDS = 24
};

struct TriAdj {
  const int64_t* x = nullptr;
  const int64_t* y = nullptr;
  const uint32_t* seq = nullptr;
  uint64_t n = 0;
};

struct TriAdjOut {
  int64_t* x = nullptr;
  int64_t* y = nullptr;
  uint32_t* seq = nullptr;
  uint64_t cap = 0;
};

// per new edge: the shorter row [sb, se) and the longer row [lb, le) of its endpoints in A,
// and the table slots of the two endpoints
struct TriRowInfo {
  uint32_t sb, se, lb, le, ss, sl;
};

__host__ __device__ constexpr uint64_t tri_blocks(uint64_t n) { return (n + TRIANGLE_TILE - 1) / TRIANGLE_TILE; }

// Which entries of A the once-only rule treats as marked (gs_triangle_k.hip tri_walk), and
// whether a counted triangle is added or taken away. A fold marks the entries of its own
// number and adds; a removal marks the dying entries and adds the two's complement.
struct TriFoldMark {
  static constexpr bool kRemove = false;
  const uint32_t* seq;
  uint32_t cur;
  __host__ __device__ bool marked(uint64_t i) const { return seq[i] == cur; }
};
struct TriDyingMark {
  static constexpr bool kRemove = true;
  const uint8_t* dead;
  __host__ __device__ bool marked(uint64_t i) const { return dead[i] != 0; }
};

// every slot empty, link = slot << 1, aux = 0 (slots 0 .. cap)
void launch_tri_init(const Table& t, hipStream_t st);
// lo[i] = min, hi[i] = max of element i (src[i * stride], dst[i * stride]); loops stay as lo == hi
void launch_tri_canon(const int64_t* src, const int64_t* dst, uint64_t n, uint64_t stride, int64_t* lo, int64_t* hi,
                      hipStream_t st);
// Over the n rows (lo[pay[i]], hi[pay[i]]) sorted by (lo, hi): flags[i] = not a loop, not equal
// to the row before, not in A; blk[b] = flagged rows of tile b.
void launch_tri_flag_new(const uint32_t* pay, const int64_t* lo, const int64_t* hi, uint64_t n, const TriAdj& A,
                         uint8_t* flags, uint32_t* blk, hipStream_t st);
// the flagged rows in order into (nx, ny), at most cap of them; blk: the tile counts after
// gs_sort.hpp's launch_tile_scan (tri_blocks(n) + 1 words)
void launch_tri_compact_new(const uint32_t* pay, const int64_t* lo, const int64_t* hi, uint64_t n,
                            const uint8_t* flags, const uint32_t* blk, int64_t* nx, int64_t* ny, uint64_t cap,
                            hipStream_t st);
// rx[j] = ny[pay[j]], ry[j] = nx[pay[j]] for j < n (pay: the new edges ordered by (hi, lo))
void launch_tri_reverse(const uint32_t* pay, const int64_t* nx, const int64_t* ny, uint64_t n, int64_t* rx,
                        int64_t* ry, hipStream_t st);
// O = merge of A, the forward entries (nx, ny) and the reverse entries (rx, ry), n_new each, all
// sorted by (x, y) and disjoint; the new entries get fold number seq.
void launch_tri_merge(const TriAdj& A, const int64_t* nx, const int64_t* ny, const int64_t* rx, const int64_t* ry,
                      uint64_t n_new, const TriAdjOut& O, uint32_t seq, hipStream_t st);
// Per new edge: insert both endpoints into the table (ctl[TRI_NV] += fresh ones), find their
// rows in A, write info[e]; binned variant: append e to the wave / workgroup list by row length.
// ctl[TRI_E] += n_new.
void launch_tri_rows(const Table& t, unsigned long long* ctl, const TriAdj& A, const int64_t* nx, const int64_t* ny,
                     uint64_t n_new, TriRowInfo* info, uint32_t* list1, uint32_t* list2, int variant,
                     hipStream_t st);
// The same pass over the dying edges D while A still holds them. Nothing is inserted (a slot is
// found, or kNoSlot), TRI_E and TRI_NV stay, and the lists and the steps are the removal's own
// words (TRI_RBIN1, TRI_RBIN2, TRI_RSTEPS); TRI_STEPS / TRI_HOT / TRI_BIN1 / TRI_BIN2 keep
// meaning folds.
void launch_tri_rows_dying(const Table& t, unsigned long long* ctl, const TriAdj& A, const int64_t* dx,
                           const int64_t* dy, uint64_t n_dying, TriRowInfo* info, uint32_t* list1, uint32_t* list2,
                           int variant, hipStream_t st);
// the intersection: every triangle closed by a new edge counted once (the once-only rule)
void launch_tri_count(const Table& t, unsigned long long* ctl, const TriAdj& A, const int64_t* nx, const int64_t* ny,
                      uint64_t n_new, const TriRowInfo* info, const uint32_t* list1, const uint32_t* list2,
                      uint32_t seq, int variant, hipStream_t st);
// The same walk over the dying edges D with A's dying bytes as the marked set: every triangle
// that loses an edge is counted once, at its greatest dying edge, and taken from t(w), t(u),
// t(v) and T by a 64-bit add of the two's complement; ctl[TRI_RTRI] += the triangles destroyed.
void launch_tri_uncount(const Table& t, unsigned long long* ctl, const TriAdj& A, const uint8_t* dead,
                        const int64_t* dx, const int64_t* dy, uint64_t n_dying, const TriRowInfo* info,
                        const uint32_t* list1, const uint32_t* list2, int variant, hipStream_t st);
// As launch_tri_flag_new, but flags the rows that ARE in A, and sets dead[] of both directed
// entries of every flagged row (dead: A.n bytes, zero before).
void launch_tri_flag_dying(const uint32_t* pay, const int64_t* lo, const int64_t* hi, uint64_t n, const TriAdj& A,
                           uint8_t* flags, uint32_t* blk, uint8_t* dead, hipStream_t st);
// dead[i] = entry i's stamp is at least `folds` folds behind `cur` (cur - seq[i] >= folds, no
// stamp exceeds cur); flags[i] = dead[i] and x < y (D's entries, in order); blk as above
void launch_tri_mark_old(const TriAdj& A, uint32_t cur, uint64_t folds, uint8_t* dead, uint8_t* flags,
                         uint32_t* blk, hipStream_t st);
// blk[b] = surviving (dead[i] == 0) entries of tile b of the n entries
void launch_tri_live_count(const uint8_t* dead, uint64_t n, uint32_t* blk, hipStream_t st);
// pos[i] = surviving entries before entry i (blk after launch_tile_scan): where a survivor goes
void launch_tri_live_pos(const uint8_t* dead, uint64_t n, const uint32_t* blk, uint32_t* pos, hipStream_t st);
// ctl[TRI_RVAN] += the rows of A without a survivor (ctl[TRI_RLIVE]: the scan's total)
void launch_tri_vanish(const TriAdj& A, const uint8_t* dead, const uint32_t* pos, unsigned long long* ctl,
                       hipStream_t st);
// O[pos[i]] = A[i] for every survivor
void launch_tri_keep(const TriAdj& A, const uint8_t* dead, const uint32_t* pos, const TriAdjOut& O, hipStream_t st);
// After a removal of n_dying edges, O the compacted adjacency of n_live entries: TRI_E -= n_dying,
// TRI_NV -= TRI_RVAN, and INT64_MIN's presence flag and counter cleared when it heads no row.
void launch_tri_removed(unsigned long long* ctl, const int64_t* ox, uint64_t n_live, uint64_t n_dying,
                        hipStream_t st);
// Refresh: seq = cur for both directed entries of every element (lo[i], hi[i]), i < n, that is
// no loop and in A (seq: A's stamps, writable).
void launch_tri_restamp(const int64_t* lo, const int64_t* hi, uint64_t n, const TriAdj& A, uint32_t* seq,
                        uint32_t cur, hipStream_t st);
// The fold number wrapped: every stamp s becomes s - 2^31, or 0 when it is older than that.
void launch_tri_rebase(uint32_t* seq, uint64_t n, hipStream_t st);
// count[i] = t(v[i]) (0 when absent), found[i] (optional) = v[i] is a vertex of G
void launch_tri_find(const Table& t, const unsigned long long* ctl, const int64_t* v, uint64_t n, int64_t* count,
                     uint8_t* found, hipStream_t st);
// flags[i] = entry i heads its row (and, nonzero, its vertex has t > 0); blk as above
void launch_tri_flag_heads(const Table& t, const unsigned long long* ctl, const TriAdj& A, int nonzero,
                           uint8_t* flags, uint32_t* blk, hipStream_t st);
// the flagged vertices in order with their counters into (ov, oc), at most cap rows
void launch_tri_compact_rows(const Table& t, const unsigned long long* ctl, const TriAdj& A, const uint8_t* flags,
                             const uint32_t* blk, int64_t* ov, int64_t* oc, uint64_t cap, hipStream_t st);
// every vertex of A but INT64_MIN inserted into `to` with its counter of `from`
void launch_tri_rehash(const Table& from, const Table& to, const TriAdj& A, hipStream_t st);

}  // namespace gs
