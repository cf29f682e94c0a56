// gs_slice.hpp -- host-side launchers of the window slices' kernels (gs_slice_k.hip): expand a
// window of (src, dst, value) into keyed entries, find the heads of the sorted entries and
// write the vertices and offsets, reduce the values of every neighbourhood in one pass, and
// gather neighbours and values into sorted order. The sort in between, its one-column digit
// histogram and the scan of the tile counts are gs_sort.hpp's. Every
// launch is queued on the given stream; kernel boundaries carry all ordering between
// workgroups (no workgroup waits on another inside a launch).
//
// State. A window of n edges has E = n (OUT, IN) or 2 n (ALL) entries;
// entry e is keyed by one endpoint of edge slice_edge_of(e) (gs_slice_seg.hpp). The handle
// keeps the edges (src, dst, val: n each), the entry keys (E), the sorted (key, payload) pairs
// in the sort's scratch, one head flag byte per sorted position (whole tiles, zero past E),
// the heads before every tile (tiles + 1 words), the vertices and offsets (nv, nv + 1), and
// per tile the leading-run, last-position and carry-in values of the last reduce.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gs_slice_seg.hpp"

namespace gs {

// Sorted positions per workgroup of the heads, write and reduce kernels (gsamd.SLICE_TILE).
constexpr uint32_t SLICE_TILE = 2048;
constexpr uint32_t kSliceBS = 256;                      // threads of every workgroup
constexpr uint32_t kSlicePer = SLICE_TILE / kSliceBS;   // consecutive positions per thread
static_assert(SLICE_TILE == kSliceBS * kSlicePer, "tile = threads x positions per thread");
static_assert(kSlicePer == 8, "a thread's head flags are the 8 bytes of one 64-bit word");

// control words (uint64) of a handle
enum SliceCtl : int {
  SLICE_NV = 0,       // vertices of the window
  SLICE_LONGEST = 1,  // diagnostics: the longest segment
  SLICE_NOHEAD = 2,   // diagnostics: tiles without a head
  SLICE_CTL_WORDS = 8
};

// Edge i = (src[i * stride], dst[i * stride], val[i * stride]) (val may be null). Writes the
// entry keys of direction dir into kid (slice_entries(n, dir) of them) and, unless src == esrc
// (the edges are in place already), the edges into esrc / edst / eval.
void launch_slice_expand(const int64_t* src, const int64_t* dst, const int64_t* val, uint64_t n, uint64_t stride,
                         int dir, int64_t* esrc, int64_t* edst, int64_t* eval, int64_t* kid, hipStream_t st);
// Over E sorted keys: flags[i] = position i is a head (whole tiles are written, 0 from E on),
// tbase[t] = heads before tile t and tbase[tiles] = ctl[SLICE_NV] = all heads; vtx / off =
// the vertices and the first position of each, off[heads] = E. Writes are bounded by cap_v heads.
void launch_slice_heads(const unsigned long long* key, uint64_t entries, uint8_t* flags, uint32_t* tbase,
                        unsigned long long* ctl, int64_t* vtx, unsigned long long* off, uint64_t cap_v,
                        hipStream_t st);
// out[k] = op over the values of vertex k's entries, k < cap (op: SUM, MIN or MAX). pay: the
// sorted payloads; val: n_edges values; lead / trail / carry: one word per tile.
void launch_slice_reduce(int op, const uint8_t* flags, const uint32_t* pay, const int64_t* val, uint64_t entries,
                         uint64_t n_edges, int dir, const uint32_t* tbase, int64_t* out, uint64_t cap, int64_t* lead,
                         int64_t* trail, int64_t* carry, hipStream_t st);
// out[k] = off[k + 1] - off[k], k < nv
void launch_slice_count(const unsigned long long* off, uint64_t nv, int64_t* out, hipStream_t st);
// neighbor[p] = the other endpoint, val[p] (val may be null) = the value of sorted position p < min(entries, cap)
void launch_slice_gather(const uint32_t* pay, uint64_t entries, uint64_t n_edges, int dir, const int64_t* esrc,
                         const int64_t* edst, const int64_t* eval, int64_t* neighbor, int64_t* val, uint64_t cap,
                         hipStream_t st);
// ctl[SLICE_LONGEST] = max (off[k + 1] - off[k]), ctl[SLICE_NOHEAD] = tiles t with tbase[t + 1] == tbase[t]
void launch_slice_stats(const unsigned long long* off, uint64_t nv, const uint32_t* tbase, uint64_t tiles,
                        unsigned long long* ctl, hipStream_t st);

}  // namespace gs
