// gs_slice_seg.hpp -- the segmented-combine operator and the tile / carry index arithmetic of
// the window slices (gs_slice_k.hip). Plain functions of their arguments: the header compiles
// with a host compiler too (tests/cpp/slice_seg_sanitize.cpp runs the arithmetic tile by tile
// against brute force under the address and UB sanitizers).
//
// The sorted entries of a window are cut into tiles of `tile` consecutive positions. A
// position is a head when its key differs from the position before it (position 0 is one); a
// segment is a head and the positions up to the next head. A SegPair is what a stretch of
// positions contributes: the heads in it and the value of its trailing open run (the values
// since its last head, or all of them when it has none). seg_combine joins two adjacent
// stretches; it is associative, so threads, waves, workgroups and launches may join their
// stretches in any grouping that keeps the order.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GS_SLICE_HD __host__ __device__ inline
#else
#define GS_SLICE_HD inline
#endif

namespace gs {

// the values of include/gs_summary.h's gs_slice_dir and gs_slice_op
enum SliceDir : int { kSliceOut = 0, kSliceIn = 1, kSliceAll = 2, kSliceDirs = 3 };
enum SliceOp : int { kSliceSum = 0, kSliceMin = 1, kSliceMax = 2, kSliceCount = 3, kSliceOps = 4 };

constexpr int64_t kSliceI64Max = 0x7FFFFFFFFFFFFFFFll;
constexpr int64_t kSliceI64Min = -kSliceI64Max - 1;

template <int OP>
GS_SLICE_HD int64_t slice_identity() {
  return OP == kSliceMin ? kSliceI64Max : OP == kSliceMax ? kSliceI64Min : 0;
}

// SUM wraps as two's complement (Java long); MIN and MAX are signed
template <int OP>
GS_SLICE_HD int64_t slice_op(int64_t a, int64_t b) {
  if (OP == kSliceMin) return b < a ? b : a;
  if (OP == kSliceMax) return b > a ? b : a;
  return (int64_t)((uint64_t)a + (uint64_t)b);
}

struct SegPair {
  uint32_t heads;  // heads in the stretch
  int64_t val;     // value of its trailing open run
};

template <int OP>
GS_SLICE_HD SegPair seg_identity() {
  SegPair r;
  r.heads = 0;
  r.val = slice_identity<OP>();
  return r;
}

// stretch a followed by stretch b
template <int OP>
GS_SLICE_HD SegPair seg_combine(const SegPair& a, const SegPair& b) {
  SegPair r;
  r.heads = a.heads + b.heads;
  r.val = b.heads ? b.val : slice_op<OP>(a.val, b.val);
  return r;
}

// the stretch `run` extended by one position
template <int OP>
GS_SLICE_HD void seg_push(SegPair& run, bool head, int64_t v) {
  if (head) {
    run.heads += 1;
    run.val = v;
  } else {
    run.val = slice_op<OP>(run.val, v);
  }
}

#if defined(__HIPCC__)
// what gs_scan.hpp's block_seg_excl needs of a SegPair
template <int OP>
struct SliceSegOps {
  using Seg = SegPair;
  static __device__ __forceinline__ SegPair identity() { return seg_identity<OP>(); }
  static __device__ __forceinline__ SegPair combine(const SegPair& a, const SegPair& b) { return seg_combine<OP>(a, b); }
  static __device__ __forceinline__ SegPair shfl_up(const SegPair& p, int o) {
    SegPair r;
    r.heads = __shfl_up(p.heads, o, 64);
    r.val = (int64_t)__shfl_up((long long)p.val, o, 64);
    return r;
  }
};
#endif

// ---- entries of a window of n edges
GS_SLICE_HD uint64_t slice_entries(uint64_t n, int dir) { return dir == kSliceAll ? 2 * n : n; }
// the edge an entry (a sort payload) came from
GS_SLICE_HD uint64_t slice_edge_of(uint64_t entry, int dir) { return dir == kSliceAll ? entry >> 1 : entry; }
// the entry is keyed by its edge's source (its neighbour is the target), or the reverse
GS_SLICE_HD bool slice_key_is_src(uint64_t entry, int dir) {
  return dir == kSliceOut || (dir == kSliceAll && (entry & 1) == 0);
}

// ---- tiles
GS_SLICE_HD uint64_t slice_tiles(uint64_t entries, uint32_t tile) { return (entries + tile - 1) / tile; }
GS_SLICE_HD uint64_t slice_tile_begin(uint64_t t, uint32_t tile) { return t * tile; }
GS_SLICE_HD uint64_t slice_tile_end(uint64_t t, uint32_t tile, uint64_t entries) {
  const uint64_t e = (t + 1) * tile;
  return e < entries ? e : entries;
}

// the segment of position i ends at i: i is the last entry or position i + 1 is a head
GS_SLICE_HD bool slice_closed(uint64_t i, uint64_t entries, bool next_is_head) {
  return i + 1 >= entries || next_is_head;
}

// What a tile does with the inclusive pair of position i (the stretch from the tile's first
// position to i): a segment that ends at i and whose head is in the tile is written out; a run
// without a head in the tile that ends at i, or reaches the tile's last position, is the
// tile's leading run (at most one position of a tile qualifies).
enum SliceEmit : int { kSliceEmitNone = 0, kSliceEmitOut = 1, kSliceEmitLead = 2 };
GS_SLICE_HD int slice_emit(uint32_t heads_incl, bool closed, bool last_of_tile) {
  if (heads_incl) return closed ? kSliceEmitOut : kSliceEmitNone;
  return (closed || last_of_tile) ? kSliceEmitLead : kSliceEmitNone;
}
// row of the segment whose head is the heads_incl-th (>= 1) of a tile with tile_base heads before it
GS_SLICE_HD uint64_t slice_out_rank(uint64_t tile_base, uint32_t heads_incl) { return tile_base + heads_incl - 1; }

// ---- carries. The record of tile t is SegPair{heads of t, value at t's last position}; the
// exclusive seg_combine scan of the records gives carry_in[t].val, the value of the run that
// is open where tile t begins. The run ends inside tile t -- and tile t writes
// out[slice_fixup_rank] = op(carry_in, leading run) -- when t does not begin with a head and
// either holds a head or is closed at its end.
GS_SLICE_HD bool slice_fixup(uint64_t t, bool first_is_head, uint32_t heads_in_tile, bool closed_at_end) {
  return t > 0 && !first_is_head && (heads_in_tile > 0 || closed_at_end);
}
GS_SLICE_HD uint64_t slice_fixup_rank(uint64_t tile_base) { return tile_base - 1; }

}  // namespace gs
