// gs_slice_k.hip -- kernels of the window slices (gfx950).
//
//   k_slice_expand : edges -> entry keys (and the handle's copy of the edges)
//   k_slice_flag   : over the sorted keys: one head flag byte per position, heads per tile
//   k_slice_write  : the heads in order: vertex[] and offset[]; between the two, the sort's
//                    launch_tile_scan turns the tile counts into tile bases and the vertex count
//   k_slice_reduce : the hot kernel. A workgroup takes a tile of SLICE_TILE sorted positions,
//                    a thread kSlicePer consecutive ones: it gathers their values through the
//                    payload, combines its own run serially, the wave scans the threads'
//                    SegPairs with cross-lane shuffles and LDS joins the waves. A segment whose
//                    head and end are in the tile is stored at its rank; the tile's leading
//                    run and the value at its last position go to the carry record.
//   k_slice_carry  : exclusive segmented scan of the carry records (one workgroup)
//   k_slice_fixup  : out[rank] = op(carry in, leading run) for every tile in which a run that
//                    began in an earlier tile ends
//   k_slice_count / k_slice_gather / k_slice_stats : the COUNT op, the neighbourhood export,
//                    the diagnostics
// The segmented-combine operator and all tile / carry index arithmetic are gs_slice_seg.hpp's;
// the tile count, the rank inside a tile and the block-wide segmented scan are gs_scan.hpp's.
//
// What bounds every loop:
//   * per-element kernels handle one element per thread, its index tested against the count;
//   * tile kernels handle kSlicePer positions per thread, each tested against the entry count;
//     a flag word is read inside the flag array's whole tiles (k_slice_flag wrote all of them);
//   * the carry scan runs over the tile count in steps of its workgroup size;
//   * a payload is tested against the entry count, the edge it names against the edge count,
//     before either is used as an index;
//   * every output position is tested against the capacity of its array before the store.
// No kernel reads what another workgroup of the same launch writes.
#include "gs_scan.hpp"
#include "gs_slice.hpp"
#include "gs_slice_seg.hpp"
#include "gs_sort.hpp"

namespace gs {
namespace {

__global__ __launch_bounds__(kSliceBS) void k_slice_expand(const int64_t* src, const int64_t* dst, const int64_t* val,
                                                           uint64_t n, uint64_t stride, int dir, int copy,
                                                           int64_t* esrc, int64_t* edst, int64_t* eval, int64_t* kid) {
  const uint64_t i = (uint64_t)blockIdx.x * kSliceBS + threadIdx.x;
  if (i >= n) return;
  const int64_t s = src[i * stride], d = dst[i * stride];
  if (copy) {
    esrc[i] = s;
    edst[i] = d;
    if (val) eval[i] = val[i * stride];
  }
  if (dir == kSliceAll) {  // entry 2 i = the edge, entry 2 i + 1 = its reverse
    kid[2 * i] = s;
    kid[2 * i + 1] = d;
  } else {
    kid[i] = dir == kSliceOut ? s : d;
  }
}

__global__ __launch_bounds__(kSliceBS) void k_slice_flag(const unsigned long long* __restrict__ key, uint64_t entries,
                                                         uint8_t* __restrict__ flags, uint64_t flag_cap,
                                                         uint32_t* __restrict__ tcount) {
  __shared__ uint32_t total;
  const uint64_t base = slice_tile_begin(blockIdx.x, SLICE_TILE);
  uint32_t cnt = 0;
#pragma unroll
  for (uint32_t k = 0; k < kSlicePer; ++k) {
    const uint64_t i = base + k * kSliceBS + threadIdx.x;
    bool head = false;
    if (i < entries) head = i == 0 || key[i] != key[i - 1];
    if (i < flag_cap) flags[i] = head ? 1 : 0;
    cnt += head ? 1u : 0u;
  }
  block_count_to<kSliceBS>(cnt, &total, tcount + blockIdx.x);
}

// the 8 flag bytes of the thread's positions i0 .. i0 + 7 (i0 a multiple of 8 inside the whole
// tiles k_slice_flag wrote)
__device__ __forceinline__ uint64_t flag_word(const uint8_t* flags, uint64_t i0) {
  return *reinterpret_cast<const uint64_t*>(flags + i0);
}

__global__ __launch_bounds__(kSliceBS) void k_slice_write(const uint8_t* __restrict__ flags,
                                                          const unsigned long long* __restrict__ key, uint64_t entries,
                                                          const uint32_t* __restrict__ tbase, int64_t* __restrict__ vtx,
                                                          unsigned long long* __restrict__ off, uint64_t cap_v) {
  __shared__ uint32_t wsum[kSliceBS / 64];
  const uint64_t i0 = slice_tile_begin(blockIdx.x, SLICE_TILE) + (uint64_t)threadIdx.x * kSlicePer;
  const uint64_t fw = flag_word(flags, i0);
  uint64_t pos = (uint64_t)tbase[blockIdx.x] + block_excl_scan<kSliceBS>((uint32_t)__popcll(fw), wsum);
#pragma unroll
  for (uint32_t k = 0; k < kSlicePer; ++k) {
    if ((fw >> (8 * k)) & 1ull) {
      const uint64_t i = i0 + k;
      if (pos < cap_v && i < entries) {
        vtx[pos] = (int64_t)(key[i] ^ kSortSignBit);
        off[pos] = i;
      }
      ++pos;
    }
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
    const uint64_t nv = tbase[gridDim.x];
    if (nv <= cap_v) off[nv] = entries;  // (off holds cap_v + 1 words)
  }
}

template <int OP>
__global__ __launch_bounds__(kSliceBS) void k_slice_reduce(const uint8_t* __restrict__ flags,
                                                           const uint32_t* __restrict__ pay,
                                                           const int64_t* __restrict__ val, uint64_t entries,
                                                           uint64_t n_edges, int dir,
                                                           const uint32_t* __restrict__ tbase,
                                                           int64_t* __restrict__ out, uint64_t cap,
                                                           int64_t* __restrict__ lead, int64_t* __restrict__ trail) {
  __shared__ SegPair wtot[kSliceBS / 64];
  const uint64_t t = blockIdx.x;
  const uint64_t i0 = slice_tile_begin(t, SLICE_TILE) + (uint64_t)threadIdx.x * kSlicePer;
  const uint64_t tile_end = slice_tile_end(t, SLICE_TILE, entries);
  const uint64_t fw = flag_word(flags, i0);
  const bool next_head = i0 + kSlicePer < entries && flags[i0 + kSlicePer] != 0;
  uint32_t p[kSlicePer];
  if (i0 + kSlicePer <= entries) {  // (pay + i0 is 32-byte aligned)
    const uint4 a = *reinterpret_cast<const uint4*>(pay + i0);
    const uint4 b = *reinterpret_cast<const uint4*>(pay + i0 + 4);
    p[0] = a.x, p[1] = a.y, p[2] = a.z, p[3] = a.w;
    p[4] = b.x, p[5] = b.y, p[6] = b.z, p[7] = b.w;
  } else {
#pragma unroll
    for (uint32_t k = 0; k < kSlicePer; ++k) p[k] = i0 + k < entries ? pay[i0 + k] : 0u;
  }
  int64_t v[kSlicePer];
#pragma unroll
  for (uint32_t k = 0; k < kSlicePer; ++k) {  // the gathers of a thread in flight together
    const uint64_t e = slice_edge_of(p[k], dir);
    v[k] = slice_identity<OP>();
    if (i0 + k < entries && e < n_edges) v[k] = val[e];
  }
  // the thread's own stretch; v[k] becomes the value of its run up to position k
  SegPair run = seg_identity<OP>();
#pragma unroll
  for (uint32_t k = 0; k < kSlicePer; ++k) {
    if (i0 + k < entries) {
      seg_push<OP>(run, (fw >> (8 * k)) & 1ull, v[k]);
      v[k] = run.val;
    }
  }
  SegPair total;
  const SegPair before = block_seg_excl<kSliceBS, SliceSegOps<OP>>(run, wtot, &total);
  const uint64_t base = tbase[t];
#pragma unroll
  for (uint32_t k = 0; k < kSlicePer; ++k) {
    const uint64_t i = i0 + k;
    if (i >= entries) continue;
    const uint64_t upto = k + 1 < kSlicePer ? (1ull << (8 * (k + 1))) - 1ull : ~0ull;
    const uint32_t own = (uint32_t)__popcll(fw & upto);  // heads of the thread up to position k
    const uint32_t heads_incl = before.heads + own;
    const int64_t incl = own ? v[k] : slice_op<OP>(before.val, v[k]);
    const bool nh = k + 1 < kSlicePer ? ((fw >> (8 * (k + 1))) & 1ull) != 0 : next_head;
    const bool last = i + 1 == tile_end;
    const int emit = slice_emit(heads_incl, slice_closed(i, entries, nh), last);
    if (emit == kSliceEmitOut) {
      const uint64_t pos = slice_out_rank(base, heads_incl);
      if (pos < cap) out[pos] = incl;
    } else if (emit == kSliceEmitLead) {
      lead[t] = incl;
    }
    if (last) trail[t] = incl;
  }
}

// carry[t] = the value of the run open where tile t begins
template <int OP>
__global__ __launch_bounds__(kSliceBS) void k_slice_carry(const uint32_t* __restrict__ tbase,
                                                          const int64_t* __restrict__ trail, uint64_t nt,
                                                          int64_t* __restrict__ carry) {
  __shared__ SegPair wtot[kSliceBS / 64];
  SegPair run = seg_identity<OP>();  // the tiles before the chunk
  for (uint64_t c0 = 0; c0 < nt; c0 += kSliceBS) {
    const uint64_t t = c0 + threadIdx.x;
    SegPair a = seg_identity<OP>();
    if (t < nt) {
      a.heads = tbase[t + 1] - tbase[t];
      a.val = trail[t];
    }
    SegPair total;
    const SegPair ex = block_seg_excl<kSliceBS, SliceSegOps<OP>>(a, wtot, &total);
    if (t < nt) carry[t] = seg_combine<OP>(run, ex).val;
    run = seg_combine<OP>(run, total);
    __syncthreads();
  }
}

template <int OP>
__global__ __launch_bounds__(kSliceBS) void k_slice_fixup(const uint8_t* __restrict__ flags, uint64_t entries,
                                                          const uint32_t* __restrict__ tbase, uint64_t nt,
                                                          const int64_t* __restrict__ lead,
                                                          const int64_t* __restrict__ carry, int64_t* __restrict__ out,
                                                          uint64_t cap) {
  const uint64_t t = (uint64_t)blockIdx.x * kSliceBS + threadIdx.x;
  if (t >= nt) return;
  const uint64_t begin = slice_tile_begin(t, SLICE_TILE), end = slice_tile_end(t, SLICE_TILE, entries);
  if (begin >= end) return;
  const bool first = flags[begin] != 0;
  const uint32_t base = tbase[t], heads = tbase[t + 1] - base;
  const bool closed = slice_closed(end - 1, entries, end < entries && flags[end] != 0);
  if (!slice_fixup(t, first, heads, closed) || base == 0) return;
  const uint64_t pos = slice_fixup_rank(base);
  if (pos < cap) out[pos] = slice_op<OP>(carry[t], lead[t]);
}

__global__ __launch_bounds__(kSliceBS) void k_slice_count(const unsigned long long* __restrict__ off, uint64_t nv,
                                                          int64_t* __restrict__ out) {
  const uint64_t k = (uint64_t)blockIdx.x * kSliceBS + threadIdx.x;
  if (k < nv) out[k] = (int64_t)(off[k + 1] - off[k]);
}

__global__ __launch_bounds__(kSliceBS) void k_slice_gather(const uint32_t* __restrict__ pay, uint64_t entries,
                                                           uint64_t n_edges, int dir, const int64_t* __restrict__ esrc,
                                                           const int64_t* __restrict__ edst,
                                                           const int64_t* __restrict__ eval,
                                                           int64_t* __restrict__ neighbor, int64_t* __restrict__ val,
                                                           uint64_t cap) {
  const uint64_t i = (uint64_t)blockIdx.x * kSliceBS + threadIdx.x;
  if (i >= entries || i >= cap) return;
  const uint64_t q = pay[i];
  const uint64_t e = slice_edge_of(q, dir);
  if (q >= entries || e >= n_edges) return;
  neighbor[i] = slice_key_is_src(q, dir) ? edst[e] : esrc[e];
  if (val) val[i] = eval[e];
}

__global__ __launch_bounds__(kSliceBS) void k_slice_stats(const unsigned long long* __restrict__ off, uint64_t nv,
                                                          const uint32_t* __restrict__ tbase, uint64_t nt,
                                                          unsigned long long* __restrict__ ctl) {
  const uint64_t step = (uint64_t)gridDim.x * kSliceBS;
  unsigned long long longest = 0, nohead = 0;
  for (uint64_t k = (uint64_t)blockIdx.x * kSliceBS + threadIdx.x; k < nv; k += step) {
    const unsigned long long len = off[k + 1] - off[k];
    longest = len > longest ? len : longest;
  }
  for (uint64_t t = (uint64_t)blockIdx.x * kSliceBS + threadIdx.x; t < nt; t += step)
    nohead += tbase[t + 1] == tbase[t] ? 1 : 0;
  if (longest) atomicMax(ctl + SLICE_LONGEST, longest);
  if (nohead) atomicAdd(ctl + SLICE_NOHEAD, nohead);
}

uint32_t blocks_of(uint64_t n) { return (uint32_t)((n + kSliceBS - 1) / kSliceBS); }

template <int OP>
void reduce_launches(const uint8_t* flags, const uint32_t* pay, const int64_t* val, uint64_t entries, uint64_t n_edges,
                     int dir, const uint32_t* tbase, int64_t* out, uint64_t cap, int64_t* lead, int64_t* trail,
                     int64_t* carry, hipStream_t st) {
  const uint64_t nt = slice_tiles(entries, SLICE_TILE);
  hipLaunchKernelGGL(k_slice_reduce<OP>, dim3((uint32_t)nt), dim3(kSliceBS), 0, st, flags, pay, val, entries, n_edges,
                     dir, tbase, out, cap, lead, trail);
  if (nt < 2) return;  // (no run crosses a tile end)
  hipLaunchKernelGGL(k_slice_carry<OP>, dim3(1), dim3(kSliceBS), 0, st, tbase, (const int64_t*)trail, nt, carry);
  hipLaunchKernelGGL(k_slice_fixup<OP>, dim3(blocks_of(nt)), dim3(kSliceBS), 0, st, flags, entries, tbase, nt,
                     (const int64_t*)lead, (const int64_t*)carry, out, cap);
}

}  // namespace

void launch_slice_expand(const int64_t* src, const int64_t* dst, const int64_t* val, uint64_t n, uint64_t stride,
                         int dir, int64_t* esrc, int64_t* edst, int64_t* eval, int64_t* kid, hipStream_t st) {
  hipLaunchKernelGGL(k_slice_expand, dim3(blocks_of(n)), dim3(kSliceBS), 0, st, src, dst, val, n, stride, dir,
                     src == esrc ? 0 : 1, esrc, edst, eval, kid);
}

void launch_slice_heads(const unsigned long long* key, uint64_t entries, uint8_t* flags, uint32_t* tbase,
                        unsigned long long* ctl, int64_t* vtx, unsigned long long* off, uint64_t cap_v,
                        hipStream_t st) {
  const uint64_t nt = slice_tiles(entries, SLICE_TILE);
  hipLaunchKernelGGL(k_slice_flag, dim3((uint32_t)nt), dim3(kSliceBS), 0, st, key, entries, flags, nt * SLICE_TILE,
                     tbase);
  launch_tile_scan(tbase, nt, ctl + SLICE_NV, st);
  hipLaunchKernelGGL(k_slice_write, dim3((uint32_t)nt), dim3(kSliceBS), 0, st, (const uint8_t*)flags, key, entries,
                     (const uint32_t*)tbase, vtx, off, cap_v);
}

void launch_slice_reduce(int op, const uint8_t* flags, const uint32_t* pay, const int64_t* val, uint64_t entries,
                         uint64_t n_edges, int dir, const uint32_t* tbase, int64_t* out, uint64_t cap, int64_t* lead,
                         int64_t* trail, int64_t* carry, hipStream_t st) {
  if (op == kSliceSum)
    reduce_launches<kSliceSum>(flags, pay, val, entries, n_edges, dir, tbase, out, cap, lead, trail, carry, st);
  else if (op == kSliceMin)
    reduce_launches<kSliceMin>(flags, pay, val, entries, n_edges, dir, tbase, out, cap, lead, trail, carry, st);
  else if (op == kSliceMax)
    reduce_launches<kSliceMax>(flags, pay, val, entries, n_edges, dir, tbase, out, cap, lead, trail, carry, st);
}

void launch_slice_count(const unsigned long long* off, uint64_t nv, int64_t* out, hipStream_t st) {
  hipLaunchKernelGGL(k_slice_count, dim3(blocks_of(nv)), dim3(kSliceBS), 0, st, off, nv, out);
}

void launch_slice_gather(const uint32_t* pay, uint64_t entries, uint64_t n_edges, int dir, const int64_t* esrc,
                         const int64_t* edst, const int64_t* eval, int64_t* neighbor, int64_t* val, uint64_t cap,
                         hipStream_t st) {
  hipLaunchKernelGGL(k_slice_gather, dim3(blocks_of(entries)), dim3(kSliceBS), 0, st, pay, entries, n_edges, dir, esrc,
                     edst, eval, neighbor, val, cap);
}

void launch_slice_stats(const unsigned long long* off, uint64_t nv, const uint32_t* tbase, uint64_t tiles,
                        unsigned long long* ctl, hipStream_t st) {
  const uint64_t work = nv > tiles ? nv : tiles;
  const uint32_t want = blocks_of(work);
  hipLaunchKernelGGL(k_slice_stats, dim3(want < 256 ? (want ? want : 1) : 256), dim3(kSliceBS), 0, st, off, nv, tbase,
                     tiles, ctl);
}

}  // namespace gs
