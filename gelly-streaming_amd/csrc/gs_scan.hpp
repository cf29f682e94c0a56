// gs_scan.hpp -- the device primitives of the flag / scan / compact idiom (gfx950): a kernel
// flags its elements and counts them per tile (block_count_to), launch_tile_scan (gs_sort.hpp)
// turns the tile counts into tile bases, and a second kernel ranks every kept element inside its
// tile (block_excl_scan) and writes the kept rows in order. block_seg_excl is the same block scan
// over a summary's own segmented element (slices, degree streams, triangle streams). Device
// functions only: a kernel in a header would be compiled into every code object that includes it.
//
// Every thread of the workgroup calls these (they hold barriers), from uniform control flow, in
// a workgroup of whole waves. How a kernel loads its flags and turns (tile base, rank) into an
// output row stays with the kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gs {

// sum of x over the lanes of the wave up to and including this one
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t x) {
  const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = __shfl_up(x, o, 64);
    if ((int)lane >= o) x += y;
  }
  return x;
}

// Sum of cnt over the threads of the workgroup before this one (threads in order): the rank of
// the thread's first kept element inside its tile when a thread owns consecutive elements.
// wsum: BS / 64 words of LDS, holding the waves' sums afterwards; the caller separates two
// calls on the same words with a barrier.
template <uint32_t BS>
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t cnt, uint32_t* wsum) {
  static_assert(BS % 64 == 0, "whole waves");
  const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
  const uint32_t inc = wave_incl_scan(cnt);
  if (lane == 63) wsum[wid] = inc;
  __syncthreads();
  uint32_t wbase = 0;
#pragma unroll
  for (uint32_t q = 0; q < BS / 64; ++q)
    if (q < wid) wbase += wsum[q];
  return wbase + (inc - cnt);
}

// *out = sum of cnt over the workgroup (thread 0 stores it). total_lds: one word of LDS; one
// LDS atomic per wave that kept anything.
template <uint32_t BS>
__device__ __forceinline__ void block_count_to(uint32_t cnt, uint32_t* total_lds, uint32_t* out) {
  static_assert(BS % 64 == 0, "whole waves");
  if (threadIdx.x == 0) *total_lds = 0;
  __syncthreads();
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if ((threadIdx.x & 63u) == 0 && cnt) atomicAdd(total_lds, cnt);
  __syncthreads();
  if (threadIdx.x == 0) *out = *total_lds;
}

// The segmented form, over any associative combine. Ops supplies the element type Seg,
// identity(), combine(first, then) and shfl_up(x, o), the wave shuffle of a Seg field by field.
// Returns the combination of `mine` over the threads of the workgroup before this one (threads in
// order), and *total = over all of them. wagg: BS / 64 Seg of LDS; holds a barrier after every
// thread's earlier loads; the caller separates two calls on the same words with a barrier.
template <uint32_t BS, class Ops>
__device__ __forceinline__ typename Ops::Seg block_seg_excl(typename Ops::Seg mine, typename Ops::Seg* wagg,
                                                            typename Ops::Seg* total) {
  static_assert(BS % 64 == 0, "whole waves");
  using Seg = typename Ops::Seg;
  const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
  Seg inc = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const Seg y = Ops::shfl_up(inc, o);
    if ((int)lane >= o) inc = Ops::combine(y, inc);
  }
  if (lane == 63) wagg[wid] = inc;
  Seg excl = Ops::shfl_up(inc, 1);
  if (lane == 0) excl = Ops::identity();
  __syncthreads();
  Seg base = Ops::identity(), all = Ops::identity();
#pragma unroll
  for (uint32_t q = 0; q < BS / 64; ++q) {
    const Seg w = wagg[q];
    if (q < wid) base = Ops::combine(base, w);
    all = Ops::combine(all, w);
  }
  *total = all;
  return Ops::combine(base, excl);
}

}  // namespace gs
