// gs_sort_k.hip -- kernels of the grouped component export (gs_export_components*):
//
//   k_sort_digits  : histograms of all 8 digits of the vertex keys and of the label keys of
//                    the exported rows in one pass, plus the count of roots. The host reads
//                    them once: a digit whose histogram has one bin equal to n is an identity
//                    pass and is skipped; each digit's global base for k_sort_scan comes from
//                    the same histogram (the multiset of keys does not depend on their order).
//   k_sort_hist    : one pass's digit counts per workgroup tile, digit-major.
//   k_sort_scan    : exclusive scan of that table, one workgroup per digit row (rows are
//                    independent once the digit's global base is known).
//   k_sort_scatter : stable scatter of one tile: wave-level digit matching with 64-bit
//                    __ballot gives each pair its rank among the pairs of its digit in its
//                    wave's chunk, wave totals in LDS order the waves, the scanned table
//                    orders the workgroups.
//   k_comp_roots   : rows with v == label (gs_num_components; no sort).
//   k_comp_heads / k_comp_write : the CSR tail over rows sorted by (label, vertex).
// and two kernels every summary with a sort or a compaction shares:
//   k_sort_digits_one : the histograms of all 8 digits of one key column (the window slices,
//                    the distinct streams' edge export).
//   k_tile_scan    : exclusive scan of the tile counts of a flag / scan / compact pass, one
//                    workgroup; the wave and workgroup scans are gs_scan.hpp's.
//
// A pass is three launches; kernel boundaries give all ordering between workgroups, so no
// workgroup waits on another and nothing relies on coherence between the per-XCD L2s
// inside a launch. Keys are id ^ 2^63: unsigned digit order is signed id order.
#include "gs_scan.hpp"
#include "gs_sort.hpp"

namespace gs {
namespace {

__device__ __forceinline__ void load_pair(const SortSrc& s, uint64_t i, unsigned long long& key, uint32_t& pay) {
  pay = s.pay ? s.pay[i] : (uint32_t)i;
  key = s.key ? s.key[i] : ((unsigned long long)(pay < s.rows ? s.ids[pay] : 0) ^ kSortSignBit);
}

// LDS histogram add of a whole wave (every lane calls it). A wave whose valid lanes all
// hold one digit -- the high digits of dense ids -- adds once instead of 64 times to one
// address.
__device__ __forceinline__ void hist_add(uint32_t* h, uint32_t d, bool valid) {
  const unsigned long long m = __ballot(valid);
  if (!m) return;  // wave-uniform
  const int first = __ffsll((long long)m) - 1;
  const uint32_t d0 = (uint32_t)__shfl((int)d, first, 64);
  if (__ballot(valid && d != d0) == 0ull) {
    if ((int)(threadIdx.x & 63) == first) atomicAdd(&h[d0], (uint32_t)__popcll(m));
  } else if (valid) {
    atomicAdd(&h[d], 1u);
  }
}

constexpr uint32_t kDigitsPer = 4;  // rows per thread and iteration of k_sort_digits

__global__ __launch_bounds__(256) void k_sort_digits(const int64_t* __restrict__ v, const int64_t* __restrict__ l,
                                                     uint64_t n, uint32_t* __restrict__ ctl) {
  __shared__ uint32_t h[kSortCtlRoots];
  __shared__ uint32_t roots;
  for (uint32_t k = threadIdx.x; k < kSortCtlRoots; k += 256) h[k] = 0;
  if (threadIdx.x == 0) roots = 0;
  __syncthreads();
  const uint64_t step = (uint64_t)gridDim.x * (256 * kDigitsPer);
  for (uint64_t base = (uint64_t)blockIdx.x * (256 * kDigitsPer); base < n; base += step) {
    unsigned long long kv[kDigitsPer], kl[kDigitsPer];
#pragma unroll
    for (uint32_t j = 0; j < kDigitsPer; ++j) {  // the loads of an iteration in flight together
      const uint64_t i = base + j * 256 + threadIdx.x;
      kv[j] = kl[j] = 0;
      if (i < n) {
        kv[j] = (unsigned long long)v[i] ^ kSortSignBit;
        kl[j] = (unsigned long long)l[i] ^ kSortSignBit;
      }
    }
#pragma unroll
    for (uint32_t j = 0; j < kDigitsPer; ++j) {
      const bool valid = base + j * 256 + threadIdx.x < n;
#pragma unroll
      for (uint32_t p = 0; p < kSortPasses; ++p) {
        hist_add(h + p * kSortRadix, (uint32_t)(kv[j] >> (8 * p)) & 255u, valid);
        hist_add(h + (kSortPasses + p) * kSortRadix, (uint32_t)(kl[j] >> (8 * p)) & 255u, valid);
      }
      const unsigned long long r = __ballot(valid && kv[j] == kl[j]);
      if ((threadIdx.x & 63) == 0 && r) atomicAdd(&roots, (uint32_t)__popcll(r));
    }
  }
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < kSortCtlRoots; k += 256)
    if (h[k]) atomicAdd(&ctl[k], h[k]);
  if (threadIdx.x == 0 && roots) atomicAdd(&ctl[kSortCtlRoots], roots);
}

constexpr uint32_t kDigitsOneBins = kSortPasses * kSortRadix;  // the eight 256-bin rows of one key column
constexpr uint32_t kDigitsOneBlocks = 256;  // at most: every workgroup ends with one global add per bin

// ctl[0 .. kDigitsOneBins) += the histograms of all 8 digits of the keys (ctl zero before)
__global__ __launch_bounds__(256) void k_sort_digits_one(const int64_t* __restrict__ id, uint64_t n,
                                                         uint32_t* __restrict__ ctl) {
  __shared__ uint32_t h[kDigitsOneBins];
  for (uint32_t k = threadIdx.x; k < kDigitsOneBins; k += 256) h[k] = 0;
  __syncthreads();
  const uint64_t step = (uint64_t)gridDim.x * (256 * kDigitsPer);
  for (uint64_t base = (uint64_t)blockIdx.x * (256 * kDigitsPer); base < n; base += step) {
    unsigned long long key[kDigitsPer];
#pragma unroll
    for (uint32_t j = 0; j < kDigitsPer; ++j) {  // the loads of an iteration in flight together
      const uint64_t i = base + j * 256 + threadIdx.x;
      key[j] = i < n ? (unsigned long long)id[i] ^ kSortSignBit : 0ull;
    }
#pragma unroll
    for (uint32_t j = 0; j < kDigitsPer; ++j) {
      const bool valid = base + j * 256 + threadIdx.x < n;
#pragma unroll
      for (uint32_t p = 0; p < kSortPasses; ++p)
        hist_add(h + p * kSortRadix, (uint32_t)(key[j] >> (8 * p)) & 255u, valid);
    }
  }
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < kDigitsOneBins; k += 256)
    if (h[k]) atomicAdd(&ctl[k], h[k]);
}

__global__ __launch_bounds__(256) void k_comp_roots(const int64_t* __restrict__ v, const int64_t* __restrict__ l,
                                                    uint64_t n, unsigned long long* __restrict__ out) {
  __shared__ uint32_t roots;
  if (threadIdx.x == 0) roots = 0;
  __syncthreads();
  const uint64_t step = (uint64_t)gridDim.x * 256;
  for (uint64_t base = (uint64_t)blockIdx.x * 256; base < n; base += step) {
    const uint64_t i = base + threadIdx.x;
    const unsigned long long r = __ballot(i < n && v[i] == l[i]);
    if ((threadIdx.x & 63) == 0 && r) atomicAdd(&roots, (uint32_t)__popcll(r));
  }
  __syncthreads();
  if (threadIdx.x == 0 && roots) atomicAdd(out, (unsigned long long)roots);
}

// table[digit * stride + workgroup] = pairs of the workgroup's tile with that digit
__global__ __launch_bounds__(kSortBS) void k_sort_hist(SortSrc s, uint64_t n, int shift, uint32_t* __restrict__ table,
                                                       uint64_t stride) {
  __shared__ uint32_t h[kSortRadix];
  h[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t base = (uint64_t)blockIdx.x * kSortTile;
  unsigned long long key[kSortItems];
#pragma unroll
  for (uint32_t j = 0; j < kSortItems; ++j) {
    const uint64_t i = base + j * kSortBS + threadIdx.x;
    uint32_t pay;
    key[j] = 0;
    if (i < n) load_pair(s, i, key[j], pay);
  }
#pragma unroll
  for (uint32_t j = 0; j < kSortItems; ++j)
    hist_add(h, (uint32_t)(key[j] >> shift) & 255u, base + j * kSortBS + threadIdx.x < n);
  __syncthreads();
  table[(uint64_t)threadIdx.x * stride + blockIdx.x] = h[threadIdx.x];
}

// Exclusive scan of row blockIdx.x of the table (`entries` live words of `stride`), starting
// from the sum of ghist[0 .. blockIdx.x) (0 without ghist): entry (d, b) becomes the first
// output position of workgroup b's pairs with digit d.
__global__ __launch_bounds__(kSortScanBS) void k_sort_scan(uint32_t* __restrict__ table, uint64_t entries,
                                                           uint64_t stride, const uint32_t* __restrict__ ghist) {
  __shared__ uint32_t ws[kSortScanBS / 64];
  __shared__ uint32_t base_sh;
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t d = blockIdx.x;
  if (threadIdx.x < 64) {
    uint32_t x = 0;
    if (ghist)
      for (uint32_t k = lane * 4; k < lane * 4 + 4; ++k)
        if (k < d) x += ghist[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    if (lane == 0) base_sh = x;
  }
  __syncthreads();
  uint32_t carry = base_sh;
  uint32_t* row = table + (uint64_t)d * stride;
  for (uint64_t c0 = 0; c0 < entries; c0 += kSortScanBS * 4) {
    const uint64_t c = c0 + (uint64_t)threadIdx.x * 4;
    uint4 x = make_uint4(0, 0, 0, 0);
    if (c < stride) x = *reinterpret_cast<const uint4*>(row + c);  // stride is a multiple of 4: c + 3 < stride
    if (c + 0 >= entries) x.x = 0;
    if (c + 1 >= entries) x.y = 0;
    if (c + 2 >= entries) x.z = 0;
    if (c + 3 >= entries) x.w = 0;
    const uint32_t before = block_excl_scan<kSortScanBS>(x.x + x.y + x.z + x.w, ws);
    uint32_t total = 0;
#pragma unroll
    for (uint32_t q = 0; q < kSortScanBS / 64; ++q) total += ws[q];
    uint4 o;
    o.x = carry + before;
    o.y = o.x + x.x;
    o.z = o.y + x.y;
    o.w = o.z + x.z;
    if (c < stride) *reinterpret_cast<uint4*>(row + c) = o;
    carry += total;
    __syncthreads();
  }
}

// tb[0 .. nt) -> their exclusive scan, tb[nt] = *total_out = the sum. The carry has 32 bits:
// the counts are of kept elements, and every caller bounds its elements by 2^32 - 1
// (kSliceMaxEntries, kTriMaxEntries, 2 kDistMaxFold), so the sum fits.
__global__ __launch_bounds__(kSortScanBS) void k_tile_scan(uint32_t* __restrict__ tb, uint64_t nt,
                                                           unsigned long long* __restrict__ total_out) {
  __shared__ uint32_t ws[kSortScanBS / 64];
  uint32_t carry = 0;
  for (uint64_t c0 = 0; c0 < nt; c0 += kSortScanBS) {  // block-uniform
    const uint64_t i = c0 + threadIdx.x;
    const uint32_t before = block_excl_scan<kSortScanBS>(i < nt ? tb[i] : 0u, ws);
    uint32_t total = 0;
#pragma unroll
    for (uint32_t q = 0; q < kSortScanBS / 64; ++q) total += ws[q];
    if (i < nt) tb[i] = carry + before;
    carry += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    tb[nt] = carry;
    *total_out = carry;
  }
}

// Stable scatter of tile blockIdx.x. Wave w owns the contiguous chunk of 64 * kSortItems
// pairs at tile + w * 64 * kSortItems, item j of lane l being pair j * 64 + l of the chunk,
// so (wave, item, lane) order is input order.
__global__ __launch_bounds__(kSortBS) void k_sort_scatter(SortSrc s, uint64_t n, int shift,
                                                          const uint32_t* __restrict__ table, uint64_t stride,
                                                          unsigned long long* __restrict__ okey,
                                                          uint32_t* __restrict__ opay) {
  constexpr uint32_t kWaves = kSortBS / 64;
  __shared__ uint32_t wcnt[kWaves][kSortRadix];
  const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  for (uint32_t k = threadIdx.x; k < kWaves * kSortRadix; k += kSortBS) (&wcnt[0][0])[k] = 0;
  const uint64_t base = (uint64_t)blockIdx.x * kSortTile + (uint64_t)wid * (64 * kSortItems);
  unsigned long long key[kSortItems];
  uint32_t pay[kSortItems], rank[kSortItems];
#pragma unroll
  for (uint32_t j = 0; j < kSortItems; ++j) {
    const uint64_t i = base + j * 64 + lane;
    key[j] = 0;
    pay[j] = 0;
    if (i < n) load_pair(s, i, key[j], pay[j]);
  }
  __syncthreads();
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (uint32_t j = 0; j < kSortItems; ++j) {
    const bool valid = base + j * 64 + lane < n;
    const uint32_t d = (uint32_t)(key[j] >> shift) & 255u;
    unsigned long long m = __ballot(valid);  // the valid lanes holding this lane's digit
#pragma unroll
    for (uint32_t bit = 0; bit < 8; ++bit) {
      const bool on = (d >> bit) & 1u;
      const unsigned long long bal = __ballot(on);
      m &= on ? bal : ~bal;
    }
    const uint32_t prev = wcnt[wid][d];
    rank[j] = prev + (uint32_t)__popcll(m & below);
    __builtin_amdgcn_wave_barrier();  // every lane of the wave has read the count before its leader moves it on
    if (valid && (m & below) == 0ull) wcnt[wid][d] = prev + (uint32_t)__popcll(m);
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  {  // thread d: the waves' counts of digit d become their first output positions
    uint32_t run = table[(uint64_t)threadIdx.x * stride + blockIdx.x];
#pragma unroll
    for (uint32_t w = 0; w < kWaves; ++w) {
      const uint32_t c = wcnt[w][threadIdx.x];
      wcnt[w][threadIdx.x] = run;
      run += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (uint32_t j = 0; j < kSortItems; ++j) {
    if (base + j * 64 + lane < n) {
      const uint64_t dst = (uint64_t)wcnt[wid][(uint32_t)(key[j] >> shift) & 255u] + rank[j];
      if (dst < n) {  // (always: the positions partition [0, n))
        okey[dst] = key[j];
        opay[dst] = pay[j];
      }
    }
  }
}

// ---- CSR tail. A thread owns 4 consecutive positions; position i is a head when its label
// key differs from position i - 1's.
constexpr uint32_t kCompPer = kCompTile / 256;

__device__ __forceinline__ uint32_t comp_load(const SortSrc& s, uint64_t n, uint64_t i0,
                                              unsigned long long (&key)[kCompPer], uint32_t (&pay)[kCompPer]) {
  unsigned long long prev = 0;
  uint32_t heads = 0;
  if (i0 > 0 && i0 < n) {
    uint32_t pp;
    load_pair(s, i0 - 1, prev, pp);
  }
#pragma unroll
  for (uint32_t k = 0; k < kCompPer; ++k) {
    const uint64_t i = i0 + k;
    key[k] = 0;
    pay[k] = 0;
    if (i < n) {
      load_pair(s, i, key[k], pay[k]);
      if (i == 0 || key[k] != prev) heads |= 1u << k;
      prev = key[k];
    }
  }
  return heads;
}

__global__ __launch_bounds__(256) void k_comp_heads(SortSrc s, uint64_t n, uint32_t* __restrict__ bcount) {
  __shared__ uint32_t total;
  unsigned long long key[kCompPer];
  uint32_t pay[kCompPer];
  const uint32_t heads = comp_load(s, n, (uint64_t)blockIdx.x * kCompTile + (uint64_t)threadIdx.x * kCompPer, key, pay);
  block_count_to<256>((uint32_t)__popc(heads), &total, bcount + blockIdx.x);
}

// bbase = the scanned head counts: heads of workgroup b take comp / offset entries from bbase[b]
__global__ __launch_bounds__(256) void k_comp_write(SortSrc s, uint64_t n, const uint32_t* __restrict__ bbase,
                                                    const int64_t* __restrict__ v, const uint8_t* __restrict__ parity,
                                                    int sign_kind, int64_t* __restrict__ comp,
                                                    unsigned long long* __restrict__ offset,
                                                    int64_t* __restrict__ member, uint8_t* __restrict__ sign,
                                                    uint64_t cap_c) {
  __shared__ uint32_t wsum[256 / 64];
  const uint64_t i0 = (uint64_t)blockIdx.x * kCompTile + (uint64_t)threadIdx.x * kCompPer;
  unsigned long long key[kCompPer];
  uint32_t pay[kCompPer];
  const uint32_t heads = comp_load(s, n, i0, key, pay);
#pragma unroll
  for (uint32_t k = 0; k < kCompPer; ++k) {
    if (i0 + k < n && pay[k] < n) {  // (a payload is a row index)
      member[i0 + k] = v[pay[k]];
      if (sign) sign[i0 + k] = (sign_kind && !parity[pay[k]]) ? 1 : 0;  // parity 0 <=> the colour of the minimum
    }
  }
  const uint64_t first = bbase[blockIdx.x];
  uint64_t pos = first + block_excl_scan<256>((uint32_t)__popc(heads), wsum);
  uint32_t total = 0;
#pragma unroll
  for (uint32_t q = 0; q < 256 / 64; ++q) total += wsum[q];
#pragma unroll
  for (uint32_t k = 0; k < kCompPer; ++k) {
    if (heads & (1u << k)) {
      if (pos < cap_c) {
        comp[pos] = (int64_t)(key[k] ^ kSortSignBit);
        offset[pos] = i0 + k;
      }
      ++pos;
    }
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0 && first + total <= cap_c) offset[first + total] = n;
}

}  // namespace

void launch_sort_digits(const int64_t* v, const int64_t* label, uint64_t n, uint32_t* ctl, hipStream_t st) {
  const uint64_t tiles = (n + 256 * kDigitsPer - 1) / (256 * kDigitsPer);
  const uint32_t grid = (uint32_t)(tiles < 1024 ? (tiles ? tiles : 1) : 1024);
  hipLaunchKernelGGL(k_sort_digits, dim3(grid), dim3(256), 0, st, v, label, n, ctl);
}

void launch_sort_digits_one(const int64_t* key, uint64_t n, uint32_t* ctl, hipStream_t st) {
  const uint64_t tiles = (n + 256 * kDigitsPer - 1) / (256 * kDigitsPer);
  const uint32_t grid = (uint32_t)(tiles < kDigitsOneBlocks ? (tiles ? tiles : 1) : kDigitsOneBlocks);
  hipLaunchKernelGGL(k_sort_digits_one, dim3(grid), dim3(256), 0, st, key, n, ctl);
}

void launch_tile_scan(uint32_t* tb, uint64_t nt, unsigned long long* total, hipStream_t st) {
  hipLaunchKernelGGL(k_tile_scan, dim3(1), dim3(kSortScanBS), 0, st, tb, nt, total);
}

void launch_comp_roots(const int64_t* v, const int64_t* label, uint64_t n, unsigned long long* out, hipStream_t st) {
  const uint64_t tiles = (n + 255) / 256;
  const uint32_t grid = (uint32_t)(tiles < 2048 ? (tiles ? tiles : 1) : 2048);
  hipLaunchKernelGGL(k_comp_roots, dim3(grid), dim3(256), 0, st, v, label, n, out);
}

void launch_sort_pass(const SortSrc& src, uint64_t n, int pass, uint32_t* table, const uint32_t* ghist,
                      unsigned long long* okey, uint32_t* opay, hipStream_t st) {
  const uint64_t blocks = sort_blocks(n), stride = sort_row_stride(blocks);
  const int shift = 8 * pass;
  hipLaunchKernelGGL(k_sort_hist, dim3((uint32_t)blocks), dim3(kSortBS), 0, st, src, n, shift, table, stride);
  hipLaunchKernelGGL(k_sort_scan, dim3(kSortRadix), dim3(kSortScanBS), 0, st, table, blocks, stride, ghist);
  hipLaunchKernelGGL(k_sort_scatter, dim3((uint32_t)blocks), dim3(kSortBS), 0, st, src, n, shift, table, stride, okey,
                     opay);
}

void launch_comp_csr(const SortSrc& src, uint64_t n, const int64_t* v, const uint8_t* parity, bool sign_kind,
                     uint32_t* table, int64_t* comp, unsigned long long* offset, int64_t* member, uint8_t* sign,
                     uint64_t cap_c, hipStream_t st) {
  const uint64_t blocks = comp_blocks(n);
  hipLaunchKernelGGL(k_comp_heads, dim3((uint32_t)blocks), dim3(256), 0, st, src, n, table);
  hipLaunchKernelGGL(k_sort_scan, dim3(1), dim3(kSortScanBS), 0, st, table, blocks, sort_row_stride(blocks),
                     (const uint32_t*)nullptr);
  hipLaunchKernelGGL(k_comp_write, dim3((uint32_t)blocks), dim3(256), 0, st, src, n, table, v, parity,
                     sign_kind ? 1 : 0, comp, offset, member, sign, cap_c);
}

}  // namespace gs
