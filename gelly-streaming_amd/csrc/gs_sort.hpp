// gs_sort.hpp -- host-side launchers of the grouped component export's kernels
// (gs_sort_k.hip): a stable LSD radix sort of (uint64 key, uint32 payload) pairs with
// 8-bit digits, and the tail that turns rows sorted by (label, vertex) into the CSR of
// gs_export_components*; beside them the two launches every summary with a sort or a compaction
// shares: the one-column digit histogram and the scan of tile counts (the device side of the
// flag / scan / compact idiom is gs_scan.hpp). Every launch is queued on the given stream; kernel boundaries
// carry all ordering between workgroups (no workgroup waits on another inside a launch).
// The host part at the end (gs_sort.cpp) owns the sort's scratch and drives its passes for
// every caller: the component export, the degree exports and step 3 of the triangle fold drive
// sort_run themselves (they read the histograms back for sort_skip_digits); the triangle, spanner
// and triangle streams' folds sort pairs through sort_by_pair; the window slices, the distinct and
// matching exports, the sampling triangle estimate and the degree and triangle streams' folds
// sort one column through sort_by_key.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gs_devbuf.hpp"

namespace gs {

constexpr uint32_t kSortBS = 256;                         // threads of a hist / scatter workgroup
constexpr uint32_t kSortItems = 8;                        // pairs per thread
constexpr uint32_t kSortTile = kSortBS * kSortItems;      // pairs per workgroup (gs_sort_tile)
constexpr uint32_t kSortRadix = 256;                      // 8-bit digits
constexpr uint32_t kSortPasses = 8;                       // digits of a 64-bit key
constexpr uint32_t kSortScanBS = 1024;                    // threads of a k_sort_scan (4 entries each) / k_tile_scan
                                                          // (one tile count each) workgroup: gsamd.TILE_SCAN_BLOCK
constexpr uint32_t kCompTile = 1024;                      // rows per k_comp_heads / k_comp_write workgroup
constexpr unsigned long long kSortSignBit = 1ull << 63;   // key = id ^ sign bit: unsigned digit order = signed order

// Control words (uint32): the digit histograms of the whole input, one 256-bin row per
// (sort, pass) -- sort 0 keyed by vertex, sort 1 by label -- then the count of roots.
constexpr uint32_t kSortCtlRoots = 2 * kSortPasses * kSortRadix;
constexpr uint32_t kSortCtlWords = kSortCtlRoots + 4;

__host__ __device__ constexpr uint64_t sort_blocks(uint64_t n) { return (n + kSortTile - 1) / kSortTile; }
// row stride of the per-workgroup histogram table (digit-major; 16-B aligned rows)
__host__ __device__ constexpr uint64_t sort_row_stride(uint64_t blocks) { return (blocks + 3) & ~3ull; }
__host__ __device__ constexpr uint64_t comp_blocks(uint64_t n) { return (n + kCompTile - 1) / kCompTile; }

// Where a pass reads its pairs. pay == nullptr: payload i of pair i is i. key == nullptr:
// the key is ids[payload] ^ kSortSignBit (the first pass of a sort gathers its keys from the
// exported rows: vertices for sort 1, labels through sort 1's permutation for sort 2).
struct SortSrc {
  const unsigned long long* key = nullptr;
  const uint32_t* pay = nullptr;
  const int64_t* ids = nullptr;
  uint64_t rows = 0;  // entries of ids (a payload is a row index below it)
};

// ctl[0 .. kSortCtlRoots) += digit histograms of v (rows 0..7) and label (rows 8..15);
// ctl[kSortCtlRoots] += rows with v == label. ctl must be zero before.
void launch_sort_digits(const int64_t* v, const int64_t* label, uint64_t n, uint32_t* ctl, hipStream_t st);
// ctl[0 .. 8 * 256) += the digit histograms of one key column (rows 0..7 of the control words,
// the `hist` of sort_run); ctl must be zero before. launch_sort_digits builds two columns, and
// every workgroup of either ends with one global add per bin.
void launch_sort_digits_one(const int64_t* key, uint64_t n, uint32_t* ctl, hipStream_t st);
// The scan step of a flag / scan / compact pass (gs_scan.hpp), one workgroup: the tile counts
// tb[0 .. nt) become their exclusive scan, tb[nt] = *total = their sum (below 2^32).
void launch_tile_scan(uint32_t* tb, uint64_t nt, unsigned long long* total, hipStream_t st);
// rows with v == label added into *out (gs_num_components)
void launch_comp_roots(const int64_t* v, const int64_t* label, uint64_t n, unsigned long long* out, hipStream_t st);

// One pass over digit `pass` (bits 8*pass .. 8*pass+7): table[digit * stride + workgroup]
// counts, their exclusive scan in (digit, workgroup) order from the digit's global base
// (ghist: the 256-bin row of this pass in ctl), the stable scatter into (okey, opay).
void launch_sort_pass(const SortSrc& src, uint64_t n, int pass, uint32_t* table, const uint32_t* ghist,
                      unsigned long long* okey, uint32_t* opay, hipStream_t st);

// Tail over rows sorted by (label, vertex): src gives label key and row index of position i.
// member[i] = v[row], sign[i] = !parity[row] (signed kind) or 0, comp / offset = the heads
// (label differs from the position before) in order; offset[number of heads] = n. `table`
// holds comp_blocks(n) words of scratch. Writes are bounded by cap_c heads.
void launch_comp_csr(const SortSrc& src, uint64_t n, const int64_t* v, const uint8_t* parity, bool sign_kind,
                     uint32_t* table, int64_t* comp, unsigned long long* offset, int64_t* member, uint8_t* sign,
                     uint64_t cap_c, hipStream_t st);

}  // namespace gs

// ---- host only (gs_sort.cpp) ----
namespace gsi {

// The sort's scratch: ping-pong (key, payload) buffers, the per-workgroup histogram table
// (also the tile scratch of launch_comp_csr) and the control words of launch_sort_digits.
struct SortScratch {
  DevBuf<unsigned long long> key[2];
  DevBuf<uint32_t> pay[2];
  DevBuf<uint32_t> table;
  DevBuf<uint32_t> ctl;  // gs::kSortCtlWords, allocated on first use
  uint64_t rows = 0;     // pairs key / pay hold (0 while they are not all allocated)
  // the eight 256-bin histogram rows of key column `col` in ctl: launch_sort_digits fills
  // column 0 (its first key) and column 1 (its second), launch_sort_digits_one column 0
  uint32_t* hist(int col) const { return ctl + (size_t)col * gs::kSortPasses * gs::kSortRadix; }
};

// Scratch for `rows` pairs: allocated on growth only, with a quarter of headroom rounded up
// to whole tiles. Synchronises st before it frees.
int sort_scratch_ensure(SortScratch& s, uint64_t rows, hipStream_t st);

// skip[p] = every one of the n keys agrees on digit p (its 256-bin row of `hist`, a host copy
// of eight rows, has one bin holding n): the pass would be an identity.
void sort_skip_digits(const uint32_t* hist, uint64_t n, bool skip[gs::kSortPasses]);
// The same from a host-known bound, with no histogram read back: every key is below `bound`, so
// the digits above the bits of `bound` itself are zero in all of them. bound == 0: nothing is
// known, no pass is skipped. Pass 0 always runs (sort_by_key needs one pass).
inline void sort_skip_above(uint64_t bound, bool skip[gs::kSortPasses]) {
  for (int p = 0; p < (int)gs::kSortPasses; ++p) skip[p] = bound != 0 && p > 0 && (bound >> (8 * p)) == 0;
}

// Stable radix passes on st over the digits of ids[payload] ^ kSortSignBit that `skip` (may be
// null: none) does not mark. hist: the device address of the eight 256-bin rows of those keys.
// Continues from *cur / *side: the payloads of an earlier sort carry over (a chained sort by a
// second key). On return *cur names the sorted (key, payload) pairs -- key null when no pass
// ran, the order is then *cur's order on entry -- and *side the buffer not holding them.
int sort_run(SortScratch& s, const int64_t* ids, uint64_t n, const uint32_t* hist, const bool* skip, gs::SortSrc* cur,
             int* side, hipStream_t st);

// The n pairs (x[i], y[i]) ordered by (x, y) on st: zeroes the control words, builds the digit
// histograms of both columns, sorts by y and then stably by x, no digit skipped (the histograms
// stay on the device). *cur names the sorted pairs, its payloads the pairs' indices. s.hist(0)
// and s.hist(1) hold the histograms of x and y afterwards, for a caller that reads them back.
int sort_by_pair(SortScratch& s, const int64_t* x, const int64_t* y, uint64_t n, gs::SortSrc* cur, hipStream_t st);

// The n keys key[i] in stable ascending order on st: zeroes the control words, builds the digit
// histograms of the column (launch_sort_digits_one), runs the passes `skip` (may be null: none)
// does not mark. *cur names the sorted pairs, its payloads the keys' indices. GS_ERR_HIP
// "<what>: the sort ran no pass" if skip marks all eight: the callers need the sorted keys.
int sort_by_key(SortScratch& s, const int64_t* key, uint64_t n, const bool* skip, gs::SortSrc* cur, hipStream_t st,
                const char* what);

}  // namespace gsi
