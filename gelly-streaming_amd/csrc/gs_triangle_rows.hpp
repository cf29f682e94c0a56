// gs_triangle_rows.hpp -- the row arithmetic of the triangle summary (gs_triangle_k.hip):
// row bounds, membership, the predecessor test of the once-only rule and the merge
// positions over an adjacency sorted by (x, y) in signed order. Plain functions of their
// arguments: the header compiles with a host compiler too (tests/cpp/triangle_rows_sanitize.cpp
// checks every function against brute force under the address and UB sanitizers).
//
// Every search halves a non-empty interval [lo, hi) of indices below n per step, so it ends
// after at most 64 steps and only reads indices in [0, n); n == 0 reads nothing.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GS_TRI_HD __host__ __device__ inline
#else
#define GS_TRI_HD inline
#endif

namespace gs {

constexpr uint64_t kTriNone = ~0ull;

// first index in [b, e) whose value is >= key (e when none); v ascending on [b, e)
GS_TRI_HD uint64_t tri_lower(const int64_t* v, uint64_t b, uint64_t e, int64_t key) {
  while (b < e) {
    const uint64_t mid = b + (e - b) / 2;
    if (v[mid] < key) b = mid + 1;
    else e = mid;
  }
  return b;
}

// first index in [b, e) whose value is > key (e when none)
GS_TRI_HD uint64_t tri_upper(const int64_t* v, uint64_t b, uint64_t e, int64_t key) {
  while (b < e) {
    const uint64_t mid = b + (e - b) / 2;
    if (v[mid] <= key) b = mid + 1;
    else e = mid;
  }
  return b;
}

// the row of `key` in the x column of n entries: [*b, *e), empty (b == e) when absent
GS_TRI_HD void tri_row(const int64_t* x, uint64_t n, int64_t key, uint64_t* b, uint64_t* e) {
  *b = tri_lower(x, 0, n, key);
  *e = tri_upper(x, *b, n, key);
}

// index of `key` in the ascending values v[b .. e), or kTriNone
GS_TRI_HD uint64_t tri_member(const int64_t* v, uint64_t b, uint64_t e, int64_t key) {
  const uint64_t p = tri_lower(v, b, e, key);
  return (p < e && v[p] == key) ? p : kTriNone;
}

GS_TRI_HD bool tri_pair_less(int64_t ax, int64_t ay, int64_t bx, int64_t by) {
  return ax < bx || (ax == bx && ay < by);
}

// entries of the n pairs (x, y), ascending by (x, y), that are < (kx, ky)
GS_TRI_HD uint64_t tri_pair_lower(const int64_t* x, const int64_t* y, uint64_t n, int64_t kx, int64_t ky) {
  uint64_t b = 0, e = n;
  while (b < e) {
    const uint64_t mid = b + (e - b) / 2;
    if (tri_pair_less(x[mid], y[mid], kx, ky)) b = mid + 1;
    else e = mid;
  }
  return b;
}

GS_TRI_HD bool tri_has_pair(const int64_t* x, const int64_t* y, uint64_t n, int64_t kx, int64_t ky) {
  const uint64_t p = tri_pair_lower(x, y, n, kx, ky);
  return p < n && x[p] == kx && y[p] == ky;
}

// index of the pair (kx, ky) among the n pairs ascending by (x, y), or kTriNone
GS_TRI_HD uint64_t tri_pair_at(const int64_t* x, const int64_t* y, uint64_t n, int64_t kx, int64_t ky) {
  const uint64_t p = tri_pair_lower(x, y, n, kx, ky);
  return (p < n && x[p] == kx && y[p] == ky) ? p : kTriNone;
}

// ---- removal (tests/cpp/triangle_removal_sanitize.cpp checks these against brute force)

// Is the stamp s at least `folds` folds behind the fold number cur (s + folds <= cur)? The age
// is a difference of 32 bits compared in 64: nothing can wrap. A stamp past cur has age 0.
GS_TRI_HD bool tri_is_old(uint32_t s, uint32_t cur, uint64_t folds) {
  const uint64_t age = s <= cur ? (uint64_t)(cur - s) : 0;
  return age >= folds;
}

// The stamp after the fold number wrapped: 2^31 lower, or 0 when it was older than that.
GS_TRI_HD uint32_t tri_rebase(uint32_t s) { return s >= 0x80000000u ? s - 0x80000000u : 0u; }

// pos[j] = survivors among the entries before j (j < n), live = survivors among all n. For
// the row head i (i < n, x[i - 1] != x[i]): does no entry of i's row survive? One search for
// the row's end inside [i, n); reads pos[i] and, when the row ends before n, pos[end].
GS_TRI_HD bool tri_row_gone(const int64_t* x, uint64_t n, uint64_t i, const uint32_t* pos, uint64_t live) {
  const uint64_t e = tri_upper(x, i, n, x[i]);
  const uint64_t pe = e < n ? (uint64_t)pos[e] : live;
  return pe == (uint64_t)pos[i];
}

// The predecessor test: does the edge of the directed entry (ex, ey) precede the canonical
// edge (u, v), u < v, in the order of canonical pairs (min, max)?
GS_TRI_HD bool tri_edge_before(int64_t ex, int64_t ey, int64_t u, int64_t v) {
  const int64_t a = ex < ey ? ex : ey, b = ex < ey ? ey : ex;
  return tri_pair_less(a, b, u, v);
}

// Position of an entry in the merge of three sorted pair lists without a common pair: its
// own index in its list plus the entries of the two other lists below it.
GS_TRI_HD uint64_t tri_merge_pos(uint64_t own_index, int64_t kx, int64_t ky, const int64_t* x1, const int64_t* y1,
                                 uint64_t n1, const int64_t* x2, const int64_t* y2, uint64_t n2) {
  return own_index + tri_pair_lower(x1, y1, n1, kx, ky) + tri_pair_lower(x2, y2, n2, kx, ky);
}

}  // namespace gs
