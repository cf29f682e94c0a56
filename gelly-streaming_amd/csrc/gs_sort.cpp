// gs_sort.cpp -- the host side of the radix sort (gs_sort.hpp, kernels in gs_sort_k.hip): the
// owner of its scratch, the one loop that queues its passes (sort_run: the component export of
// gs_capi.cpp, the degree exports of gs_degree.cpp and step 3 of the triangle fold call it
// themselves) and the two whole sorts built on it: sort_by_pair (the triangle, spanner and
// triangle streams' folds) and sort_by_key (the window slices, the distinct and matching exports,
// the sampling triangle estimate, the degree and triangle streams' folds).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gs_internal.hpp"

namespace gsi {

int sort_scratch_ensure(SortScratch& s, uint64_t rows, hipStream_t st) {
  if (!s.ctl) GS_HIP(s.ctl.alloc(gs::kSortCtlWords));
  if (s.rows >= rows) return GS_OK;
  GS_HIP(hipStreamSynchronize(st));
  s.rows = 0;
  for (int i = 0; i < 2; ++i) {
    s.key[i].reset();
    s.pay[i].reset();
  }
  s.table.reset();
  const uint64_t c = gs::sort_blocks(rows + rows / 4) * gs::kSortTile;
  for (int i = 0; i < 2; ++i) {
    GS_HIP(s.key[i].alloc(c));
    GS_HIP(s.pay[i].alloc(c));
  }
  GS_HIP(s.table.alloc(gs::kSortRadix * gs::sort_row_stride(gs::sort_blocks(c))));
  s.rows = c;
  return GS_OK;
}

void sort_skip_digits(const uint32_t* hist, uint64_t n, bool skip[gs::kSortPasses]) {
  for (int p = 0; p < (int)gs::kSortPasses; ++p) {
    const uint32_t* gh = hist + p * gs::kSortRadix;
    skip[p] = *std::max_element(gh, gh + gs::kSortRadix) == n;
  }
}

int sort_run(SortScratch& s, const int64_t* ids, uint64_t n, const uint32_t* hist, const bool* skip, gs::SortSrc* cur,
             int* side, hipStream_t st) {
  cur->key = nullptr;
  cur->ids = ids;
  cur->rows = n;
  for (int p = 0; p < (int)gs::kSortPasses; ++p) {
    if (skip && skip[p]) continue;
    GS_LAUNCH(gs::launch_sort_pass(*cur, n, p, s.table, hist + p * gs::kSortRadix, s.key[*side], s.pay[*side], st));
    cur->key = s.key[*side];
    cur->pay = s.pay[*side];
    cur->ids = nullptr;
    *side ^= 1;
  }
  return GS_OK;
}

int sort_by_pair(SortScratch& s, const int64_t* x, const int64_t* y, uint64_t n, gs::SortSrc* cur, hipStream_t st) {
  GS_HIP(hipMemsetAsync(s.ctl, 0, gs::kSortCtlWords * 4, st));
  GS_LAUNCH(gs::launch_sort_digits(x, y, n, s.ctl, st));
  *cur = gs::SortSrc();
  int side = 0;
  if (int rc = sort_run(s, y, n, s.hist(1), nullptr, cur, &side, st)) return rc;
  return sort_run(s, x, n, s.hist(0), nullptr, cur, &side, st);
}

int sort_by_key(SortScratch& s, const int64_t* key, uint64_t n, const bool* skip, gs::SortSrc* cur, hipStream_t st,
                const char* what) {
  GS_HIP(hipMemsetAsync(s.ctl, 0, gs::kSortCtlWords * 4, st));
  GS_LAUNCH(gs::launch_sort_digits_one(key, n, s.ctl, st));
  *cur = gs::SortSrc();  // (pay null: payload i of key i is i)
  int side = 0;
  if (int rc = sort_run(s, key, n, s.hist(0), skip, cur, &side, st)) return rc;
  if (!cur->key || !cur->pay) return fail(GS_ERR_HIP, std::string(what) + ": the sort ran no pass");
  return GS_OK;
}

}  // namespace gsi
