// gs_degree.cpp -- the degree summary (GS_KIND_DEGREE) behind include/gs_summary.h's
// gs_degree_* section: streaming vertex degrees (SimpleEdgeStream.getDegrees /
// getInDegrees / getOutDegrees) and the degree distribution (example/DegreeDistribution).
//
// The summary is the relabel table of every other kind with a signed 32-bit net count per
// vertex in the slot's link word (gs_degree.hpp). Capacity is tracked on the host the simple
// way: an upper bound of 2 new vertices per folded edge since the last exact count, and one
// synchronising read of the exact count (and a rebuild carrying the counts) when that bound
// crosses the load limit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "gs_degree.hpp"
#include "gs_internal.hpp"

using namespace gsi;

namespace {

// No counter may pass 2^31 - 1: the handle keeps the endpoint occurrences folded since reset
// (deletions included: they bound the negative side the same way) and refuses a call that
// would take the total past it.
constexpr uint64_t kDegreeMaxTotal = (1ull << 31) - 1;

int check_degree(gs_handle h) {
  if (!h) return fail(GS_ERR_INVALID, "null handle");
  if (h->kind != GS_KIND_DEGREE) return fail(GS_ERR_INVALID, "not a degree summary (gs_create kind 2)");
  ++h->api_calls;
  return GS_OK;
}

int fold_variant() {
  const int64_t v = testing_value(GS_TESTING_DEGREE_VARIANT, gs::kDegreeProduct);
  return v >= 0 && v < gs::kDegreeVariants ? (int)v : gs::kDegreeProduct;
}

int guard_total(const gs_summary* h, uint64_t add) {
  if (h->deg_total + add > kDegreeMaxTotal)
    return fail(GS_ERR_CAPACITY, "degree counters are 32-bit: " + std::to_string(h->deg_total) + " + " +
                                     std::to_string(add) + " endpoint occurrences would pass 2^31 - 1");
  return GS_OK;
}

// Room for n more elements (each may add 2 vertices) below the load limit.
int ensure_degree_capacity(gs_summary* h, uint64_t n) {
  const double limit = kMaxLoad * (double)h->cap;
  const uint64_t b = h->nv_exact + 2 * (h->e_launched - h->e_exact);
  if ((double)(b + 2 * n) <= limit) {
    h->nv_ub = b + 2 * n;
    h->e_launched += n;
    return GS_OK;
  }
  uint64_t nv = 0;
  h->cap_syncs++;
  if (int rc = read_nv(h, &nv)) return rc;
  if (int rc = check_flags_now(h)) return rc;
  exact_count(h, nv);
  if ((double)(nv + 2 * n) > limit) {
    uint64_t nc = h->cap;
    while (kMaxLoad * (double)nc < (double)(nv + 2 * n)) nc <<= 1;
    if (int rc = degree_grow(h, nc)) return rc;
  }
  h->nv_ub = h->nv_exact + 2 * n;
  h->e_launched += n;
  return GS_OK;
}

int launch_chunks(gs_summary* h, gs::DegreeLaunch f, uint64_t n, bool check_cap) {
  const int variant = fold_variant();
  const int64_t *src = f.src, *dst = f.dst, *wt = f.wt;
  const uint8_t* del = f.del;
  for (uint64_t off = 0; off < n; off += kMaxChunk) {
    const uint64_t c = std::min<uint64_t>(kMaxChunk, n - off);
    if (check_cap)
      if (int rc = ensure_degree_capacity(h, c)) return rc;
    f.src = src + off * f.stride;
    f.dst = dst ? dst + off * f.stride : nullptr;
    f.del = del ? del + off : nullptr;
    f.wt = wt ? wt + off : nullptr;
    f.n = (uint32_t)c;
    f.shard0 = h->shard0;
    h->shard0 = (h->shard0 + gs::degree_blocks(f.n, variant)) & (gs::kShards - 1);
    GS_LAUNCH(gs::launch_degree_fold(h->table(), f, variant, h->stream));
  }
  return GS_OK;
}

int fold_edges(gs_summary* h, const int64_t* src, const int64_t* dst, const uint8_t* del, uint64_t n, uint64_t stride,
               int dir) {
  gs::DegreeLaunch f;
  f.src = src;
  f.dst = dst;
  f.del = del;
  f.stride = (uint32_t)stride;
  f.dir = dir;
  return launch_chunks(h, f, n, true);
}

// wt[i] added to vertex v[i] (device arrays), every v inserted whatever its weight
int add_rows(gs_summary* h, const int64_t* v, const int64_t* wt, uint64_t n, bool check_cap) {
  gs::DegreeLaunch f;
  f.src = v;
  f.wt = wt;
  return launch_chunks(h, f, n, check_cap);
}

int fold_args(gs_handle h, const void* src, const void* dst, size_t n, int dir, uint64_t* occ) {
  if (n && (!src || !dst)) return fail(GS_ERR_INVALID, "null edge arrays");
  if (dir != gs::kDegreeAll && dir != gs::kDegreeIn && dir != gs::kDegreeOut)
    return fail(GS_ERR_INVALID, "unknown degree direction");
  if (n > kDegreeMaxTotal) return fail(GS_ERR_CAPACITY, "degree counters are 32-bit: too many edges in one call");
  *occ = (uint64_t)n * (dir == gs::kDegreeAll ? 2 : 1);
  return guard_total(h, *occ);
}

// Unordered rows (vertex, count as int64) of the summary in x_v / x_l: every table entry
// (all) or those with a count > 0. Synchronises; *n rows.
int gather_rows(gs_summary* h, bool all, uint64_t* n) {
  *n = 0;
  uint64_t nv = 0;
  if (int rc = read_nv(h, &nv)) return rc;
  if (int rc = check_flags_now(h)) return rc;
  exact_count(h, nv);
  if (nv == 0) return GS_OK;
  if (int rc = x_scratch(h, nv + 1)) return rc;
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(h->d_scratch.get());
  unsigned long long got = 0;
  GS_HIP(hipMemsetAsync(cnt, 0, 8, h->stream));
  GS_LAUNCH(gs::launch_degree_export(h->table(), h->x_v, h->x_l, h->x_cap, cnt, all, h->stream));
  GS_HIP(hipMemcpyAsync(&got, cnt, 8, hipMemcpyDeviceToHost, h->stream));
  GS_HIP(hipStreamSynchronize(h->stream));
  if (got > h->x_cap) return fail(GS_ERR_HIP, "degree export found more rows than the table's vertex count");
  *n = got;
  return GS_OK;
}

// Stable radix sort of n int64 ids (signed order) with the shared driver (gs_sort.cpp): on
// return `cur` names the sorted (key, row index) pairs -- key / pay null when no pass had to
// run (the input order is the sorted order) -- and *side the ping-pong buffer not holding them.
int sort_rows(gs_summary* h, const int64_t* ids, uint64_t n, gs::SortSrc* cur, int* side) {
  SortScratch& ss = h->sort;
  if (int rc = sort_scratch_ensure(ss, n, h->stream)) return rc;
  std::vector<uint32_t> ctl(gs::kSortCtlWords);
  GS_HIP(hipMemsetAsync(ss.ctl, 0, gs::kSortCtlWords * 4, h->stream));
  GS_LAUNCH(gs::launch_sort_digits(ids, ids, n, ss.ctl, h->stream));
  GS_HIP(hipMemcpyAsync(ctl.data(), ss.ctl, gs::kSortCtlWords * 4, hipMemcpyDeviceToHost, h->stream));
  GS_HIP(hipStreamSynchronize(h->stream));
  bool skip[gs::kSortPasses];
  sort_skip_digits(ctl.data(), n, skip);
  *cur = gs::SortSrc();
  *side = 0;
  return sort_run(ss, ids, n, ss.ctl, skip, cur, side, h->stream);
}

int export_impl(gs_summary* h, int64_t* v, int64_t* degree, size_t cap, size_t* n, int sorted, bool to_host) {
  *n = 0;
  if (int rc = join_lanes(h)) return rc;
  uint64_t rows = 0;
  if (int rc = gather_rows(h, false, &rows)) return rc;
  *n = rows;
  if (cap < rows) return truncated(cap, rows);
  if (rows == 0) return GS_OK;
  if (!v || !degree) return fail(GS_ERR_INVALID, "null arrays");
  const int64_t *rv = h->x_v, *rd = h->x_l;
  const hipMemcpyKind kind = to_host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
  if (sorted) {
    gs::SortSrc cur;
    int side = 0;
    if (int rc = sort_rows(h, h->x_v, rows, &cur, &side)) return rc;
    if (to_host) {
      if (int rc = comp_staging(h, rows, rows)) return rc;
      GS_LAUNCH(gs::launch_degree_gather(cur.pay, h->x_v, h->x_l, rows, h->co_member, h->co_comp, h->stream));
      rv = h->co_member;
      rd = h->co_comp;
    } else {
      GS_LAUNCH(gs::launch_degree_gather(cur.pay, h->x_v, h->x_l, rows, v, degree, h->stream));
      rv = rd = nullptr;
    }
  }
  if (rv) {
    GS_HIP(hipMemcpyAsync(v, rv, rows * 8, kind, h->stream));
    GS_HIP(hipMemcpyAsync(degree, rd, rows * 8, kind, h->stream));
  }
  GS_HIP(hipStreamSynchronize(h->stream));
  return GS_OK;
}

int distribution_impl(gs_summary* h, int64_t* degree, int64_t* count, size_t cap, size_t* n, bool to_host) {
  *n = 0;
  if (int rc = join_lanes(h)) return rc;
  uint64_t rows = 0;
  if (int rc = gather_rows(h, false, &rows)) return rc;
  if (rows == 0) return GS_OK;
  // sort the counts, take the heads: distinct degrees ascending and their run lengths
  gs::SortSrc cur;
  int side = 0;
  if (int rc = sort_rows(h, h->x_l, rows, &cur, &side)) return rc;
  unsigned long long nd = 1;  // no pass ran: every key equal
  if (cur.key) {
    unsigned long long* heads = reinterpret_cast<unsigned long long*>(h->d_scratch.get()) + 1;
    GS_HIP(hipMemsetAsync(heads, 0, 8, h->stream));
    GS_LAUNCH(gs::launch_degree_heads(cur.key, rows, heads, h->stream));
    GS_HIP(hipMemcpyAsync(&nd, heads, 8, hipMemcpyDeviceToHost, h->stream));
    GS_HIP(hipStreamSynchronize(h->stream));
  }
  *n = nd;
  if (cap < nd) return truncated(cap, nd);
  if (!degree || !count) return fail(GS_ERR_INVALID, "null arrays");
  if (int rc = comp_staging(h, rows, rows)) return rc;
  if (!cur.key) cur.ids = h->x_l;
  GS_LAUNCH(gs::launch_comp_csr(cur, rows, h->x_l, nullptr, false, h->sort.table, h->co_comp, h->co_off, h->co_member,
                                nullptr, h->co_ccap, h->stream));
  if (to_host) {
    // (the CSR's member column and the sort's free ping-pong buffer are dead by now)
    int64_t* sd = h->co_member;
    int64_t* sc = reinterpret_cast<int64_t*>(h->sort.key[side].get());
    GS_LAUNCH(gs::launch_degree_runs(h->co_comp, h->co_off, nd, sd, sc, h->stream));
    GS_HIP(hipMemcpyAsync(degree, sd, nd * 8, hipMemcpyDeviceToHost, h->stream));
    GS_HIP(hipMemcpyAsync(count, sc, nd * 8, hipMemcpyDeviceToHost, h->stream));
  } else {
    GS_LAUNCH(gs::launch_degree_runs(h->co_comp, h->co_off, nd, degree, count, h->stream));
  }
  GS_HIP(hipStreamSynchronize(h->stream));
  return GS_OK;
}

}  // namespace

namespace gsi {

// Rebuild into a table of new_cap slots carrying every entry's count (entries at <= 0 too).
int degree_grow(gs_summary* h, uint64_t new_cap) {
  if (new_cap > kMaxCap) return fail(GS_ERR_CAPACITY, "vertex table would exceed 2^30 slots");
  uint64_t nv = 0;
  if (int rc = read_nv(h, &nv)) return rc;
  DevBuf<int64_t> v, d;
  const size_t m = nv + 1;
  if (v.alloc(m) != hipSuccess || d.alloc(m) != hipSuccess)
    return fail(GS_ERR_HIP, "table rebuild: out of device memory");
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(h->d_scratch.get());
  unsigned long long got = 0;
  int rc = GS_OK;
  if (hipMemsetAsync(cnt, 0, 8, h->stream) != hipSuccess) rc = fail(GS_ERR_HIP, "table rebuild: memset failed");
  if (!rc) {
    gs::launch_degree_export(h->table(), v, d, m, cnt, true, h->stream);
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&got, cnt, 8, hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
        hipStreamSynchronize(h->stream) != hipSuccess)
      rc = fail(GS_ERR_HIP, "table rebuild: export failed");
  }
  if (!rc && got > m) rc = fail(GS_ERR_HIP, "table rebuild: more entries than the vertex count");
  if (!rc) rc = rebuild_table(h, new_cap);
  if (!rc) rc = add_rows(h, v, d, got, /*check_cap=*/false);
  if (!rc && hipStreamSynchronize(h->stream) != hipSuccess) rc = fail(GS_ERR_HIP, "table rebuild: sync failed");
  if (!rc) exact_count(h, got);
  return rc;
}

// dst += src (src unchanged): src's entries, those at <= 0 included, added as rows.
int degree_combine(gs_summary* dst, gs_summary* src) {
  if (int rc = guard_total(dst, src->deg_total)) return rc;
  uint64_t rows = 0;
  {
    DeviceGuard g(src->device);
    if (int rc = join_lanes(src)) return rc;
    if (int rc = gather_rows(src, true, &rows)) return rc;
  }
  DeviceGuard g(dst->device);
  if (int rc = join_lanes(dst)) return rc;
  const int64_t *rv = src->x_v, *rd = src->x_l;
  if (rows && dst->device != src->device) {
    if (int rc = x_scratch(dst, rows + 1)) return rc;
    GS_HIP(hipMemcpyPeerAsync(dst->x_v, dst->device, src->x_v, src->device, rows * 8, dst->stream));
    GS_HIP(hipMemcpyPeerAsync(dst->x_l, dst->device, src->x_l, src->device, rows * 8, dst->stream));
    rv = dst->x_v;
    rd = dst->x_l;
  }
  if (int rc = add_rows(dst, rv, rd, rows, true)) return rc;
  GS_HIP(hipStreamSynchronize(dst->stream));  // src's scratch is free again
  dst->deg_total += src->deg_total;
  return check_flags_now(dst);
}

// Image: u32 magic 'GSS1', u32 kind (2), u32 1, u32 endpoint-occurrence total, u64 n,
// int64 v[n], int64 count[n], u8 0[n] -- the layout of the other kinds' image.
int degree_serialize(gs_summary* h, void* buf, size_t cap, size_t* len) {
  DeviceGuard g(h->device);
  if (int rc = join_lanes(h)) return rc;
  uint64_t nv = 0;
  if (int rc = read_nv(h, &nv)) return rc;
  *len = 24 + nv * 17;
  if (!buf) return GS_OK;
  if (cap < *len) return fail(GS_ERR_TRUNCATED, "buffer too small");
  uint64_t rows = 0;
  if (int rc = gather_rows(h, true, &rows)) return rc;
  uint8_t* b = static_cast<uint8_t*>(buf);
  const uint32_t hdr[4] = {0x31535347u, (uint32_t)h->kind, 1u, (uint32_t)h->deg_total};
  memcpy(b, hdr, 16);
  memcpy(b + 16, &rows, 8);
  if (rows) {
    GS_HIP(hipMemcpy(b + 24, h->x_v, rows * 8, hipMemcpyDeviceToHost));
    GS_HIP(hipMemcpy(b + 24 + rows * 8, h->x_l, rows * 8, hipMemcpyDeviceToHost));
    memset(b + 24 + rows * 16, 0, rows);
  }
  *len = 24 + rows * 17;
  return GS_OK;
}

// after the caller validated magic, kind and length and reset the summary
int degree_deserialize(gs_summary* h, const void* buf, uint64_t n, uint32_t total) {
  if ((uint64_t)total > kDegreeMaxTotal) return fail(GS_ERR_INVALID, "image total out of range");
  DeviceGuard g(h->device);
  const uint8_t* b = static_cast<const uint8_t*>(buf);
  if (n) {
    if (int rc = x_scratch(h, n + 1)) return rc;
    GS_HIP(hipMemcpyAsync(h->x_v, b + 24, n * 8, hipMemcpyHostToDevice, h->stream));
    GS_HIP(hipMemcpyAsync(h->x_l, b + 24 + n * 8, n * 8, hipMemcpyHostToDevice, h->stream));
    if (int rc = add_rows(h, h->x_v, h->x_l, n, true)) return rc;
  }
  h->deg_total = total;
  if (int rc = join_lanes(h)) return rc;
  return check_device_flags(h);
}

}  // namespace gsi

extern "C" {

int gs_degree_fold_device(gs_handle h, const int64_t* src, const int64_t* dst, const uint8_t* del, size_t n,
                          size_t stride, int dir) {
  if (int rc = check_degree(h)) return rc;
  if (stride == 0 || stride > 0xFFFFFFFFull) return fail(GS_ERR_INVALID, "stride must be >= 1");
  uint64_t occ = 0;
  if (int rc = fold_args(h, src, dst, n, dir, &occ)) return rc;
  DeviceGuard g(h->device);
  if (int rc = join_lanes(h)) return rc;
  h->deg_total += occ;
  return fold_edges(h, src, dst, del, n, stride, dir);
}

// Host edges in chunks of up to 2^20 through the handle's device staging; the caller may
// reuse its arrays when the call returns.
int gs_degree_fold(gs_handle h, const int64_t* src, const int64_t* dst, const uint8_t* del, size_t n, int dir) {
  if (int rc = check_degree(h)) return rc;
  uint64_t occ = 0;
  if (int rc = fold_args(h, src, dst, n, dir, &occ)) return rc;
  if (n == 0) return GS_OK;
  DeviceGuard g(h->device);
  if (int rc = join_lanes(h)) return rc;
  if (int rc = dev_stage(h, std::min<size_t>(n, kStageChunk))) return rc;
  h->deg_total += occ;
  const size_t sc = h->d_stage_chunk;
  for (size_t off = 0; off < n; off += kStageChunk) {
    const size_t c = std::min<size_t>(kStageChunk, n - off);
    const int b = h->stage_next;
    h->stage_next ^= 1;
    int64_t* ds = h->d_stage + (size_t)b * 2 * sc;
    uint8_t* dd = del ? h->d_wstage + (size_t)b * sc : nullptr;
    GS_HIP(hipMemcpyAsync(ds, src + off, c * 8, hipMemcpyHostToDevice, h->stream));
    GS_HIP(hipMemcpyAsync(ds + sc, dst + off, c * 8, hipMemcpyHostToDevice, h->stream));
    if (del) GS_HIP(hipMemcpyAsync(dd, del + off, c, hipMemcpyHostToDevice, h->stream));
    if (int rc = fold_edges(h, ds, ds + sc, dd, c, 1, dir)) return rc;
  }
  GS_HIP(hipStreamSynchronize(h->stream));
  return GS_OK;
}

int gs_degree_find_device(gs_handle h, const int64_t* v, size_t n, int64_t* degree, uint8_t* found) {
  if (int rc = check_degree(h)) return rc;
  if (n && (!v || !degree)) return fail(GS_ERR_INVALID, "null arrays");
  DeviceGuard g(h->device);
  if (int rc = join_lanes(h)) return rc;
  GS_LAUNCH(gs::launch_degree_find(h->table(), v, n, degree, found, h->stream));
  return GS_OK;
}

int gs_degree_export_device(gs_handle h, int64_t* v, int64_t* degree, size_t cap, size_t* n, int sorted) {
  if (int rc = check_degree(h)) return rc;
  if (!n) return fail(GS_ERR_INVALID, "n is null");
  DeviceGuard g(h->device);
  return export_impl(h, v, degree, cap, n, sorted, false);
}

int gs_degree_export(gs_handle h, int64_t* v, int64_t* degree, size_t cap, size_t* n, int sorted) {
  if (int rc = check_degree(h)) return rc;
  if (!n) return fail(GS_ERR_INVALID, "n is null");
  DeviceGuard g(h->device);
  return export_impl(h, v, degree, cap, n, sorted, true);
}

int gs_degree_distribution_device(gs_handle h, int64_t* degree, int64_t* count, size_t cap, size_t* n) {
  if (int rc = check_degree(h)) return rc;
  if (!n) return fail(GS_ERR_INVALID, "n is null");
  DeviceGuard g(h->device);
  return distribution_impl(h, degree, count, cap, n, false);
}

int gs_degree_distribution(gs_handle h, int64_t* degree, int64_t* count, size_t cap, size_t* n) {
  if (int rc = check_degree(h)) return rc;
  if (!n) return fail(GS_ERR_INVALID, "n is null");
  DeviceGuard g(h->device);
  return distribution_impl(h, degree, count, cap, n, true);
}

}  // extern "C"
