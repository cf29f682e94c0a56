// gs_degstream.cpp -- the degree streams behind include/gs_summary.h's gs_degstream_* section:
// every running degree of SimpleEdgeStream.getDegrees / getInDegrees / getOutDegrees and every
// (degree, count) record of example/DegreeDistribution.java. State layout and kernels are
// described in gs_degstream.hpp / gs_degstream_k.hip, the rules and the exactness argument in
// gs_degstream_seq.hpp (ds_fold_seq, ds_fold_parts) and DESIGN.md section 6i.
//
// A fold of n edges: growth of the vertex table is decided first from host-known totals, so
// nothing grows inside the vertex phase; the distinct streams' vertex phase
// (launch_dist_vertices) gives every new id its rank; the occurrences are keyed by rank and
// sorted stably (the digits above the largest possible rank are skipped); the clamped segmented
// scan writes (old, new) per occurrence and the degrees; the records are counted per tile and
// the counts scanned; the fold's one wait reads the new vertices, the record count, the largest
// new degree and the error word. Then the count array grows if the largest degree asks for it,
// the records are written in arrival order, sorted stably by degree, and the seeded segmented
// sum writes every record's count. That tail is queued, not waited for.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "gs_degstream.hpp"
#include "gs_internal.hpp"
#include "gs_vtable.hpp"

using namespace gsi;

struct gs_degstream_s : StreamOwner, VertexTable {  // (the vertex table and the vertices in rank order)
  int dir = gs::kDsAll;
  DevBuf<unsigned long long> ctl;   // gs::DsCtl words
  DevBuf<unsigned long long> dctl;  // gs::DistCtl words of the vertex phase
  DevBuf<uint32_t> degree;          // [dist_vid_cap(vcap)] the degree of every rank
  DevBuf<uint32_t> count;           // [count_cap] vertices per degree
  uint64_t count_cap = 0;
  // fold scratch for n_cap edges: the vertex phase's, then one row per occurrence (2 n_cap)
  uint64_t n_cap = 0;
  DevBuf<uint32_t> vslot, entry;  // [2 n]
  DevBuf<uint8_t> flags;          // whole tiles of 2 n positions
  DevBuf<uint32_t> tbase;         // [tiles + 1]: the vertex phase's tile counts, then the records', then an export's
  DevBuf<int64_t> key, row_v;
  DevBuf<int8_t> sgn;
  DevBuf<uint32_t> row_old, row_new;
  // the records of the last fold
  uint64_t r_cap = 0;
  DevBuf<uint32_t> r_occ, r_deg, r_cnt;
  DevBuf<int64_t> r_key;
  DevBuf<int8_t> r_delta;
  // the scans' tile scratch for s_tiles tiles
  uint64_t s_tiles = 0;
  DevBuf<gs::DsSeg> agg, carry;
  DevBuf<uint32_t> late_idx, late_val;
  SortScratch sort;
  // device staging of a host fold
  FoldStage stage;  // (src, dst) and the deletion bytes
  // state exports: tile counts, staging of the host-array form
  uint64_t x_tiles = 0;
  DevBuf<uint32_t> x_blk;
  OutStage out;  // two columns
  // host-known totals (nv: VertexTable)
  uint64_t total = 0, max_degree = 0;
  uint64_t last_nv = 0, last_occ = 0, last_rec = 0;
  bool kept = true;  // false after a fold the library cut into pieces
  uint64_t last_tiles = 0, growths = 0;
  // gs_testing_degstream_tune (profile) and the last profiled fold's phases
  bool profile = false;
  uint64_t phase_us[5] = {0, 0, 0, 0, 0};
};

namespace {

constexpr const char* kWhat = "degstream";  // check_handle: "null degstream handle"

// The vertex table grows (VertexTable::grow) and the degrees with it, inside the same wait.
int grow_vertices(gs_degstream_s* d, uint64_t cap) { return d->grow_ranked(cap, d->dctl, d->stream, d->degree); }

// count[] holds degrees 0 .. max_degree; the old counts move over
int grow_counts(gs_degstream_s* d, uint64_t max_degree) {
  if (d->count_cap > max_degree) return GS_OK;
  const uint64_t cap = gs::ds_count_cap(max_degree, gs::kDsMinCounts);
  DevBuf<uint32_t> c;
  GS_HIP(c.alloc(cap));
  GS_HIP(hipMemsetAsync(c, 0, cap * 4, d->stream));
  if (d->count_cap) {
    GS_HIP(hipMemcpyAsync(c, d->count, d->count_cap * 4, hipMemcpyDeviceToDevice, d->stream));
    GS_HIP(hipStreamSynchronize(d->stream));  // before the old array is freed
    ++d->growths;
  }
  d->count.swap(c);
  d->count_cap = cap;
  return GS_OK;
}

int ensure_tiles(gs_degstream_s* d, uint64_t rows) {
  const uint64_t tiles = gs::ds_tiles(rows, gs::DEGSTREAM_TILE);
  GS_HIP(grow_group(d->stream, d->s_tiles, tiles, tiles + tiles / 4 + 1, [&](uint64_t c) {
    return alloc_each(c, d->agg, d->carry, d->late_idx, d->late_val);
  }));
  return GS_OK;
}

int ensure_scratch(gs_degstream_s* d, uint64_t n) {
  static_assert(gs::DEGSTREAM_TILE == gs::DISTINCT_TILE, "tbase serves both compactions: 2 n / 2048 tiles");
  const auto alloc_scratch = [&](uint64_t c) {
    const uint64_t tiles = gs::dist_tiles(2 * c, gs::DISTINCT_TILE);
    hipError_t e = alloc_each(2 * c, d->vslot, d->entry, d->key, d->row_v, d->sgn, d->row_old, d->row_new);
    if (e == hipSuccess) e = d->flags.alloc(tiles * gs::DISTINCT_TILE);
    if (e == hipSuccess) e = d->tbase.alloc(tiles + 1);
    return e;
  };
  GS_HIP(grow_group(d->stream, d->n_cap, n, std::min<uint64_t>(gs::kDsMaxFold, n + n / 4), alloc_scratch));
  return GS_OK;
}

int ensure_records(gs_degstream_s* d, uint64_t rows) {
  GS_HIP(grow_group(d->stream, d->r_cap, rows, rows + rows / 4, [&](uint64_t c) {
    return alloc_each(c, d->r_occ, d->r_deg, d->r_cnt, d->r_key, d->r_delta);
  }));
  return GS_OK;
}

void forget_last(gs_degstream_s* d) {
  d->last_nv = d->last_occ = d->last_rec = d->last_tiles = 0;
  d->kept = true;
  for (uint64_t& us : d->phase_us) us = 0;
}

int fold_guard(gs_degstream_s* d, const void* src, const void* dst, size_t n) {
  if (int rc = check_handle(d, kWhat)) return rc;
  if (n && (!src || !dst)) return fail(GS_ERR_INVALID, "null edge arrays");
  const uint64_t occs = gs::ds_occurrences(n, d->dir);
  if ((uint64_t)n > gs::kDsMaxTotal || d->total + occs > gs::kDsMaxTotal)
    return fail(GS_ERR_CAPACITY, "degstream fold: " + std::to_string(d->total) + " + " + std::to_string(occs) +
                                     " endpoint occurrences pass 2^31 - 1 since the last reset");
  return d->fold_guard_vertices(n, std::min<uint64_t>(n, gs::kDsMaxFold), kWhat);
}

// 0 < n <= kDsMaxFold device edges on d->stream
int fold_piece(gs_degstream_s* d, const int64_t* src, const int64_t* dst, const uint8_t* del, uint64_t n,
               uint64_t stride) {
  hipStream_t st = d->stream;
  const uint64_t occs = gs::ds_occurrences(n, d->dir);
  if (int rc = d->ensure_for(n, [&](uint64_t slots) { return grow_vertices(d, slots); })) return rc;
  if (int rc = ensure_scratch(d, n)) return rc;
  if (int rc = ensure_tiles(d, occs)) return rc;
  if (int rc = sort_scratch_ensure(d->sort, occs, st)) return rc;
  const gs::DistVTable vt = d->vtable();
  const uint64_t ranks = gs::dist_vid_cap(d->vcap);
  // ranks: only collected endpoints are looked up or inserted, so IN and OUT hand the vertex
  // phase their one array as both endpoints
  const int64_t* ea = d->dir == gs::kDsIn ? dst : src;
  const int64_t* eb = d->dir == gs::kDsOut ? src : dst;
  // phases: ranks and keys | sort by rank | clamped scan, record counts and the wait | record rows
  // and sort by degree | seeded sum
  PhaseTimer timer(st, d->profile, d->phase_us, 5);
  timer.mark(0);
  GS_HIP(hipMemsetAsync(d->dctl, 0, gs::DIST_CTL_WORDS * 8, st));
  GS_HIP(hipMemsetAsync(d->ctl, 0, gs::DS_CTL_WORDS * 8, st));
  GS_LAUNCH(gs::launch_dist_vertices(ea, eb, n, stride, vt, d->vslot, d->flags, d->tbase, d->nv, d->vid, ranks, d->entry,
                                     d->dctl, st));
  GS_LAUNCH(gs::launch_ds_keys(src, dst, del, n, stride, d->dir, vt, d->vslot, ranks, d->key, d->sgn, d->row_v, d->ctl,
                               st));
  timer.mark(1);
  // every key is a rank below the bound, every record key a degree below its own: the digits
  // above a bound's bits are skipped (neither bound is 0, which would skip none: n > 0 gives
  // dist_worst_vertices(n) > 0, and max_degree + 1 > 0)
  gs::SortSrc cur;
  bool skip[gs::kSortPasses];
  sort_skip_above(d->nv + gs::dist_worst_vertices(n), skip);
  if (int rc = sort_by_key(d->sort, d->key, occs, skip, &cur, st, "degstream fold")) return rc;
  timer.mark(2);
  GS_LAUNCH(gs::launch_ds_seg_pass(cur.key, cur.pay, d->sgn, occs, true, d->degree, ranks, d->agg, d->carry,
                                   d->late_idx, d->late_val, d->row_old, d->row_new, d->ctl, d->ctl + gs::DS_MAX, st));
  const uint64_t nt = gs::ds_tiles(occs, gs::DEGSTREAM_TILE);
  GS_LAUNCH(gs::launch_ds_rec_count(d->row_old, d->row_new, d->sgn, occs, d->tbase, st));
  GS_LAUNCH(gs::launch_tile_scan(d->tbase, nt, d->ctl + gs::DS_RECORDS, st));
  // the fold's one host synchronisation
  unsigned long long c[gs::DS_CTL_WORDS], v[gs::DIST_CTL_WORDS];
  GS_HIP(hipMemcpyAsync(c, d->ctl, sizeof(c), hipMemcpyDeviceToHost, st));
  GS_HIP(hipMemcpyAsync(v, d->dctl, sizeof(v), hipMemcpyDeviceToHost, st));
  timer.mark(3);
  GS_HIP(hipStreamSynchronize(st));
  if (v[gs::DIST_OVERFLOW]) return fail(GS_ERR_HIP, "degstream fold: the vertex table overflowed (the handle's state is undefined)");
  if (c[gs::DS_ERR]) return fail(GS_ERR_HIP, "degstream fold: a rank or row index out of range (the handle's state is undefined)");
  if (v[gs::DIST_NEW_V] > 2 * n || c[gs::DS_RECORDS] > 2 * occs || c[gs::DS_MAX] > d->total + occs)
    return fail(GS_ERR_HIP, "degstream fold: counts out of range");
  d->nv += v[gs::DIST_NEW_V];
  d->total += occs;
  d->max_degree = std::max<uint64_t>(d->max_degree, c[gs::DS_MAX]);
  d->last_nv = v[gs::DIST_NEW_V];
  d->last_occ = occs;
  d->last_rec = c[gs::DS_RECORDS];
  d->last_tiles = nt;
  const uint64_t recs = d->last_rec;
  if (recs == 0) {
    timer.finish();
    return GS_OK;
  }
  // records: written in arrival order, sorted by degree, summed from the stored counts
  if (int rc = grow_counts(d, d->max_degree)) return rc;
  if (int rc = ensure_records(d, recs)) return rc;
  if (int rc = ensure_tiles(d, recs)) return rc;
  if (int rc = sort_scratch_ensure(d->sort, recs, st)) return rc;
  GS_LAUNCH(gs::launch_ds_rec_write(d->row_old, d->row_new, d->sgn, occs, d->tbase, d->r_occ, d->r_key, d->r_deg,
                                    d->r_delta, recs, d->ctl, st));
  sort_skip_above(d->max_degree + 1, skip);
  if (int rc = sort_by_key(d->sort, d->r_key, recs, skip, &cur, st, "degstream fold")) return rc;
  timer.mark(4);
  GS_LAUNCH(gs::launch_ds_seg_pass(cur.key, cur.pay, d->r_delta, recs, false, d->count, d->count_cap, d->agg, d->carry,
                                   d->late_idx, d->late_val, nullptr, d->r_cnt, d->ctl, nullptr, st));
  timer.mark(5);
  timer.finish();
  return GS_OK;
}

// the whole fold, cut into pieces of at most kDsMaxFold edges; host: the arrays are HOST arrays
int fold_all(gs_degstream_s* d, const int64_t* src, const int64_t* dst, const uint8_t* del, size_t n, uint64_t stride,
             bool host) {
  forget_last(d);
  if (n == 0) return GS_OK;
  DeviceGuard g(d->device);
  uint64_t sum[3] = {0, 0, 0};
  for (uint64_t at = 0; at < n; at += gs::kDsMaxFold) {
    const uint64_t len = std::min<uint64_t>(gs::kDsMaxFold, n - at);
    const int64_t* col[2] = {src + at * stride, dst + at * stride};
    const uint8_t* pe = del ? del + at : nullptr;
    if (host) GS_HIP(d->stage.put(d->stream, len, gs::kDsMaxFold, col, &pe));
    if (int rc = fold_piece(d, col[0], col[1], pe, len, host ? 1 : stride)) return rc;
    sum[0] += d->last_nv;
    sum[1] += d->last_occ;
    sum[2] += d->last_rec;
  }
  if (n > gs::kDsMaxFold) {
    d->last_nv = sum[0];
    d->last_occ = sum[1];
    d->last_rec = sum[2];
    d->kept = false;
  }
  if (host) GS_HIP(hipStreamSynchronize(d->stream));
  return GS_OK;
}

int rows_guard(gs_degstream_s* d, size_t* n) {
  if (int rc = check_handle(d, kWhat)) return rc;
  if (!n) return fail(GS_ERR_INVALID, "n is null");
  if (!d->kept) return fail(GS_ERR_INVALID, "degstream rows: the last fold was cut into pieces, its rows were not kept");
  return GS_OK;
}

int rows_impl(gs_degstream_s* d, int64_t* vertex, uint32_t* old_d, uint32_t* new_d, size_t cap, size_t* n, bool to_host) {
  if (int rc = rows_guard(d, n)) return rc;
  DeviceGuard g(d->device);
  const uint64_t rows = d->last_occ;
  *n = rows;
  if (cap < rows) return truncated(cap, rows);
  if (rows == 0) return GS_OK;
  const ColumnCopy copy(d->stream, to_host);
  GS_HIP(copy.col(vertex, d->row_v.get(), rows));
  GS_HIP(copy.col(old_d, d->row_old.get(), rows));
  GS_HIP(copy.col(new_d, d->row_new.get(), rows));
  GS_HIP(copy.done());
  return GS_OK;
}

int records_impl(gs_degstream_s* d, uint32_t* occ, uint32_t* degree, uint32_t* count, size_t cap, size_t* n,
                 bool to_host) {
  if (int rc = rows_guard(d, n)) return rc;
  DeviceGuard g(d->device);
  const uint64_t rows = d->last_rec;
  *n = rows;
  if (cap < rows) return truncated(cap, rows);
  if (rows == 0) return GS_OK;
  const ColumnCopy copy(d->stream, to_host);
  GS_HIP(copy.col(occ, d->r_occ.get(), rows));
  GS_HIP(copy.col(degree, d->r_deg.get(), rows));
  GS_HIP(copy.col(count, d->r_cnt.get(), rows));
  GS_HIP(copy.done());
  return GS_OK;
}

// the live entries of degree[] (ids: the vertex list) or count[] (ids null: the index), in index order
int live_impl(gs_degstream_s* d, const uint32_t* state, uint64_t entries, const int64_t* ids, int64_t* id_out,
              int64_t* value_out, size_t cap, size_t* n, bool to_host) {
  *n = 0;
  if (entries == 0) return GS_OK;
  hipStream_t st = d->stream;
  const uint64_t tiles = gs::ds_tiles(entries, gs::DEGSTREAM_TILE);
  GS_HIP(grow_group(st, d->x_tiles, tiles + 1, tiles + tiles / 4 + 1, [&](uint64_t c) { return d->x_blk.alloc(c); }));
  GS_LAUNCH(gs::launch_ds_live_count(state, entries, d->x_blk, st));
  GS_LAUNCH(gs::launch_tile_scan(d->x_blk, tiles, d->ctl + gs::DS_LIVE, st));
  unsigned long long rows = 0;
  GS_HIP(hipMemcpyAsync(&rows, d->ctl + gs::DS_LIVE, 8, hipMemcpyDeviceToHost, st));
  GS_HIP(hipStreamSynchronize(st));
  if (rows > entries) return fail(GS_ERR_HIP, "degstream export: counts out of range");
  *n = rows;
  if (cap < rows) return truncated(cap, rows);
  if (rows == 0) return GS_OK;
  if (to_host) GS_HIP(d->out.ensure(2, rows, st));
  GS_LAUNCH(gs::launch_ds_live_write(state, entries, d->x_blk, ids, d->out.dev(0, id_out, to_host),
                                     d->out.dev(1, value_out, to_host), rows, st));
  if (to_host) GS_HIP(d->out.finish(st, rows, id_out, value_out));
  return GS_OK;
}

int degrees_impl(gs_degstream_s* d, int64_t* vertex, int64_t* degree, size_t cap, size_t* n, bool to_host) {
  if (int rc = check_handle(d, kWhat)) return rc;
  if (!n) return fail(GS_ERR_INVALID, "n is null");
  DeviceGuard g(d->device);
  return live_impl(d, d->degree, d->nv, d->vid, vertex, degree, cap, n, to_host);
}

int distribution_impl(gs_degstream_s* d, int64_t* degree, int64_t* count, size_t cap, size_t* n, bool to_host) {
  if (int rc = check_handle(d, kWhat)) return rc;
  if (!n) return fail(GS_ERR_INVALID, "n is null");
  DeviceGuard g(d->device);
  return live_impl(d, d->count, std::min<uint64_t>(d->count_cap, d->max_degree + 1), nullptr, degree, count, cap, n,
                   to_host);
}

}  // namespace

extern "C" {

int gs_degstream_destroy(gs_degstream d) { return owner_destroy(d); }

int gs_degstream_create(gs_degstream* out, int device, int dir, uint64_t vertex_hint) {
  if (!out) return fail(GS_ERR_INVALID, "out is null");
  *out = nullptr;
  if (dir < 0 || dir >= gs::kDsDirections) return fail(GS_ERR_INVALID, "degstream create: unknown direction");
  if (vertex_hint > gs::kDistMaxVertices || gs::dist_slots_for(vertex_hint) > gs::kDistMaxSlots)
    return fail(GS_ERR_CAPACITY, "degstream create: the hint passes 2^31 table slots");
  if (int rc = check_device_index(device)) return rc;
  return owner_create(out, device, [&](gs_degstream_s* d) -> int {
    d->dir = dir;
    GS_HIP(d->ctl.alloc(gs::DS_CTL_WORDS));
    GS_HIP(hipMemsetAsync(d->ctl, 0, gs::DS_CTL_WORDS * 8, d->stream));
    GS_HIP(d->dctl.alloc(gs::DIST_CTL_WORDS));
    GS_HIP(hipMemsetAsync(d->dctl, 0, gs::DIST_CTL_WORDS * 8, d->stream));
    if (int rc = grow_counts(d, 0)) return rc;
    return grow_vertices(d, gs::dist_slots_for(vertex_hint));
  });
}

int gs_degstream_reset(gs_degstream d) {
  if (int rc = check_handle(d, kWhat)) return rc;
  DeviceGuard g(d->device);
  GS_LAUNCH(gs::launch_dist_init(d->vtable(), d->stream));
  GS_HIP(hipMemsetAsync(d->degree, 0, gs::dist_vid_cap(d->vcap) * 4, d->stream));
  GS_HIP(hipMemsetAsync(d->count, 0, d->count_cap * 4, d->stream));
  GS_HIP(hipMemsetAsync(d->ctl, 0, gs::DS_CTL_WORDS * 8, d->stream));
  d->nv = d->total = d->max_degree = 0;
  forget_last(d);
  return GS_OK;
}

int gs_degstream_fold_device(gs_degstream d, const int64_t* src, const int64_t* dst, const uint8_t* del, size_t n,
                             size_t stride) {
  if (int rc = fold_guard(d, src, dst, n)) return rc;
  if (stride == 0 || stride > 0xFFFFFFFFull) return fail(GS_ERR_INVALID, "stride must be >= 1");
  return fold_all(d, src, dst, del, n, stride, false);
}

int gs_degstream_fold(gs_degstream d, const int64_t* src, const int64_t* dst, const uint8_t* del, size_t n) {
  if (int rc = fold_guard(d, src, dst, n)) return rc;
  return fold_all(d, src, dst, del, n, 1, true);
}

int gs_degstream_rows_device(gs_degstream d, int64_t* vertex, uint32_t* old_degree, uint32_t* new_degree, size_t cap,
                             size_t* n) {
  return rows_impl(d, vertex, old_degree, new_degree, cap, n, false);
}

int gs_degstream_rows(gs_degstream d, int64_t* vertex, uint32_t* old_degree, uint32_t* new_degree, size_t cap,
                      size_t* n) {
  return rows_impl(d, vertex, old_degree, new_degree, cap, n, true);
}

int gs_degstream_records_device(gs_degstream d, uint32_t* occurrence, uint32_t* degree, uint32_t* count, size_t cap,
                                size_t* n) {
  return records_impl(d, occurrence, degree, count, cap, n, false);
}

int gs_degstream_records(gs_degstream d, uint32_t* occurrence, uint32_t* degree, uint32_t* count, size_t cap,
                         size_t* n) {
  return records_impl(d, occurrence, degree, count, cap, n, true);
}

int gs_degstream_size(gs_degstream d, uint64_t* out) {
  if (int rc = check_handle(d, kWhat)) return rc;
  if (!out) return fail(GS_ERR_INVALID, "out is null");
  out[0] = d->last_nv;
  out[1] = d->last_occ;
  out[2] = d->last_rec;
  out[3] = d->total;
  out[4] = d->max_degree;
  return GS_OK;
}

int gs_degstream_degrees_device(gs_degstream d, int64_t* vertex, int64_t* degree, size_t cap, size_t* n) {
  return degrees_impl(d, vertex, degree, cap, n, false);
}

int gs_degstream_degrees(gs_degstream d, int64_t* vertex, int64_t* degree, size_t cap, size_t* n) {
  return degrees_impl(d, vertex, degree, cap, n, true);
}

int gs_degstream_distribution_device(gs_degstream d, int64_t* degree, int64_t* count, size_t cap, size_t* n) {
  return distribution_impl(d, degree, count, cap, n, false);
}

int gs_degstream_distribution(gs_degstream d, int64_t* degree, int64_t* count, size_t cap, size_t* n) {
  return distribution_impl(d, degree, count, cap, n, true);
}

int gs_degstream_sync(gs_degstream d) { return owner_sync(d, kWhat); }
int gs_degstream_get_stream(gs_degstream d, void** stream) { return owner_get_stream(d, kWhat, stream); }
int gs_degstream_wait_stream(gs_degstream d, void* stream) { return owner_wait_stream(d, kWhat, stream); }

// gs_testing.h: the last fold (synchronises: the crossed-tile word is read from the device)
int gs_testing_degstream_stats(void* handle, uint64_t* out) {
  gs_degstream d = static_cast<gs_degstream>(handle);
  if (int rc = check_handle(d, kWhat)) return rc;
  if (!out) return fail(GS_ERR_INVALID, "out is null");
  DeviceGuard g(d->device);
  unsigned long long crossed = 0;
  GS_HIP(hipMemcpyAsync(&crossed, d->ctl + gs::DS_CROSSED, 8, hipMemcpyDeviceToHost, d->stream));
  GS_HIP(hipStreamSynchronize(d->stream));
  out[0] = d->last_tiles;
  out[1] = d->last_occ ? crossed : 0;
  out[2] = d->count_cap;
  out[3] = d->growths;
  for (int i = 0; i < 5; ++i) out[4 + i] = d->phase_us[i];
  return GS_OK;
}

int gs_testing_degstream_tune(void* handle, int what, int64_t value) {
  gs_degstream d = static_cast<gs_degstream>(handle);
  if (int rc = check_handle(d, kWhat)) return rc;
  if (what != 0) return fail(GS_ERR_INVALID, "degstream tune: unknown control");
  d->profile = value > 0;
  return GS_OK;
}

}  // extern "C"
