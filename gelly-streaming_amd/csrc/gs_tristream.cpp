// gs_tristream.cpp -- the triangle streams behind include/gs_summary.h's gs_tristream_* section:
// every record example/ExactTriangleCount.java emits, exact in arrival order wherever the stream
// is cut into folds. State layout and kernels are described in gs_tristream.hpp /
// gs_tristream_k.hip, the rules and the exactness argument in gs_tristream_seq.hpp (trs_fold_seq,
// trs_fold_parts) and DESIGN.md section 6j.
//
// A fold of n arrivals: growth of the vertex table is decided first from host-known totals; the
// distinct streams' vertex phase gives every new id its rank; the arrivals are canonised and
// sorted stably by (min, max); run heads that are not in A are the new pairs, stamped with the
// number of their arrival. The FIRST wait reads their count, after which the other adjacency
// buffer grows and takes the stamped merge. Every arrival's rows are found in the merged
// adjacency and its intersection counted under the stamp test; the counts are reduced and the
// SECOND wait reads the record count: a fold past the record limit returns here, and nothing it
// did is visible (the buffers are not swapped, the counters, rows and records not written). Then
// the rows and record offsets are written, the records in arrival order, their ranks looked up,
// sorted stably by rank, and the seeded segmented sum writes every record's count and, last,
// the counters. That tail is queued, not waited for.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "gs_internal.hpp"
#include "gs_tristream.hpp"
#include "gs_vtable.hpp"

using namespace gsi;

struct gs_tristream_s : StreamOwner, VertexTable {  // (the vertex table and the vertices in rank order)
  int mode = gs::kTrsCount;
  DevBuf<unsigned long long> ctl;   // gs::TrsCtl words
  DevBuf<unsigned long long> dctl;  // gs::DistCtl words of the vertex phase
  DevBuf<int64_t> counter;          // [dist_vid_cap(vcap)] t of every rank
  // adjacency: two buffers, the merge of a fold reads one and writes the other
  DevBuf<int64_t> ax[2], ay[2];
  DevBuf<uint32_t> af[2];
  uint64_t acap[2] = {0, 0};
  int cur = 0;
  uint64_t entries = 0;  // live entries of buffer `cur` (2 |G|)
  // fold scratch for n_cap arrivals
  uint64_t n_cap = 0;
  DevBuf<uint32_t> vslot, entry;  // [2 n] the vertex phase's
  DevBuf<uint8_t> vflags;         // whole tiles of 2 n positions
  DevBuf<uint32_t> tbase;
  DevBuf<int64_t> lo, hi, nx, ny, rx, ry;
  DevBuf<uint32_t> nf, rf, blk, cnt, roff;
  DevBuf<uint8_t> flags, is_new;
  DevBuf<gs::TrsRowInfo> info;
  DevBuf<gs::TrsSeg> a_agg, a_carry;
  // the rows and records of the last fold, and the record scan's scratch
  uint64_t w_cap = 0;
  DevBuf<uint32_t> row_closed;
  DevBuf<int64_t> row_total;
  uint64_t r_cap = 0;
  DevBuf<uint32_t> r_arr, r_delta;
  DevBuf<int64_t> r_v, r_key, r_cnt;
  DevBuf<gs::TrsSeg> agg, carry;
  SortScratch sort;
  // device staging of a host fold
  FoldStage stage;  // (src, dst)
  // head counts of a fold and of an export; the export's vertices and ranks; host-array staging
  uint64_t x_tiles = 0;
  DevBuf<uint32_t> x_blk;
  uint64_t v_cap = 0;
  DevBuf<int64_t> hv, hrank;
  OutStage out;  // two columns
  // host-known totals (nv of VertexTable: every endpoint seen, a failed fold's included)
  uint64_t vertices = 0, edges = 0, total = 0;
  int64_t triangles = 0;
  uint64_t last_n = 0, last_rec = 0, last_new = 0, last_tiles = 0;
  bool kept = true;  // false after a fold the library cut into pieces
  // gs_testing_tristream_tune (profile, record limit) and the last profiled fold's phases
  bool profile = false;
  uint64_t max_records = gs::kTrsMaxRecords;
  uint64_t phase_us[6] = {0, 0, 0, 0, 0, 0};

  gs::TrsAdj adj(int side, uint64_t n) const {
    gs::TrsAdj a;
    a.x = ax[side];
    a.y = ay[side];
    a.first = af[side];
    a.n = n;
    return a;
  }
};

namespace {

// Adjacency entries are row indices of 32 bits (TrsRowInfo).
constexpr uint64_t kTrsMaxEntries = 0xFFFFFFFFull;
constexpr uint64_t kTrsMinEdges = 32;

constexpr const char* kWhat = "tristream";  // check_handle: "null tristream handle"

// The vertex table grows (VertexTable::grow) and the counters with it, inside the same wait.
int grow_vertices(gs_tristream_s* d, uint64_t cap) { return d->grow_ranked(cap, d->dctl, d->stream, d->counter); }

int ensure_adj(gs_tristream_s* d, int side, uint64_t need) {
  GS_HIP(grow_group(d->stream, d->acap[side], need, std::min<uint64_t>(kTrsMaxEntries, need + need / 2),
                    [&](uint64_t c) { return alloc_each(c, d->ax[side], d->ay[side], d->af[side]); }));
  return GS_OK;
}

int ensure_scratch(gs_tristream_s* d, uint64_t n) {
  const auto alloc_scratch = [&](uint64_t c) {
    const uint64_t vtiles = gs::dist_tiles(2 * c, gs::DISTINCT_TILE);
    const uint64_t tiles = gs::trs_tiles(c, gs::TRISTREAM_TILE) + 1;
    hipError_t e = alloc_each(2 * c, d->vslot, d->entry);
    if (e == hipSuccess) e = d->vflags.alloc(vtiles * gs::DISTINCT_TILE);
    if (e == hipSuccess) e = d->tbase.alloc(vtiles + 1);
    if (e == hipSuccess)
      e = alloc_each(c, d->lo, d->hi, d->nx, d->ny, d->rx, d->ry, d->nf, d->rf, d->cnt, d->roff, d->flags, d->is_new,
                     d->info);
    if (e == hipSuccess) e = d->blk.alloc(gs::tri_blocks(c) + 1);
    if (e == hipSuccess) e = alloc_each(tiles, d->a_agg, d->a_carry);
    return e;
  };
  GS_HIP(grow_group(d->stream, d->n_cap, n, std::min<uint64_t>(gs::kTrsMaxFold, n + n / 4), alloc_scratch));
  return GS_OK;
}

int ensure_rows(gs_tristream_s* d, uint64_t rows) {
  GS_HIP(grow_group(d->stream, d->w_cap, rows, std::min<uint64_t>(gs::kTrsMaxFold, rows + rows / 4),
                    [&](uint64_t c) { return alloc_each(c, d->row_closed, d->row_total); }));
  return GS_OK;
}

int ensure_records(gs_tristream_s* d, uint64_t rows) {
  GS_HIP(grow_group(d->stream, d->r_cap, rows, rows + rows / 4, [&](uint64_t c) {
    const hipError_t e = alloc_each(c, d->r_arr, d->r_delta, d->r_v, d->r_key, d->r_cnt);
    return e != hipSuccess ? e : alloc_each(gs::trs_tiles(c, gs::TRISTREAM_TILE) + 1, d->agg, d->carry);
  }));
  return GS_OK;
}

int ensure_head_tiles(gs_tristream_s* d, uint64_t positions) {
  const uint64_t tiles = gs::trs_tiles(positions, gs::TRISTREAM_TILE) + 1;
  GS_HIP(grow_group(d->stream, d->x_tiles, tiles, tiles + tiles / 4, [&](uint64_t c) { return d->x_blk.alloc(c); }));
  return GS_OK;
}

void forget_last(gs_tristream_s* d) {
  d->last_n = d->last_rec = d->last_new = d->last_tiles = 0;
  d->kept = true;
  for (uint64_t& us : d->phase_us) us = 0;
}

int fold_guard(gs_tristream_s* d, const void* src, const void* dst, size_t n) {
  if (int rc = check_handle(d, kWhat)) return rc;
  if (n && (!src || !dst)) return fail(GS_ERR_INVALID, "null edge arrays");
  if ((uint64_t)n > gs::kTrsMaxTotal || d->total + n > gs::kTrsMaxTotal)
    return fail(GS_ERR_CAPACITY, "tristream fold: " + std::to_string(d->total) + " + " + std::to_string(n) +
                                     " arrivals pass 2^31 - 1 since the last reset");
  if (2 * (d->edges + (uint64_t)n) > kTrsMaxEntries)
    return fail(GS_ERR_CAPACITY, "tristream adjacency: " + std::to_string(d->edges) + " + " + std::to_string(n) +
                                     " pairs could pass 2^32 - 1 entries");
  return d->fold_guard_vertices(n, std::min<uint64_t>(n, gs::kTrsMaxFold), kWhat);
}

// 0 < n <= kTrsMaxFold device arrivals on d->stream
int fold_piece(gs_tristream_s* d, const int64_t* src, const int64_t* dst, uint64_t n, uint64_t stride) {
  hipStream_t st = d->stream;
  const uint64_t t0 = d->total;
  if (int rc = d->ensure_for(n, [&](uint64_t slots) { return grow_vertices(d, slots); })) return rc;
  if (int rc = ensure_scratch(d, n)) return rc;
  if (int rc = sort_scratch_ensure(d->sort, n, st)) return rc;
  const gs::DistVTable vt = d->vtable();
  const uint64_t ranks = gs::dist_vid_cap(d->vcap);
  // phases: ranks, sort and dedupe | merge | count | write | record sort | scan
  PhaseTimer timer(st, d->profile, d->phase_us, 6);
  timer.mark(0);
  GS_HIP(hipMemsetAsync(d->dctl, 0, gs::DIST_CTL_WORDS * 8, st));
  static_assert(gs::TRS_ERR == 0, "the error word outlives a fold: every wait reads it");
  GS_HIP(hipMemsetAsync(d->ctl + 1, 0, (gs::TRS_CTL_WORDS - 1) * 8, st));
  // 1. ranks for every endpoint; canonical pairs
  GS_LAUNCH(gs::launch_dist_vertices(src, dst, n, stride, vt, d->vslot, d->vflags, d->tbase, d->nv, d->vid, ranks,
                                     d->entry, d->dctl, st));
  GS_LAUNCH(gs::launch_tri_canon(src, dst, n, stride, d->lo, d->hi, st));
  // 2. sort by max, then stably by min: the head of a run of equal pairs is its earliest arrival
  gs::SortSrc cur;
  if (int rc = sort_by_pair(d->sort, d->lo, d->hi, n, &cur, st)) return rc;
  gs::TriAdj old;
  old.x = d->ax[d->cur];
  old.y = d->ay[d->cur];
  old.n = d->entries;
  GS_LAUNCH(gs::launch_tri_flag_new(cur.pay, d->lo, d->hi, n, old, d->flags, d->blk, st));
  GS_LAUNCH(gs::launch_tile_scan(d->blk, gs::tri_blocks(n), d->ctl + gs::TRS_NEW, st));
  GS_LAUNCH(gs::launch_trs_compact_new(cur.pay, d->lo, d->hi, n, d->flags, d->blk, t0, d->nx, d->ny, d->nf, d->is_new,
                                       d->n_cap, st));
  // the first wait: the new pairs, the new ids
  unsigned long long c[gs::TRS_CTL_WORDS], v[gs::DIST_CTL_WORDS];
  GS_HIP(hipMemcpyAsync(c, d->ctl, sizeof(c), hipMemcpyDeviceToHost, st));
  GS_HIP(hipMemcpyAsync(v, d->dctl, sizeof(v), hipMemcpyDeviceToHost, st));
  timer.mark(1);
  GS_HIP(hipStreamSynchronize(st));
  if (v[gs::DIST_OVERFLOW]) return fail(GS_ERR_HIP, "tristream fold: the vertex table overflowed (the handle's state is undefined)");
  if (c[gs::TRS_ERR]) return fail(GS_ERR_HIP, "tristream fold: an index out of range (the handle's state is undefined)");
  const uint64_t m = c[gs::TRS_NEW];
  if (v[gs::DIST_NEW_V] > 2 * n || m > n) return fail(GS_ERR_HIP, "tristream fold: counts out of range");
  d->nv += v[gs::DIST_NEW_V];  // (the table holds them whatever becomes of the fold; their counters are 0)
  // 3. the stamped merge into the other buffer
  const int other = d->cur ^ 1;
  int side = d->cur;
  const uint64_t merged = d->entries + 2 * m;
  if (m) {
    if (int rc = ensure_adj(d, other, merged)) return rc;
    if (int rc = ensure_head_tiles(d, merged)) return rc;
    if (int rc = sort_by_key(d->sort, d->ny, m, nullptr, &cur, st, "tristream fold")) return rc;  // (ids: no bound)
    GS_LAUNCH(gs::launch_trs_reverse(cur.pay, d->nx, d->ny, d->nf, m, d->rx, d->ry, d->rf, st));
    gs::TrsAdjOut out;
    out.x = d->ax[other];
    out.y = d->ay[other];
    out.first = d->af[other];
    out.cap = d->acap[other];
    GS_LAUNCH(gs::launch_trs_merge(d->adj(d->cur, d->entries), d->nx, d->ny, d->nf, d->rx, d->ry, d->rf, m, out, st));
    GS_LAUNCH(gs::launch_trs_head_count(d->ax[other], merged, d->x_blk, st));
    GS_LAUNCH(gs::launch_tile_scan(d->x_blk, gs::trs_tiles(merged, gs::TRISTREAM_TILE), d->ctl + gs::TRS_HEADS, st));
    side = other;
  }
  const gs::TrsAdj M = d->adj(side, merged);
  timer.mark(2);
  // 4. rows and the count pass; the reduce half of the scan over the arrivals
  GS_LAUNCH(gs::launch_trs_rows(M, d->lo, d->hi, d->mode == gs::kTrsIgnore ? d->is_new.get() : nullptr, n, d->info,
                                d->ctl, st));
  GS_LAUNCH(gs::launch_trs_count(M, d->info, n, t0, d->cnt, d->ctl, st));
  GS_LAUNCH(gs::launch_trs_arr_reduce(d->cnt, n, d->a_agg, d->a_carry, d->ctl, st));
  // the second wait: the record count
  GS_HIP(hipMemcpyAsync(c, d->ctl, sizeof(c), hipMemcpyDeviceToHost, st));
  timer.mark(3);
  GS_HIP(hipStreamSynchronize(st));
  if (c[gs::TRS_ERR]) return fail(GS_ERR_HIP, "tristream fold: an index out of range (the handle's state is undefined)");
  const uint64_t closed = c[gs::TRS_CLOSED], recs = c[gs::TRS_RECORDS];
  if (recs > d->max_records)
    return fail(GS_ERR_CAPACITY, "tristream fold: " + std::to_string(recs) + " records pass the limit of " +
                                     std::to_string(d->max_records) + " per fold (fold smaller pieces: the stream is the same)");
  if (m && c[gs::TRS_HEADS] > merged) return fail(GS_ERR_HIP, "tristream fold: counts out of range");
  if (int rc = ensure_rows(d, n)) return rc;
  if (recs) {
    if (int rc = ensure_records(d, recs)) return rc;
    if (int rc = sort_scratch_ensure(d->sort, recs, st)) return rc;
  }
  // 5. from here on the fold is visible: rows and offsets, 6. the ordered write
  GS_LAUNCH(gs::launch_trs_arr_apply(d->cnt, n, d->a_carry, d->triangles, d->row_closed, d->row_total, d->roff, st));
  if (recs)
    GS_LAUNCH(gs::launch_trs_write(M, d->info, d->lo, d->hi, d->cnt, d->roff, n, t0, d->r_arr, d->r_v, d->r_delta, recs,
                                   d->ctl, st));
  timer.mark(4);
  if (recs) {
    // 7. ranks, the stable sort by rank, the seeded segmented sum, the counters
    GS_LAUNCH(gs::launch_dist_rank(vt, d->r_v, recs, d->r_key, nullptr, st));
    bool skip[gs::kSortPasses];  // every key is a rank below nv
    sort_skip_above(d->nv, skip);
    if (int rc = sort_by_key(d->sort, d->r_key, recs, skip, &cur, st, "tristream fold")) return rc;
    timer.mark(5);
    GS_LAUNCH(gs::launch_trs_seg_pass(cur.key, cur.pay, d->r_delta, recs, d->counter, ranks, d->agg, d->carry, d->r_cnt,
                                      d->ctl, st));
    timer.mark(6);
  }
  if (m) {
    d->cur = other;
    d->entries = merged;
    d->edges += m;
    d->vertices = c[gs::TRS_HEADS];
  }
  d->total += n;
  d->triangles += (int64_t)closed;
  d->last_n = n;
  d->last_rec = recs;
  d->last_new = m;
  d->last_tiles = gs::trs_tiles(recs, gs::TRISTREAM_TILE);
  d->kept = true;
  timer.finish();
  return GS_OK;
}

// the whole fold, cut into pieces of at most kTrsMaxFold arrivals; host: the arrays are HOST arrays
int fold_all(gs_tristream_s* d, const int64_t* src, const int64_t* dst, size_t n, uint64_t stride, bool host) {
  if (n == 0) {
    forget_last(d);
    return GS_OK;
  }
  DeviceGuard g(d->device);
  uint64_t sum[3] = {0, 0, 0};
  for (uint64_t at = 0; at < n; at += gs::kTrsMaxFold) {
    const uint64_t len = std::min<uint64_t>(gs::kTrsMaxFold, n - at);
    const int64_t* col[2] = {src + at * stride, dst + at * stride};
    if (host) GS_HIP(d->stage.put(d->stream, len, gs::kTrsMaxFold, col));
    if (int rc = fold_piece(d, col[0], col[1], len, host ? 1 : stride)) {
      if (at) d->kept = false;  // (the pieces before this one are folded: gs_tristream_size tells how far)
      return rc;
    }
    sum[0] += d->last_n;
    sum[1] += d->last_rec;
    sum[2] += d->last_new;
  }
  if (n > gs::kTrsMaxFold) {
    d->last_n = sum[0];
    d->last_rec = sum[1];
    d->last_new = sum[2];
    d->kept = false;
  }
  if (host) GS_HIP(hipStreamSynchronize(d->stream));
  return GS_OK;
}

int rows_guard(gs_tristream_s* d, size_t* n) {
  if (int rc = check_handle(d, kWhat)) return rc;
  if (!n) return fail(GS_ERR_INVALID, "n is null");
  if (!d->kept) return fail(GS_ERR_INVALID, "tristream rows: the last fold was cut into pieces, its rows were not kept");
  return GS_OK;
}

int rows_impl(gs_tristream_s* d, uint32_t* closed, int64_t* total, size_t cap, size_t* n, bool to_host) {
  if (int rc = rows_guard(d, n)) return rc;
  DeviceGuard g(d->device);
  const uint64_t rows = d->last_n;
  *n = rows;
  if (cap < rows) return truncated(cap, rows);
  if (rows == 0) return GS_OK;
  const ColumnCopy copy(d->stream, to_host);
  GS_HIP(copy.col(closed, d->row_closed.get(), rows));
  GS_HIP(copy.col(total, d->row_total.get(), rows));
  GS_HIP(copy.done());
  return GS_OK;
}

int records_impl(gs_tristream_s* d, uint32_t* arrival, int64_t* vertex, int64_t* count, size_t cap, size_t* n,
                 bool to_host) {
  if (int rc = rows_guard(d, n)) return rc;
  DeviceGuard g(d->device);
  const uint64_t rows = d->last_rec;
  *n = rows;
  if (cap < rows) return truncated(cap, rows);
  if (rows == 0) return GS_OK;
  const ColumnCopy copy(d->stream, to_host);
  GS_HIP(copy.col(arrival, d->r_arr.get(), rows));
  GS_HIP(copy.col(vertex, d->r_v.get(), rows));
  GS_HIP(copy.col(count, d->r_cnt.get(), rows));
  GS_HIP(copy.done());
  return GS_OK;
}

// (vertex, t) with t > 0 ascending by vertex: A's row heads are the vertices in that order
int counts_impl(gs_tristream_s* d, int64_t* vertex, int64_t* count, size_t cap, size_t* n, bool to_host) {
  if (int rc = check_handle(d, kWhat)) return rc;
  if (!n) return fail(GS_ERR_INVALID, "n is null");
  DeviceGuard g(d->device);
  *n = 0;
  const uint64_t heads = d->vertices;
  if (heads == 0 || d->entries == 0) return GS_OK;
  hipStream_t st = d->stream;
  if (int rc = ensure_head_tiles(d, d->entries)) return rc;
  GS_HIP(grow_group(st, d->v_cap, heads, heads + heads / 4, [&](uint64_t c) { return alloc_each(c, d->hv, d->hrank); }));
  const int64_t* x = d->ax[d->cur];
  const uint64_t ranks = gs::dist_vid_cap(d->vcap);
  GS_LAUNCH(gs::launch_trs_head_count(x, d->entries, d->x_blk, st));
  GS_LAUNCH(gs::launch_tile_scan(d->x_blk, gs::trs_tiles(d->entries, gs::TRISTREAM_TILE), d->ctl + gs::TRS_LIVE, st));
  GS_LAUNCH(gs::launch_trs_head_write(x, d->entries, d->x_blk, d->hv, heads, st));
  GS_LAUNCH(gs::launch_dist_rank(d->vtable(), d->hv, heads, d->hrank, nullptr, st));
  GS_LAUNCH(gs::launch_trs_live_count(d->hrank, heads, d->counter, ranks, d->x_blk, st));
  GS_LAUNCH(gs::launch_tile_scan(d->x_blk, gs::trs_tiles(heads, gs::TRISTREAM_TILE), d->ctl + gs::TRS_LIVE, st));
  unsigned long long rows = 0;
  GS_HIP(hipMemcpyAsync(&rows, d->ctl + gs::TRS_LIVE, 8, hipMemcpyDeviceToHost, st));
  GS_HIP(hipStreamSynchronize(st));
  if (rows > heads) return fail(GS_ERR_HIP, "tristream counts: counts out of range");
  *n = rows;
  if (cap < rows) return truncated(cap, rows);
  if (rows == 0) return GS_OK;
  if (to_host) GS_HIP(d->out.ensure(2, rows, st));
  GS_LAUNCH(gs::launch_trs_live_write(d->hv, d->hrank, heads, d->counter, ranks, d->x_blk, d->out.dev(0, vertex, to_host),
                                      d->out.dev(1, count, to_host), rows, st));
  if (to_host) GS_HIP(d->out.finish(st, rows, vertex, count));
  return GS_OK;
}

}  // namespace

extern "C" {

int gs_tristream_destroy(gs_tristream d) { return owner_destroy(d); }

int gs_tristream_create(gs_tristream* out, int device, int repeats_mode, uint64_t edge_hint) {
  if (!out) return fail(GS_ERR_INVALID, "out is null");
  *out = nullptr;
  if (repeats_mode < 0 || repeats_mode >= gs::kTrsModes) return fail(GS_ERR_INVALID, "tristream create: unknown repeats mode");
  if (2 * edge_hint > kTrsMaxEntries || gs::dist_slots_for(2 * edge_hint) > gs::kDistMaxSlots)
    return fail(GS_ERR_CAPACITY, "tristream create: the hint passes 2^31 - 1 pairs");
  if (int rc = check_device_index(device)) return rc;
  return owner_create(out, device, [&](gs_tristream_s* d) -> int {
    d->mode = repeats_mode;
    GS_HIP(d->ctl.alloc(gs::TRS_CTL_WORDS));
    GS_HIP(hipMemsetAsync(d->ctl, 0, gs::TRS_CTL_WORDS * 8, d->stream));
    GS_HIP(d->dctl.alloc(gs::DIST_CTL_WORDS));
    GS_HIP(hipMemsetAsync(d->dctl, 0, gs::DIST_CTL_WORDS * 8, d->stream));
    const uint64_t e = std::max<uint64_t>(edge_hint, kTrsMinEdges);
    if (int rc = ensure_adj(d, 0, 2 * e)) return rc;
    return grow_vertices(d, gs::dist_slots_for(e));
  });
}

int gs_tristream_reset(gs_tristream d) {
  if (int rc = check_handle(d, kWhat)) return rc;
  DeviceGuard g(d->device);
  GS_LAUNCH(gs::launch_dist_init(d->vtable(), d->stream));
  GS_HIP(hipMemsetAsync(d->counter, 0, gs::dist_vid_cap(d->vcap) * 8, d->stream));
  GS_HIP(hipMemsetAsync(d->ctl, 0, gs::TRS_CTL_WORDS * 8, d->stream));
  d->nv = d->vertices = d->edges = d->total = d->entries = 0;
  d->triangles = 0;
  forget_last(d);
  return GS_OK;
}

int gs_tristream_fold_device(gs_tristream d, const int64_t* src, const int64_t* dst, size_t n, size_t stride) {
  if (int rc = fold_guard(d, src, dst, n)) return rc;
  if (stride == 0 || stride > 0xFFFFFFFFull) return fail(GS_ERR_INVALID, "stride must be >= 1");
  return fold_all(d, src, dst, n, stride, false);
}

int gs_tristream_fold(gs_tristream d, const int64_t* src, const int64_t* dst, size_t n) {
  if (int rc = fold_guard(d, src, dst, n)) return rc;
  return fold_all(d, src, dst, n, 1, true);
}

int gs_tristream_rows_device(gs_tristream d, uint32_t* closed, int64_t* total, size_t cap, size_t* n) {
  return rows_impl(d, closed, total, cap, n, false);
}

int gs_tristream_rows(gs_tristream d, uint32_t* closed, int64_t* total, size_t cap, size_t* n) {
  return rows_impl(d, closed, total, cap, n, true);
}

int gs_tristream_records_device(gs_tristream d, uint32_t* arrival, int64_t* vertex, int64_t* count, size_t cap,
                                size_t* n) {
  return records_impl(d, arrival, vertex, count, cap, n, false);
}

int gs_tristream_records(gs_tristream d, uint32_t* arrival, int64_t* vertex, int64_t* count, size_t cap, size_t* n) {
  return records_impl(d, arrival, vertex, count, cap, n, true);
}

int gs_tristream_size(gs_tristream d, uint64_t* out) {
  if (int rc = check_handle(d, kWhat)) return rc;
  if (!out) return fail(GS_ERR_INVALID, "out is null");
  out[0] = d->last_n;
  out[1] = d->last_rec;
  out[2] = d->last_new;
  out[3] = d->total;
  return GS_OK;
}

// synchronises: the error word of the last fold's queued tail is read
int gs_tristream_count(gs_tristream d, uint64_t* out) {
  if (int rc = check_handle(d, kWhat)) return rc;
  if (!out) return fail(GS_ERR_INVALID, "out is null");
  DeviceGuard g(d->device);
  unsigned long long err = 0;
  GS_HIP(hipMemcpyAsync(&err, d->ctl + gs::TRS_ERR, 8, hipMemcpyDeviceToHost, d->stream));
  GS_HIP(hipStreamSynchronize(d->stream));
  if (err) return fail(GS_ERR_HIP, "tristream: an index out of range in the last fold (the handle's state is undefined)");
  out[0] = (uint64_t)d->triangles;
  out[1] = d->edges;
  out[2] = d->vertices;
  out[3] = d->total;
  return GS_OK;
}

int gs_tristream_counts_device(gs_tristream d, int64_t* vertex, int64_t* count, size_t cap, size_t* n) {
  return counts_impl(d, vertex, count, cap, n, false);
}

int gs_tristream_counts(gs_tristream d, int64_t* vertex, int64_t* count, size_t cap, size_t* n) {
  return counts_impl(d, vertex, count, cap, n, true);
}

int gs_tristream_sync(gs_tristream d) { return owner_sync(d, kWhat); }
int gs_tristream_get_stream(gs_tristream d, void** stream) { return owner_get_stream(d, kWhat, stream); }
int gs_tristream_wait_stream(gs_tristream d, void* stream) { return owner_wait_stream(d, kWhat, stream); }

// gs_testing.h: the last fold (synchronises: the words are read from the device)
int gs_testing_tristream_stats(void* handle, uint64_t* out) {
  gs_tristream d = static_cast<gs_tristream>(handle);
  if (int rc = check_handle(d, kWhat)) return rc;
  if (!out) return fail(GS_ERR_INVALID, "out is null");
  DeviceGuard g(d->device);
  unsigned long long c[gs::TRS_CTL_WORDS];
  GS_HIP(hipMemcpyAsync(c, d->ctl, sizeof(c), hipMemcpyDeviceToHost, d->stream));
  GS_HIP(hipStreamSynchronize(d->stream));
  const bool any = d->last_n != 0;
  out[0] = d->last_tiles;
  out[1] = any ? c[gs::TRS_CROSSED] : 0;
  out[2] = any ? c[gs::TRS_HOT] : 0;
  out[3] = any ? c[gs::TRS_STEPS] : 0;
  for (int i = 0; i < 6; ++i) out[4 + i] = d->phase_us[i];
  return GS_OK;
}

int gs_testing_tristream_tune(void* handle, int what, int64_t value) {
  gs_tristream d = static_cast<gs_tristream>(handle);
  if (int rc = check_handle(d, kWhat)) return rc;
  if (what == 0) {
    d->profile = value > 0;
    return GS_OK;
  }
  if (what == 1) {
    if (value > (int64_t)gs::kTrsMaxRecords) return fail(GS_ERR_INVALID, "tristream tune: the record limit is at most 2^27");
    d->max_records = value > 0 ? (uint64_t)value : gs::kTrsMaxRecords;
    return GS_OK;
  }
  return fail(GS_ERR_INVALID, "tristream tune: unknown control");
}

}  // extern "C"
