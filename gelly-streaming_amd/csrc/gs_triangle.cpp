// gs_triangle.cpp -- the triangle summary behind include/gs_summary.h's gs_triangle_* section:
// exact triangle counts of the graph G folded so far, global (T) and per vertex (t(v)), per
// window (reset, fold, read: example/WindowTriangles) or running (fold after fold:
// example/ExactTriangleCount). State layout, the once-only rule and the kernels are described
// in gs_triangle.hpp / gs_triangle_k.hip and DESIGN.md section 6c.
//
// A fold of n edges: canonise; sort by (min, max) with two stable passes of gs_sort_k.hip's
// radix sort; drop loops, repeats and pairs already in A (the new edges N); ONE host
// synchronisation to learn |N| and the vertex count, after which the table and the adjacency
// buffers grow when they must; sort N's reverse entries; merge A, N and reverse N into the
// other adjacency buffer; per new edge insert the endpoints and find their rows; count.
//
// A removal (by name: gs_triangle_remove; by age in folds: gs_triangle_expire): the dying edges
// D and a dying byte per entry of A, every survivor's position and the rows without one; ONE
// host synchronisation to learn |D|; per dying edge find its rows in A as it stands; the same
// count with the dying entries as the marked set, taken away; compact the survivors into the
// other buffer; rebuild the table at its capacity when a vertex vanished (remove_impl).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "gs_internal.hpp"
#include "gs_triangle.hpp"

using namespace gsi;

struct gs_triangles_s : StreamOwner {
  // relabel table with the counters t(v)
  DevBuf<gs::Slot> tab;
  uint64_t cap = 0;
  int logcap = 0;
  DevBuf<uint32_t> ctr;
  DevBuf<unsigned long long> ctl;  // gs::TriCtl words
  // adjacency: two buffers, the merge of a fold reads one and writes the other
  DevBuf<int64_t> ax[2];
  DevBuf<int64_t> ay[2];
  DevBuf<uint32_t> aseq[2];
  uint64_t acap[2] = {0, 0};
  int cur = 0;
  uint64_t entries = 0;  // live entries of buffer `cur` (2 |G|)
  uint64_t edges = 0;    // |G|, exact after every fold
  uint32_t seq = 0;      // number of the last fold
  // fold scratch, sized for f_cap elements; the radix sort's scratch holds as many pairs
  uint64_t f_cap = 0;
  DevBuf<int64_t> stage;  // [2][f_cap] host folds
  DevBuf<int64_t> lo;     // canonical pairs; later the reverse entries of N
  DevBuf<int64_t> hi;
  DevBuf<int64_t> nx;     // N
  DevBuf<int64_t> ny;
  DevBuf<gs::TriRowInfo> info;
  DevBuf<uint32_t> list1;
  DevBuf<uint32_t> list2;
  SortScratch sort;
  // flag / tile-count scratch of the dedup and of the exports, sized for g_cap elements
  uint64_t g_cap = 0;
  DevBuf<uint8_t> flags;
  DevBuf<uint32_t> blk;
  // device staging of the host export
  uint64_t o_cap = 0;
  DevBuf<int64_t> o_v;
  DevBuf<int64_t> o_c;
  // diagnostics (gs_testing_triangle_stats): phase times of the last profiled fold, microseconds
  uint64_t phase_us[4] = {0, 0, 0, 0};
  // removal: a dying byte and a survivor position per entry of A, sized for d_cap entries
  uint64_t d_cap = 0;
  DevBuf<uint8_t> dead;
  DevBuf<uint32_t> pos;
  // the dying edges D with their rows and the removal's own lists, sized for r_cap edges
  uint64_t r_cap = 0;
  DevBuf<int64_t> dx;
  DevBuf<int64_t> dy;
  DevBuf<gs::TriRowInfo> rinfo;
  DevBuf<uint32_t> rlist1;
  DevBuf<uint32_t> rlist2;
  // the table a removal that loses a vertex rebuilds into (cap2 slots; swapped with tab)
  DevBuf<gs::Slot> tab2;
  uint64_t cap2 = 0;
  bool refresh = false;   // gs_triangle_set_refresh
  uint64_t r_edges = 0;   // |D| of the last removal
  uint64_t rphase_us[3] = {0, 0, 0};  // its mark / count / compact and rebuild phases when profiled

  gs::Table table() const { return make_table(tab, ctr, cap, logcap); }
  gs::TriAdj adj() const {
    gs::TriAdj a;
    a.x = ax[cur];
    a.y = ay[cur];
    a.seq = aseq[cur];
    a.n = entries;
    return a;
  }
};

namespace {

// Adjacency entries are row indices of 32 bits (TriRowInfo, the sort's payload).
constexpr uint64_t kTriMaxEntries = 0xFFFFFFFFull;
constexpr uint64_t kTriMinCap = 64;

constexpr const char* kWhat = "triangle";  // check_handle: "null triangle handle"

int count_variant() {
  const int64_t v = testing_value(GS_TESTING_TRIANGLE_VARIANT, gs::kTriangleProduct);
  return v >= 0 && v < gs::kTriangleVariants ? (int)v : gs::kTriangleProduct;
}

// (t->tab empty: gs_triangle_create, or grow_table holding the old table aside)
int alloc_table(gs_triangles_s* t, uint64_t cap) {
  if (cap > kMaxCap) return fail(GS_ERR_CAPACITY, "vertex table would exceed 2^30 slots");
  GS_HIP(t->tab.alloc(cap + 1));
  t->cap = cap;
  t->logcap = log2_ceil(cap);
  GS_LAUNCH(gs::launch_tri_init(t->table(), t->stream));
  return GS_OK;
}

int ensure_adj(gs_triangles_s* t, int side, uint64_t need) {
  GS_HIP(grow_group(t->stream, t->acap[side], need, std::min<uint64_t>(kTriMaxEntries, need + need / 2),
                    [&](uint64_t c) { return alloc_each(c, t->ax[side], t->ay[side], t->aseq[side]); }));
  return GS_OK;
}

int ensure_flags(gs_triangles_s* t, uint64_t n) {
  GS_HIP(grow_group(t->stream, t->g_cap, n, n + n / 4, [&](uint64_t c) {
    const hipError_t e = t->flags.alloc(c);
    return e != hipSuccess ? e : t->blk.alloc(gs::tri_blocks(c) + 1);
  }));
  return GS_OK;
}

int ensure_fold_scratch(gs_triangles_s* t, uint64_t n) {
  if (int rc = ensure_flags(t, n)) return rc;
  if (int rc = sort_scratch_ensure(t->sort, n, t->stream)) return rc;
  // (the sort scratch's count)
  GS_HIP(grow_group(t->stream, t->f_cap, n, gs::sort_blocks(n + n / 4) * gs::kSortTile, [&](uint64_t c) {
    const hipError_t e = t->stage.alloc(2 * c);
    return e != hipSuccess ? e : alloc_each(c, t->lo, t->hi, t->nx, t->ny, t->info, t->list1, t->list2);
  }));
  return GS_OK;
}

// A table of new_cap slots carrying every vertex's counter: A's row heads are the vertices.
int grow_table(gs_triangles_s* t, uint64_t new_cap) {
  if (new_cap > kMaxCap) return fail(GS_ERR_CAPACITY, "vertex table would exceed 2^30 slots");
  const gs::Table old = t->table();
  DevBuf<gs::Slot> old_tab;  // (alive until the new table holds its counters)
  old_tab.swap(t->tab);
  if (int rc = alloc_table(t, new_cap)) {
    old_tab.swap(t->tab);  // (the old table still serves)
    t->cap = old.cap;
    t->logcap = 64 - old.shift;
    return rc;
  }
  GS_LAUNCH(gs::launch_tri_rehash(old, t->table(), t->adj(), t->stream));
  GS_HIP(hipStreamSynchronize(t->stream));
  return GS_OK;
}

// The next fold number; a fold of no elements takes one too (ages count calls). At the wrap of
// the 32 bits every stamp moves down by 2^31 (older ones to 0) and the fold becomes number 2^31:
// ages inside the last 2^31 folds stay exact, and no stamp equals or exceeds the new number.
int advance_fold(gs_triangles_s* t) {
  if (++t->seq == 0) {
    GS_LAUNCH(gs::launch_tri_rebase(t->aseq[t->cur], t->entries, t->stream));
    t->seq = 0x80000000u;
  }
  return GS_OK;
}

// n > 0 device elements src[i * stride], dst[i * stride] on t->stream
int fold_impl(gs_triangles_s* t, const int64_t* src, const int64_t* dst, uint64_t n, uint64_t stride) {
  if (int rc = ensure_fold_scratch(t, n)) return rc;
  if (int rc = advance_fold(t)) return rc;
  PhaseTimer timer(t->stream, testing_value(GS_TESTING_TRIANGLE_PROFILE, 0) == 1, t->phase_us, 4);
  timer.mark(0);
  // 1. canonise
  GS_LAUNCH(gs::launch_tri_canon(src, dst, n, stride, t->lo, t->hi, t->stream));
  timer.mark(1);
  // 2. sort by max, then stably by min; flag, scan, compact: N in (nx, ny)
  // (no digit is skipped: the histograms are on the device only)
  gs::SortSrc cur;
  if (int rc = sort_by_pair(t->sort, t->lo, t->hi, n, &cur, t->stream)) return rc;
  GS_LAUNCH(gs::launch_tri_flag_new(cur.pay, t->lo, t->hi, n, t->adj(), t->flags, t->blk, t->stream));
  GS_LAUNCH(gs::launch_tile_scan(t->blk, gs::tri_blocks(n), t->ctl + gs::TRI_NEW, t->stream));
  GS_LAUNCH(gs::launch_tri_compact_new(cur.pay, t->lo, t->hi, n, t->flags, t->blk, t->nx, t->ny, t->f_cap, t->stream));
  // the fold's one host synchronisation: |N|, the vertex count, the digit histograms of max
  unsigned long long words[4] = {0, 0, 0, 0};
  std::vector<uint32_t> hist(gs::kSortPasses * gs::kSortRadix);
  GS_HIP(hipMemcpyAsync(words, t->ctl, sizeof(words), hipMemcpyDeviceToHost, t->stream));
  GS_HIP(hipMemcpyAsync(hist.data(), t->sort.hist(1), hist.size() * 4, hipMemcpyDeviceToHost, t->stream));
  timer.mark(2);
  GS_HIP(hipStreamSynchronize(t->stream));
  const uint64_t m = words[gs::TRI_NEW], nv = words[gs::TRI_NV];
  if (m > n) return fail(GS_ERR_HIP, "triangle fold: more new edges than elements");
  // Refresh (off by default): the edges of this fold that A already held take its number, in a
  // pass BEHIND the count step, which reads seq == current as "new in this fold".
  const auto restamp = [&]() -> int {
    if (!t->refresh) return GS_OK;
    GS_LAUNCH(gs::launch_tri_restamp(t->lo, t->hi, n, t->adj(), t->aseq[t->cur], t->seq, t->stream));
    return GS_OK;
  };
  if (m == 0) {
    if (int rc = restamp()) return rc;
    timer.finish();
    return GS_OK;
  }
  // (a failure below -- out of device memory while growing -- leaves G and its counts as they were)
  if ((double)(nv + 2 * m) > kMaxLoad * (double)t->cap) {
    uint64_t nc = t->cap;
    while (kMaxLoad * (double)nc < (double)(nv + 2 * m)) nc <<= 1;
    if (int rc = grow_table(t, nc)) return rc;
  }
  const int other = t->cur ^ 1;
  if (int rc = ensure_adj(t, other, t->entries + 2 * m)) return rc;
  // 3. N ordered by (max, min): a stable sort of N by max. A digit on which every max of the
  // fold agrees is an identity pass for N's subset of them.
  bool skip[gs::kSortPasses];
  sort_skip_digits(hist.data(), n, skip);
  uint32_t* const sctl = t->sort.ctl;
  GS_HIP(hipMemsetAsync(sctl, 0, gs::kSortCtlWords * 4, t->stream));
  GS_LAUNCH(gs::launch_sort_digits(t->ny, t->ny, m, sctl, t->stream));
  cur = gs::SortSrc();
  int side = 0;
  if (int rc = sort_run(t->sort, t->ny, m, sctl, skip, &cur, &side, t->stream)) return rc;
  // (refresh reads the canonical pairs again behind the count: the reverse entries then go to the
  // host fold's staging, whose elements the canonise pass has consumed)
  int64_t* const rx = t->refresh ? (int64_t*)t->stage : (int64_t*)t->lo;
  int64_t* const ry = t->refresh ? (int64_t*)t->stage + t->f_cap : (int64_t*)t->hi;
  GS_LAUNCH(gs::launch_tri_reverse(cur.pay, t->nx, t->ny, m, rx, ry, t->stream));
  gs::TriAdjOut out;
  out.x = t->ax[other];
  out.y = t->ay[other];
  out.seq = t->aseq[other];
  out.cap = t->acap[other];
  GS_LAUNCH(gs::launch_tri_merge(t->adj(), t->nx, t->ny, rx, ry, m, out, t->seq, t->stream));
  t->cur = other;
  t->entries += 2 * m;
  t->edges += m;
  timer.mark(3);
  // 4. rows and count
  const int variant = count_variant();
  GS_HIP(hipMemsetAsync(t->ctl + gs::TRI_BIN1, 0, 16, t->stream));
  GS_LAUNCH(gs::launch_tri_rows(t->table(), t->ctl, t->adj(), t->nx, t->ny, m, t->info, t->list1, t->list2, variant,
                                t->stream));
  GS_LAUNCH(gs::launch_tri_count(t->table(), t->ctl, t->adj(), t->nx, t->ny, m, t->info, t->list1, t->list2, t->seq,
                                 variant, t->stream));
  timer.mark(4);
  if (int rc = restamp()) return rc;
  timer.finish();
  return GS_OK;
}

int ensure_removal(gs_triangles_s* t, uint64_t entries, uint64_t dying) {
  GS_HIP(grow_group(t->stream, t->d_cap, entries, std::min<uint64_t>(kTriMaxEntries, entries + entries / 4),
                    [&](uint64_t c) { return alloc_each(c, t->dead, t->pos); }));
  GS_HIP(grow_group(t->stream, t->r_cap, dying, dying + dying / 4,
                    [&](uint64_t c) { return alloc_each(c, t->dx, t->dy, t->rinfo, t->rlist1, t->rlist2); }));
  return GS_OK;
}

// A fresh table of the same capacity holding the vertices of A (its row heads) with their
// counters: a removal that loses a vertex leaves its slot behind otherwise, found by
// gs_triangle_find_device and never reused. The two tables are swapped, so only the first
// rebuild at a capacity waits (for the allocation).
int rebuild_table(gs_triangles_s* t) {
  if (t->cap2 != t->cap) {
    GS_HIP(hipStreamSynchronize(t->stream));
    t->cap2 = 0;
    GS_HIP(t->tab2.alloc(t->cap + 1));
    t->cap2 = t->cap;
  }
  const gs::Table old = t->table();
  t->tab.swap(t->tab2);
  GS_LAUNCH(gs::launch_tri_init(t->table(), t->stream));
  GS_LAUNCH(gs::launch_tri_rehash(old, t->table(), t->adj(), t->stream));
  return GS_OK;
}

// The removal path: folds == 0 removes the n device pairs src[i * stride],
// dst[i * stride]; folds >= 1 removes by age. One host synchronisation, for |D|.
int remove_impl(gs_triangles_s* t, const int64_t* src, const int64_t* dst, uint64_t n, uint64_t stride,
                uint64_t folds) {
  const bool by_age = folds != 0;
  t->r_edges = 0;
  for (uint64_t& u : t->rphase_us) u = 0;
  static_assert(gs::TRI_RLIVE - gs::TRI_RNEW == 6, "the removal's words are adjacent");
  GS_HIP(hipMemsetAsync(t->ctl + gs::TRI_RNEW, 0, 7 * 8, t->stream));
  // nothing can die: G is empty, no element, or no stamp that old (every stamp is >= 0 and <= seq)
  if (t->entries == 0 || (by_age ? folds > (uint64_t)t->seq : n == 0)) return GS_OK;
  const uint64_t E = t->entries;
  const uint64_t bound = by_age ? t->edges : std::min<uint64_t>(n, t->edges);
  if (int rc = ensure_flags(t, std::max<uint64_t>(E, by_age ? 0 : n))) return rc;
  if (!by_age)
    if (int rc = ensure_fold_scratch(t, n)) return rc;
  if (int rc = ensure_removal(t, E, bound)) return rc;
  PhaseTimer timer(t->stream, testing_value(GS_TESTING_TRIANGLE_PROFILE, 0) == 1, t->rphase_us, 3);
  timer.mark(0);
  const gs::TriAdj A = t->adj();
  // 1. D in canonical order into (dx, dy), a dying byte per entry of A
  if (by_age) {
    GS_LAUNCH(gs::launch_tri_mark_old(A, t->seq, folds, t->dead, t->flags, t->blk, t->stream));
    GS_LAUNCH(gs::launch_tile_scan(t->blk, gs::tri_blocks(E), t->ctl + gs::TRI_RNEW, t->stream));
    GS_LAUNCH(gs::launch_tri_compact_new(nullptr, A.x, A.y, E, t->flags, t->blk, t->dx, t->dy, t->r_cap, t->stream));
  } else {
    GS_HIP(hipMemsetAsync(t->dead, 0, E, t->stream));
    GS_LAUNCH(gs::launch_tri_canon(src, dst, n, stride, t->lo, t->hi, t->stream));
    gs::SortSrc cur;
    if (int rc = sort_by_pair(t->sort, t->lo, t->hi, n, &cur, t->stream)) return rc;
    GS_LAUNCH(gs::launch_tri_flag_dying(cur.pay, t->lo, t->hi, n, A, t->flags, t->blk, t->dead, t->stream));
    GS_LAUNCH(gs::launch_tile_scan(t->blk, gs::tri_blocks(n), t->ctl + gs::TRI_RNEW, t->stream));
    GS_LAUNCH(gs::launch_tri_compact_new(cur.pay, t->lo, t->hi, n, t->flags, t->blk, t->dx, t->dy, t->r_cap,
                                         t->stream));
  }
  // where every survivor goes, and the rows without one: known before the host looks
  GS_LAUNCH(gs::launch_tri_live_count(t->dead, E, t->blk, t->stream));
  GS_LAUNCH(gs::launch_tile_scan(t->blk, gs::tri_blocks(E), t->ctl + gs::TRI_RLIVE, t->stream));
  GS_LAUNCH(gs::launch_tri_live_pos(t->dead, E, t->blk, t->pos, t->stream));
  GS_LAUNCH(gs::launch_tri_vanish(A, t->dead, t->pos, t->ctl, t->stream));
  // the removal's one host synchronisation: |D|, the survivors, the vanished vertices
  unsigned long long words[gs::TRI_RLIVE + 1] = {};
  GS_HIP(hipMemcpyAsync(words, t->ctl, sizeof(words), hipMemcpyDeviceToHost, t->stream));
  timer.mark(1);
  GS_HIP(hipStreamSynchronize(t->stream));
  const uint64_t m = words[gs::TRI_RNEW], live = words[gs::TRI_RLIVE], vanished = words[gs::TRI_RVAN];
  if (m > bound || live + 2 * m != E) return fail(GS_ERR_HIP, "triangle removal: the dying entries do not add up");
  if (m == 0) {
    timer.finish();
    return GS_OK;
  }
  const int other = t->cur ^ 1;
  if (int rc = ensure_adj(t, other, live)) return rc;
  // 2. + 3. rows of D's endpoints in A as it stands, then the count, taken away
  const int variant = count_variant();
  GS_LAUNCH(gs::launch_tri_rows_dying(t->table(), t->ctl, A, t->dx, t->dy, m, t->rinfo, t->rlist1, t->rlist2, variant,
                                      t->stream));
  GS_LAUNCH(gs::launch_tri_uncount(t->table(), t->ctl, A, t->dead, t->dx, t->dy, m, t->rinfo, t->rlist1, t->rlist2,
                                   variant, t->stream));
  timer.mark(2);
  // 4. the survivors into the other buffer; |G|, the vertex count and INT64_MIN's flag follow
  gs::TriAdjOut out;
  out.x = t->ax[other];
  out.y = t->ay[other];
  out.seq = t->aseq[other];
  out.cap = t->acap[other];
  GS_LAUNCH(gs::launch_tri_keep(A, t->dead, t->pos, out, t->stream));
  t->cur = other;
  t->entries = live;
  t->edges -= m;
  t->r_edges = m;
  GS_LAUNCH(gs::launch_tri_removed(t->ctl, t->ax[other], live, m, t->stream));
  // 5. no slot of a vanished vertex stays behind
  if (vanished)
    if (int rc = rebuild_table(t)) return rc;
  timer.mark(3);
  timer.finish();
  return GS_OK;
}

int fold_guard(gs_triangles_s* t, const void* src, const void* dst, size_t n) {
  if (n && (!src || !dst)) return fail(GS_ERR_INVALID, "null edge arrays");
  if (2 * (t->edges + (uint64_t)n) > kTriMaxEntries || (uint64_t)n > kTriMaxEntries)
    return fail(GS_ERR_CAPACITY, "triangle adjacency: " + std::to_string(t->edges) + " + " + std::to_string(n) +
                                     " edges could pass 2^32 - 1 entries, the sort payload's range");
  return GS_OK;
}

int remove_guard(const void* src, const void* dst, size_t n) {
  if (n && (!src || !dst)) return fail(GS_ERR_INVALID, "null edge arrays");
  if ((uint64_t)n > kTriMaxEntries)
    return fail(GS_ERR_CAPACITY, "triangle removal: " + std::to_string(n) +
                                     " elements pass 2^32 - 1, the sort payload's range");
  return GS_OK;
}

int export_impl(gs_triangles_s* t, int64_t* v, int64_t* count, size_t cap, size_t* n, int nonzero_only, bool to_host) {
  if (int rc = check_handle(t, kWhat)) return rc;
  if (!n) return fail(GS_ERR_INVALID, "n is null");
  DeviceGuard g(t->device);
  *n = 0;
  if (t->entries == 0) {
    GS_HIP(hipStreamSynchronize(t->stream));
    return GS_OK;
  }
  if (int rc = ensure_flags(t, t->entries)) return rc;
  const gs::TriAdj A = t->adj();
  GS_LAUNCH(gs::launch_tri_flag_heads(t->table(), t->ctl, A, nonzero_only ? 1 : 0, t->flags, t->blk, t->stream));
  GS_LAUNCH(gs::launch_tile_scan(t->blk, gs::tri_blocks(A.n), t->ctl + gs::TRI_ROWS, t->stream));
  unsigned long long rows = 0;
  GS_HIP(hipMemcpyAsync(&rows, t->ctl + gs::TRI_ROWS, 8, hipMemcpyDeviceToHost, t->stream));
  GS_HIP(hipStreamSynchronize(t->stream));
  *n = rows;
  if (cap < rows) return truncated(cap, rows);
  if (rows == 0) return GS_OK;
  if (!v || !count) return fail(GS_ERR_INVALID, "null arrays");
  int64_t *dv = v, *dc = count;
  if (to_host) {
    if (t->o_cap < rows) {  // (not grow_group: the stream is idle, the wait for `rows` above)
      t->o_cap = 0;
      const uint64_t c = rows + rows / 4;
      GS_HIP(alloc_each(c, t->o_v, t->o_c));
      t->o_cap = c;
    }
    dv = t->o_v;
    dc = t->o_c;
  }
  GS_LAUNCH(gs::launch_tri_compact_rows(t->table(), t->ctl, A, t->flags, t->blk, dv, dc, rows, t->stream));
  if (to_host) {
    GS_HIP(hipMemcpyAsync(v, dv, rows * 8, hipMemcpyDeviceToHost, t->stream));
    GS_HIP(hipMemcpyAsync(count, dc, rows * 8, hipMemcpyDeviceToHost, t->stream));
  }
  GS_HIP(hipStreamSynchronize(t->stream));
  return GS_OK;
}

}  // namespace

extern "C" {

int gs_triangle_destroy(gs_triangles t) { return owner_destroy(t); }

int gs_triangle_create(gs_triangles* out, int device, uint64_t edge_hint) {
  if (!out) return fail(GS_ERR_INVALID, "out is null");
  *out = nullptr;
  if (int rc = check_device_index(device)) return rc;
  if (2 * edge_hint > kTriMaxEntries) return fail(GS_ERR_CAPACITY, "edge hint beyond 2^31 - 1 edges");
  return owner_create(out, device, [&](gs_triangles_s* t) -> int {
    GS_HIP(t->ctr.alloc((uint64_t)gs::CTR_COUNT * gs::kCtrStride));
    GS_HIP(hipMemsetAsync(t->ctr, 0, (size_t)gs::CTR_COUNT * gs::kCtrStride * 4, t->stream));
    GS_HIP(t->ctl.alloc(gs::TRI_CTL_WORDS));
    GS_HIP(hipMemsetAsync(t->ctl, 0, gs::TRI_CTL_WORDS * 8, t->stream));
    const uint64_t e = std::max<uint64_t>(edge_hint, kTriMinCap / 2);
    if (int r = alloc_table(t, std::min<uint64_t>(kMaxCap, next_pow2(2 * e)))) return r;
    return ensure_adj(t, 0, 2 * e);
  });
}

int gs_triangle_reset(gs_triangles t) {
  if (int rc = check_handle(t, kWhat)) return rc;
  DeviceGuard g(t->device);
  GS_LAUNCH(gs::launch_tri_init(t->table(), t->stream));
  GS_HIP(hipMemsetAsync(t->ctr, 0, (size_t)gs::CTR_COUNT * gs::kCtrStride * 4, t->stream));
  GS_HIP(hipMemsetAsync(t->ctl, 0, gs::TRI_CTL_WORDS * 8, t->stream));
  t->entries = 0;
  t->edges = 0;
  t->r_edges = 0;
  return GS_OK;
}

int gs_triangle_fold_device(gs_triangles t, const int64_t* src, const int64_t* dst, size_t n, size_t stride) {
  if (int rc = check_handle(t, kWhat)) return rc;
  if (stride == 0 || stride > 0xFFFFFFFFull) return fail(GS_ERR_INVALID, "stride must be >= 1");
  if (int rc = fold_guard(t, src, dst, n)) return rc;
  DeviceGuard g(t->device);
  if (n == 0) return advance_fold(t);
  return fold_impl(t, src, dst, n, stride);
}

int gs_triangle_fold(gs_triangles t, const int64_t* src, const int64_t* dst, size_t n) {
  if (int rc = check_handle(t, kWhat)) return rc;
  if (int rc = fold_guard(t, src, dst, n)) return rc;
  DeviceGuard g(t->device);
  if (n == 0) return advance_fold(t);
  if (int rc = ensure_fold_scratch(t, n)) return rc;
  int64_t *ds = t->stage, *dd = t->stage + t->f_cap;
  GS_HIP(hipMemcpyAsync(ds, src, n * 8, hipMemcpyHostToDevice, t->stream));
  GS_HIP(hipMemcpyAsync(dd, dst, n * 8, hipMemcpyHostToDevice, t->stream));
  if (int rc = fold_impl(t, ds, dd, n, 1)) return rc;
  GS_HIP(hipStreamSynchronize(t->stream));
  return GS_OK;
}

int gs_triangle_remove_device(gs_triangles t, const int64_t* src, const int64_t* dst, size_t n, size_t stride) {
  if (int rc = check_handle(t, kWhat)) return rc;
  if (stride == 0 || stride > 0xFFFFFFFFull) return fail(GS_ERR_INVALID, "stride must be >= 1");
  if (int rc = remove_guard(src, dst, n)) return rc;
  DeviceGuard g(t->device);
  return remove_impl(t, src, dst, n, stride, 0);
}

int gs_triangle_remove(gs_triangles t, const int64_t* src, const int64_t* dst, size_t n) {
  if (int rc = check_handle(t, kWhat)) return rc;
  if (int rc = remove_guard(src, dst, n)) return rc;
  DeviceGuard g(t->device);
  int64_t *ds = nullptr, *dd = nullptr;
  if (n && t->entries) {  // (remove_impl returns before it reads an element otherwise)
    if (int rc = ensure_fold_scratch(t, n)) return rc;
    ds = t->stage;
    dd = t->stage + t->f_cap;
    GS_HIP(hipMemcpyAsync(ds, src, n * 8, hipMemcpyHostToDevice, t->stream));
    GS_HIP(hipMemcpyAsync(dd, dst, n * 8, hipMemcpyHostToDevice, t->stream));
  }
  if (int rc = remove_impl(t, ds, dd, n, 1, 0)) return rc;
  GS_HIP(hipStreamSynchronize(t->stream));
  return GS_OK;
}

int gs_triangle_expire(gs_triangles t, uint64_t folds) {
  if (folds == 0) return fail(GS_ERR_INVALID, "folds must be >= 1");
  if (int rc = check_handle(t, kWhat)) return rc;
  DeviceGuard g(t->device);
  return remove_impl(t, nullptr, nullptr, 0, 1, folds);
}

int gs_triangle_set_refresh(gs_triangles t, int on) {
  if (int rc = check_handle(t, kWhat)) return rc;
  t->refresh = on != 0;
  return GS_OK;
}

int gs_triangle_count(gs_triangles t, uint64_t* triangles, uint64_t* edges, uint64_t* vertices) {
  if (int rc = check_handle(t, kWhat)) return rc;
  if (!triangles || !edges || !vertices) return fail(GS_ERR_INVALID, "null count pointers");
  DeviceGuard g(t->device);
  unsigned long long w[3] = {0, 0, 0};
  GS_HIP(hipMemcpyAsync(w, t->ctl, sizeof(w), hipMemcpyDeviceToHost, t->stream));
  GS_HIP(hipStreamSynchronize(t->stream));
  *triangles = w[gs::TRI_T];
  *edges = w[gs::TRI_E];
  *vertices = w[gs::TRI_NV];
  return GS_OK;
}

int gs_triangle_count_device(gs_triangles t, uint64_t* out) {
  if (int rc = check_handle(t, kWhat)) return rc;
  if (!out) return fail(GS_ERR_INVALID, "out is null");
  DeviceGuard g(t->device);
  GS_HIP(hipMemcpyAsync(out, t->ctl, 24, hipMemcpyDeviceToDevice, t->stream));
  return GS_OK;
}

int gs_triangle_find_device(gs_triangles t, const int64_t* v, size_t n, int64_t* count, uint8_t* found) {
  if (int rc = check_handle(t, kWhat)) return rc;
  if (n && (!v || !count)) return fail(GS_ERR_INVALID, "null arrays");
  DeviceGuard g(t->device);
  GS_LAUNCH(gs::launch_tri_find(t->table(), t->ctl, v, n, count, found, t->stream));
  return GS_OK;
}

int gs_triangle_export_device(gs_triangles t, int64_t* v, int64_t* count, size_t cap, size_t* n, int nonzero_only) {
  return export_impl(t, v, count, cap, n, nonzero_only, false);
}

int gs_triangle_export(gs_triangles t, int64_t* v, int64_t* count, size_t cap, size_t* n, int nonzero_only) {
  return export_impl(t, v, count, cap, n, nonzero_only, true);
}

int gs_triangle_sync(gs_triangles t) { return owner_sync(t, kWhat); }
int gs_triangle_get_stream(gs_triangles t, void** stream) { return owner_get_stream(t, kWhat, stream); }
int gs_triangle_wait_stream(gs_triangles t, void* stream) { return owner_wait_stream(t, kWhat, stream); }

// gs_testing.h: out[0] = intersection steps since reset, out[1] = the longest row a new edge
// met, out[2..5] = microseconds of the last profiled fold's canonise / sort and dedup / merge
// / count phases. Synchronises.
int gs_testing_triangle_stats(void* handle, uint64_t* out) {
  gs_triangles t = static_cast<gs_triangles>(handle);
  if (int rc = check_handle(t, kWhat)) return rc;
  if (!out) return fail(GS_ERR_INVALID, "out is null");
  DeviceGuard g(t->device);
  unsigned long long w[2] = {0, 0};
  GS_HIP(hipMemcpyAsync(w, t->ctl + gs::TRI_STEPS, sizeof(w), hipMemcpyDeviceToHost, t->stream));
  GS_HIP(hipStreamSynchronize(t->stream));
  out[0] = w[0];
  out[1] = w[1];
  for (int i = 0; i < 4; ++i) out[2 + i] = t->phase_us[i];
  return GS_OK;
}

// gs_testing.h: out[0] = edges of the wave list, out[1] = edges of the workgroup list of the
// last fold that had new edges (both 0 under the wave variant and after reset). Synchronises.
int gs_testing_triangle_bins(void* handle, uint64_t* out) {
  gs_triangles t = static_cast<gs_triangles>(handle);
  if (int rc = check_handle(t, kWhat)) return rc;
  if (!out) return fail(GS_ERR_INVALID, "out is null");
  DeviceGuard g(t->device);
  static_assert(gs::TRI_BIN2 == gs::TRI_BIN1 + 1, "the two list lengths are adjacent words");
  unsigned long long w[2] = {0, 0};
  GS_HIP(hipMemcpyAsync(w, t->ctl + gs::TRI_BIN1, sizeof(w), hipMemcpyDeviceToHost, t->stream));
  GS_HIP(hipStreamSynchronize(t->stream));
  out[0] = w[0];
  out[1] = w[1];
  return GS_OK;
}

// gs_testing.h: the last removal (remove, remove_device or expire; all zero but the last two
// words when it removed nothing, and after a reset). Synchronises.
int gs_testing_triangle_remove_stats(void* handle, uint64_t* out) {
  gs_triangles t = static_cast<gs_triangles>(handle);
  if (int rc = check_handle(t, kWhat)) return rc;
  if (!out) return fail(GS_ERR_INVALID, "out is null");
  DeviceGuard g(t->device);
  unsigned long long w[gs::TRI_RLIVE + 1] = {};
  GS_HIP(hipMemcpyAsync(w, t->ctl, sizeof(w), hipMemcpyDeviceToHost, t->stream));
  GS_HIP(hipStreamSynchronize(t->stream));
  const bool any = t->r_edges != 0;
  out[0] = t->r_edges;
  out[1] = any ? w[gs::TRI_RTRI] : 0;
  out[2] = any ? w[gs::TRI_RVAN] : 0;
  out[3] = any ? w[gs::TRI_RBIN1] : 0;
  out[4] = any ? w[gs::TRI_RBIN2] : 0;
  out[5] = any ? w[gs::TRI_RSTEPS] : 0;
  out[6] = t->cap;
  out[7] = t->entries;
  return GS_OK;
}

// gs_testing.h: microseconds of the last profiled removal's mark / count / compact and rebuild phases
int gs_testing_triangle_remove_phases(void* handle, uint64_t* out) {
  gs_triangles t = static_cast<gs_triangles>(handle);
  if (int rc = check_handle(t, kWhat)) return rc;
  if (!out) return fail(GS_ERR_INVALID, "out is null");
  for (int i = 0; i < 3; ++i) out[i] = t->rphase_us[i];
  return GS_OK;
}

// gs_testing.h: the fold number becomes `value` (the next fold takes value + 1)
int gs_testing_triangle_set_fold(void* handle, uint64_t value) {
  gs_triangles t = static_cast<gs_triangles>(handle);
  if (int rc = check_handle(t, kWhat)) return rc;
  if (value > 0xFFFFFFFFull) return fail(GS_ERR_INVALID, "the fold number has 32 bits");
  if (t->entries) return fail(GS_ERR_INVALID, "set the fold number on an empty handle: stamps must not exceed it");
  t->seq = (uint32_t)value;
  return GS_OK;
}

}  // extern "C"
