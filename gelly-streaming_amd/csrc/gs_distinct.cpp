// gs_distinct.cpp -- the distinct streams behind include/gs_summary.h's gs_distinct_* section:
// the first-seen vertices and edges of an edge stream (SimpleEdgeStream.distinct / getVertices),
// the first-appearance rank of every vertex, and the whole sets in arrival order. State layout
// and the kernels are described in gs_distinct.hpp / gs_distinct_k.hip and DESIGN.md section 6e.
//
// A fold of n edges: growth is decided first, from host-known totals (worst case + 2 n vertices,
// + n edges), so no table grows inside the fold; then the vertex phase (probe and stamp; flag,
// scan, write), the edge phase (the same shape over rank pairs) and ONE host synchronisation to
// read the two new counts and the overflow flag. A fold that grows a table or its scratch waits
// once more, before the old arrays are freed.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "gs_distinct.hpp"
#include "gs_internal.hpp"
#include "gs_vtable.hpp"

using namespace gsi;

struct gs_distinct_s : StreamOwner, VertexTable {  // (the vertex table and the vertex list: vtab, vid, vcap)
  int mode = GS_DISTINCT_DIRECTED;
  DevBuf<unsigned long long> ctl;  // gs::DistCtl words
  DevBuf<gs::DistESlot> etab;      // [ecap] the edge table
  uint64_t ecap = 0;
  // the last fold's scratch and emissions, sized for n_cap edges
  uint64_t n_cap = 0;
  DevBuf<uint32_t> vslot;       // [2 n] slot of every entry
  DevBuf<uint32_t> eslot;       // [n] slot of every edge
  DevBuf<uint8_t> flags;        // whole tiles of 2 n positions
  DevBuf<uint32_t> tbase;       // [tiles + 1]
  DevBuf<uint32_t> newv_entry;  // [2 n] entries of the new vertices
  DevBuf<uint32_t> newe_index;  // [n] indices of the kept edges
  // device staging of a host fold
  FoldStage stage;  // (src, dst)
  // host-known totals (nv: VertexTable)
  uint64_t ne = 0, folded = 0;
  uint64_t last_n = 0, last_nv = 0, last_ne = 0;
  // edge export: compacted (stamp, key) rows, the sort's scratch, staging of the host-array forms
  SortScratch sort;
  uint64_t x_cap = 0;
  DevBuf<int64_t> x_stamp;
  DevBuf<unsigned long long> x_key;
  OutStage out;  // three columns
  // diagnostics (gs_testing_distinct_stats)
  uint64_t v_rebuilds = 0, e_rebuilds = 0, last_probe = 0, last_tiles = 0;
  uint64_t phase_us[5] = {0, 0, 0, 0, 0};  // of the last profiled fold (gs_testing_distinct_phases)
  uint64_t last_atomics = 0;

  gs::DistETable etable() const { return etable_of(etab, ecap); }
  static gs::DistETable etable_of(gs::DistESlot* tab, uint64_t cap) {
    gs::DistETable t;
    t.tab = tab;
    t.cap = (uint32_t)cap;
    t.mask = (uint32_t)(cap - 1);
    t.shift = 64 - gs::dist_log2(cap);
    return t;
  }
};

namespace {

constexpr const char* kWhat = "distinct";  // check_handle: "null distinct handle"

int grow_vertices(gs_distinct_s* d, uint64_t cap) {
  const bool rebuild = d->vtab;
  if (int rc = d->grow(cap, d->ctl, d->stream, [](bool) { return GS_OK; })) return rc;
  if (rebuild) ++d->v_rebuilds;
  return GS_OK;
}

int grow_edges(gs_distinct_s* d, uint64_t cap) {
  DevBuf<gs::DistESlot> tab;
  GS_HIP(tab.alloc(cap));
  const gs::DistETable to = gs_distinct_s::etable_of(tab, cap);
  GS_LAUNCH(gs::launch_dist_init(to, d->stream));
  if (d->etab) {
    GS_LAUNCH(gs::launch_dist_rebuild(d->etable(), to, d->ctl, d->stream));
    GS_HIP(hipStreamSynchronize(d->stream));
    ++d->e_rebuilds;
  }
  d->etab.swap(tab);
  d->ecap = cap;
  return GS_OK;
}

int ensure_scratch(gs_distinct_s* d, uint64_t n) {
  const auto alloc_scratch = [&](uint64_t c) {
    const uint64_t tiles = gs::dist_tiles(2 * c, gs::DISTINCT_TILE);
    hipError_t e = alloc_each(2 * c, d->vslot, d->newv_entry);
    if (e == hipSuccess) e = alloc_each(c, d->eslot, d->newe_index);
    if (e == hipSuccess) e = d->flags.alloc(tiles * gs::DISTINCT_TILE);
    if (e == hipSuccess) e = d->tbase.alloc(tiles + 1);
    return e;
  };
  GS_HIP(grow_group(d->stream, d->n_cap, n, std::min<uint64_t>(gs::kDistMaxFold, n + n / 4), alloc_scratch));
  return GS_OK;
}

void forget_last(gs_distinct_s* d) {
  d->last_n = d->last_nv = d->last_ne = d->last_probe = d->last_tiles = d->last_atomics = 0;
  for (uint64_t& us : d->phase_us) us = 0;
}

int fold_guard(gs_distinct d, const void* src, const void* dst, size_t n) {
  if (int rc = check_handle(d, kWhat)) return rc;
  if (n && (!src || !dst)) return fail(GS_ERR_INVALID, "null edge arrays");
  if ((uint64_t)n > gs::kDistMaxFold)
    return fail(GS_ERR_CAPACITY, "distinct fold: " + std::to_string(n) + " edges pass 2^31 - 2 per fold");
  // the worst case of this fold, before any device work
  const uint64_t need_v = d->nv + gs::dist_worst_vertices(n), need_e = d->ne + gs::dist_worst_edges(n);
  if (need_v > gs::kDistMaxVertices)
    return fail(GS_ERR_CAPACITY, "distinct fold: the fold may pass 2^32 - 2 distinct vertices");
  if ((gs::dist_must_grow(d->nv, gs::dist_worst_vertices(n), d->vcap) && gs::dist_slots_for(need_v) > gs::kDistMaxSlots) ||
      (gs::dist_must_grow(d->ne, gs::dist_worst_edges(n), d->ecap) && gs::dist_slots_for(need_e) > gs::kDistMaxSlots))
    return fail(GS_ERR_CAPACITY, "distinct fold: a table would pass 2^31 slots");
  return GS_OK;
}

// n > 0 device edges on d->stream
int fold_impl(gs_distinct_s* d, const int64_t* src, const int64_t* dst, uint64_t n, uint64_t stride) {
  forget_last(d);
  static_assert(gs::DIST_PROBE == 3 && gs::DIST_ATOMICS == 5, "the fold's words are among the first six");
  GS_HIP(hipMemsetAsync(d->ctl, 0, 6 * 8, d->stream));
  if (int rc = d->ensure_for(n, [&](uint64_t slots) { return grow_vertices(d, slots); })) return rc;
  if (gs::dist_must_grow(d->ne, gs::dist_worst_edges(n), d->ecap))
    if (int rc = grow_edges(d, gs::dist_slots_for(d->ne + gs::dist_worst_edges(n)))) return rc;
  if (int rc = ensure_scratch(d, n)) return rc;
  const gs::DistVTable vt = d->vtable();
  const gs::DistETable et = d->etable();
  PhaseTimer timer(d->stream, testing_value(GS_TESTING_DISTINCT_PROFILE, 0) == 1, d->phase_us, 5);
  timer.mark(0);
  GS_LAUNCH(gs::launch_dist_vertices(src, dst, n, stride, vt, d->vslot, d->flags, d->tbase, d->nv, d->vid,
                                     gs::dist_vid_cap(d->vcap), d->newv_entry, d->ctl, d->stream, timer.event(1)));
  timer.mark(2);
  GS_LAUNCH(gs::launch_dist_edges(n, d->folded, d->mode, vt, d->vslot, et, d->eslot, d->flags, d->tbase, d->newe_index,
                                  d->ctl, d->stream, timer.event(3)));
  timer.mark(4);
  // the fold's one host synchronisation: new vertices, new edges, overflow, longest probe
  unsigned long long w[6] = {0, 0, 0, 0, 0, 0};
  GS_HIP(hipMemcpyAsync(w, d->ctl, sizeof(w), hipMemcpyDeviceToHost, d->stream));
  timer.mark(5);
  GS_HIP(hipStreamSynchronize(d->stream));
  timer.finish();
  d->last_atomics = w[gs::DIST_ATOMICS];
  if (w[gs::DIST_OVERFLOW]) return fail(GS_ERR_HIP, "distinct fold: a table overflowed (the handle's state is undefined)");
  if (w[gs::DIST_NEW_V] > 2 * n || w[gs::DIST_NEW_E] > n) return fail(GS_ERR_HIP, "distinct fold: counts out of range");
  d->nv += w[gs::DIST_NEW_V];
  d->ne += w[gs::DIST_NEW_E];
  d->folded += n;
  d->last_n = n;
  d->last_nv = w[gs::DIST_NEW_V];
  d->last_ne = w[gs::DIST_NEW_E];
  d->last_probe = w[gs::DIST_PROBE];
  d->last_tiles = gs::dist_tiles(n, gs::DISTINCT_TILE);
  return GS_OK;
}

int new_edges_impl(gs_distinct_s* d, uint32_t* index, int64_t* src, int64_t* dst, size_t cap, size_t* n, bool to_host) {
  if (int rc = check_handle(d, kWhat)) return rc;
  if (!n) return fail(GS_ERR_INVALID, "n is null");
  DeviceGuard g(d->device);
  const uint64_t ne = d->last_ne;
  *n = ne;
  if (cap < ne) return truncated(cap, ne);
  if (ne == 0) return GS_OK;
  if (to_host && (src || dst)) GS_HIP(d->out.ensure(3, ne, d->stream));
  if (src || dst) {
    GS_LAUNCH(gs::launch_dist_new_edges(d->newe_index, ne, d->eslot, d->last_n, d->etable(), d->vid, d->nv,
                                        d->out.dev(0, src, to_host), d->out.dev(1, dst, to_host), d->stream));
  }
  GS_HIP(ColumnCopy(d->stream, to_host).col(index, d->newe_index.get(), ne));
  if (to_host) GS_HIP(d->out.finish(d->stream, ne, src, dst));
  return GS_OK;
}

int new_vertices_impl(gs_distinct_s* d, int64_t* v, uint32_t* entry, size_t cap, size_t* n, bool to_host) {
  if (int rc = check_handle(d, kWhat)) return rc;
  if (!n) return fail(GS_ERR_INVALID, "n is null");
  DeviceGuard g(d->device);
  const uint64_t k = d->last_nv;
  *n = k;
  if (cap < k) return truncated(cap, k);
  if (k == 0) return GS_OK;
  const ColumnCopy copy(d->stream, to_host);
  GS_HIP(copy.col(v, d->vid + (d->nv - k), k));  // the new vertices are the tail of the vertex list
  GS_HIP(copy.col(entry, d->newv_entry.get(), k));
  GS_HIP(copy.done());
  return GS_OK;
}

int vertices_impl(gs_distinct_s* d, int64_t* v, size_t cap, size_t* n, bool to_host) {
  if (int rc = check_handle(d, kWhat)) return rc;
  if (!n) return fail(GS_ERR_INVALID, "n is null");
  DeviceGuard g(d->device);
  *n = d->nv;
  if (cap < d->nv) return truncated(cap, d->nv);
  if (d->nv == 0) return GS_OK;
  if (!v) return fail(GS_ERR_INVALID, "null arrays");
  const ColumnCopy copy(d->stream, to_host);
  GS_HIP(copy.col(v, d->vid.get(), d->nv));
  GS_HIP(copy.done());
  return GS_OK;
}

int edges_impl(gs_distinct_s* d, int64_t* src, int64_t* dst, uint64_t* first, size_t cap, size_t* n, bool to_host) {
  if (int rc = check_handle(d, kWhat)) return rc;
  if (!n) return fail(GS_ERR_INVALID, "n is null");
  DeviceGuard g(d->device);
  const uint64_t ne = d->ne;
  *n = ne;
  if (cap < ne) return truncated(cap, ne);
  if (ne == 0) return GS_OK;
  GS_HIP(grow_group(d->stream, d->x_cap, ne, ne + ne / 4,
                    [&](uint64_t c) { return alloc_each(c, d->x_stamp, d->x_key); }));
  if (int rc = sort_scratch_ensure(d->sort, ne, d->stream)) return rc;
  if (to_host) GS_HIP(d->out.ensure(3, ne, d->stream));
  // scan the table, compact, sort by stamp, decode through the vertex list
  GS_HIP(hipMemsetAsync(d->ctl + gs::DIST_EXPORT, 0, 8, d->stream));
  GS_LAUNCH(gs::launch_dist_export(d->etable(), d->x_stamp, d->x_key, ne, d->ctl, d->stream));
  // every stamp is below 2 * folded (not 0: there are edges): the digits above its bits are equal in all keys
  bool skip[gs::kSortPasses];
  sort_skip_above(2 * d->folded, skip);
  gs::SortSrc cur;
  if (int rc = sort_by_key(d->sort, d->x_stamp, ne, skip, &cur, d->stream, "distinct edges")) return rc;
  GS_LAUNCH(gs::launch_dist_decode(cur.key, cur.pay, d->x_key, ne, d->vid, d->nv, d->out.dev(0, src, to_host),
                                   d->out.dev(1, dst, to_host),
                                   d->out.dev(2, reinterpret_cast<unsigned long long*>(first), to_host), d->stream));
  if (to_host) GS_HIP(d->out.finish(d->stream, ne, src, dst, first));
  return GS_OK;
}

}  // namespace

extern "C" {

int gs_distinct_destroy(gs_distinct d) { return owner_destroy(d); }

int gs_distinct_create(gs_distinct* out, int device, int mode, uint64_t vertex_hint, uint64_t edge_hint) {
  if (!out) return fail(GS_ERR_INVALID, "out is null");
  *out = nullptr;
  if (mode < 0 || mode >= gs::kDistModes) return fail(GS_ERR_INVALID, "unknown distinct mode");
  if (vertex_hint > gs::kDistMaxVertices || gs::dist_slots_for(vertex_hint) > gs::kDistMaxSlots ||
      edge_hint > gs::kDistMaxSlots / 2)
    return fail(GS_ERR_CAPACITY, "distinct create: a hint passes 2^31 table slots");
  if (int rc = check_device_index(device)) return rc;
  return owner_create(out, device, [&](gs_distinct_s* d) -> int {
    d->mode = mode;
    GS_HIP(d->ctl.alloc(gs::DIST_CTL_WORDS));
    GS_HIP(hipMemsetAsync(d->ctl, 0, gs::DIST_CTL_WORDS * 8, d->stream));
    if (int rc = grow_vertices(d, gs::dist_slots_for(vertex_hint))) return rc;
    return grow_edges(d, gs::dist_slots_for(edge_hint));
  });
}

int gs_distinct_reset(gs_distinct d) {
  if (int rc = check_handle(d, kWhat)) return rc;
  DeviceGuard g(d->device);
  GS_LAUNCH(gs::launch_dist_init(d->vtable(), d->stream));
  GS_LAUNCH(gs::launch_dist_init(d->etable(), d->stream));
  d->nv = d->ne = d->folded = 0;
  forget_last(d);
  return GS_OK;
}

int gs_distinct_fold_device(gs_distinct d, const int64_t* src, const int64_t* dst, size_t n, size_t stride) {
  if (int rc = fold_guard(d, src, dst, n)) return rc;
  if (stride == 0 || stride > 0xFFFFFFFFull) return fail(GS_ERR_INVALID, "stride must be >= 1");
  if (n == 0) {
    forget_last(d);
    return GS_OK;
  }
  DeviceGuard g(d->device);
  return fold_impl(d, src, dst, n, stride);
}

int gs_distinct_fold(gs_distinct d, const int64_t* src, const int64_t* dst, size_t n) {
  if (int rc = fold_guard(d, src, dst, n)) return rc;
  if (n == 0) {
    forget_last(d);
    return GS_OK;
  }
  DeviceGuard g(d->device);
  const int64_t* col[2] = {src, dst};
  GS_HIP(d->stage.put(d->stream, n, UINT64_MAX, col));  // (one piece: fold_guard bounds n, nothing clamps the growth)
  // (fold_impl waits for the stream before it returns: the host arrays are free then)
  return fold_impl(d, col[0], col[1], n, 1);
}

int gs_distinct_size(gs_distinct d, uint64_t* vertices, uint64_t* edges, uint64_t* folded, uint64_t* new_vertices,
                     uint64_t* new_edges) {
  if (int rc = check_handle(d, kWhat)) return rc;
  if (!vertices || !edges || !folded || !new_vertices || !new_edges)
    return fail(GS_ERR_INVALID, "null count pointers");
  *vertices = d->nv;
  *edges = d->ne;
  *folded = d->folded;
  *new_vertices = d->last_nv;
  *new_edges = d->last_ne;
  return GS_OK;
}

int gs_distinct_new_edges_device(gs_distinct d, uint32_t* index, int64_t* src, int64_t* dst, size_t cap, size_t* n) {
  return new_edges_impl(d, index, src, dst, cap, n, false);
}

int gs_distinct_new_edges(gs_distinct d, uint32_t* index, int64_t* src, int64_t* dst, size_t cap, size_t* n) {
  return new_edges_impl(d, index, src, dst, cap, n, true);
}

int gs_distinct_new_vertices_device(gs_distinct d, int64_t* v, uint32_t* entry, size_t cap, size_t* n) {
  return new_vertices_impl(d, v, entry, cap, n, false);
}

int gs_distinct_new_vertices(gs_distinct d, int64_t* v, uint32_t* entry, size_t cap, size_t* n) {
  return new_vertices_impl(d, v, entry, cap, n, true);
}

int gs_distinct_vertices_device(gs_distinct d, int64_t* v, size_t cap, size_t* n) {
  return vertices_impl(d, v, cap, n, false);
}

int gs_distinct_vertices(gs_distinct d, int64_t* v, size_t cap, size_t* n) {
  return vertices_impl(d, v, cap, n, true);
}

int gs_distinct_edges_device(gs_distinct d, int64_t* src, int64_t* dst, uint64_t* first, size_t cap, size_t* n) {
  return edges_impl(d, src, dst, first, cap, n, false);
}

int gs_distinct_edges(gs_distinct d, int64_t* src, int64_t* dst, uint64_t* first, size_t cap, size_t* n) {
  return edges_impl(d, src, dst, first, cap, n, true);
}

int gs_distinct_rank_device(gs_distinct d, const int64_t* v, size_t n, int64_t* rank, uint8_t* found) {
  if (int rc = check_handle(d, kWhat)) return rc;
  if (n == 0) return GS_OK;
  if (!v || !rank) return fail(GS_ERR_INVALID, "null arrays");
  DeviceGuard g(d->device);
  GS_LAUNCH(gs::launch_dist_rank(d->vtable(), v, n, rank, found, d->stream));
  return GS_OK;
}

int gs_distinct_contains_device(gs_distinct d, const int64_t* src, const int64_t* dst, size_t n, uint8_t* found) {
  if (int rc = check_handle(d, kWhat)) return rc;
  if (n == 0) return GS_OK;
  if (!src || !dst || !found) return fail(GS_ERR_INVALID, "null arrays");
  DeviceGuard g(d->device);
  GS_LAUNCH(gs::launch_dist_contains(d->vtable(), d->etable(), d->mode, src, dst, n, found, d->stream));
  return GS_OK;
}

int gs_distinct_sync(gs_distinct d) { return owner_sync(d, kWhat); }
int gs_distinct_get_stream(gs_distinct d, void** stream) { return owner_get_stream(d, kWhat, stream); }
int gs_distinct_wait_stream(gs_distinct d, void* stream) { return owner_wait_stream(d, kWhat, stream); }

// gs_testing.h: six words, all host-known (no device call)
int gs_testing_distinct_stats(void* handle, uint64_t* out) {
  gs_distinct d = static_cast<gs_distinct>(handle);
  if (int rc = check_handle(d, kWhat)) return rc;
  if (!out) return fail(GS_ERR_INVALID, "out is null");
  out[0] = d->vcap;
  out[1] = d->ecap;
  out[2] = d->v_rebuilds;
  out[3] = d->e_rebuilds;
  out[4] = d->last_probe;
  out[5] = d->last_tiles;
  return GS_OK;
}

// gs_testing.h: seven words of the last profiled fold, all host-known
int gs_testing_distinct_phases(void* handle, uint64_t* out) {
  gs_distinct d = static_cast<gs_distinct>(handle);
  if (int rc = check_handle(d, kWhat)) return rc;
  if (!out) return fail(GS_ERR_INVALID, "out is null");
  for (int i = 0; i < 5; ++i) out[i] = d->phase_us[i];
  out[5] = d->last_atomics;
  out[6] = 3 * d->last_n;
  return GS_OK;
}

}  // extern "C"
