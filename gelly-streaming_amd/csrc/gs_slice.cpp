// gs_slice.cpp -- the window slices behind include/gs_summary.h's gs_slice_* section: the
// per-vertex neighbourhoods of one window of (src, dst, value) edges in arrival order, their
// reduction (reduceOnEdges) and their CSR (foldNeighbors / applyOnNeighbors). State layout and
// the kernels are described in gs_slice.hpp / gs_slice_k.hip and DESIGN.md section 6d.
//
// A window of n edges, E entries: expand the edges into entry keys; digit histograms; eight
// stable radix passes of gs_sort_k.hip over (key, entry index) -- none is skipped, the
// histograms stay on the device; head flags, their scan, vertices and offsets; ONE host
// synchronisation to learn the vertex count. A reduce or an export afterwards queues its
// launches and does not wait (the host-array forms wait for their copies).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "gs_internal.hpp"
#include "gs_slice.hpp"

using namespace gsi;

struct gs_slices_s : StreamOwner {
  DevBuf<unsigned long long> ctl;  // gs::SliceCtl words
  // the window's edges, n_cap each (eval is written only by a window with values)
  uint64_t n_cap = 0;
  DevBuf<int64_t> esrc;
  DevBuf<int64_t> edst;
  DevBuf<int64_t> eval;
  // per entry / per tile arrays, sized for e_cap entries
  uint64_t e_cap = 0;
  DevBuf<int64_t> kid;             // entry keys
  DevBuf<int64_t> vtx;             // vertices, ascending
  DevBuf<unsigned long long> off;  // [e_cap + 1]
  DevBuf<uint8_t> flags;           // whole tiles
  DevBuf<uint32_t> tbase;          // [tiles + 1]
  DevBuf<int64_t> lead;            // [tiles] each: the carry records of the last reduce
  DevBuf<int64_t> trail;
  DevBuf<int64_t> carry;
  SortScratch sort;
  // the current window
  uint64_t n = 0, entries = 0, nv = 0;
  int dir = GS_SLICE_OUT;
  bool has_val = true;
  const unsigned long long* skey = nullptr;  // the sorted pairs (in the sort's scratch)
  const uint32_t* spay = nullptr;
  // device staging of the host-array forms
  OutStage out;  // two columns
  // diagnostics (gs_testing_slice_stats)
  uint64_t reduce_tiles = 0;
  uint64_t phase_us[5] = {0, 0, 0, 0, 0};  // expand, sort, heads, reduce, gather of the last profiled calls
};

namespace {

// A sort payload is an entry index of 32 bits.
constexpr uint64_t kSliceMaxEntries = 0xFFFFFFFFull;
enum { PH_EXPAND = 0, PH_SORT = 1, PH_HEADS = 2, PH_REDUCE = 3, PH_GATHER = 4 };

constexpr const char* kWhat = "slice";  // check_handle: "null slice handle"

int ensure_window(gs_slices_s* s, uint64_t n, uint64_t entries) {
  GS_HIP(grow_group(s->stream, s->n_cap, n, n + n / 4,
                    [&](uint64_t c) { return alloc_each(c, s->esrc, s->edst, s->eval); }));
  const auto alloc_entries = [&](uint64_t c) {
    const uint64_t tiles = gs::slice_tiles(c, gs::SLICE_TILE);
    hipError_t e = alloc_each(c, s->kid, s->vtx);
    if (e == hipSuccess) e = s->off.alloc(c + 1);
    if (e == hipSuccess) e = s->flags.alloc(tiles * gs::SLICE_TILE);
    if (e == hipSuccess) e = s->tbase.alloc(tiles + 1);
    if (e == hipSuccess) e = alloc_each(tiles, s->lead, s->trail, s->carry);
    return e;
  };
  GS_HIP(grow_group(s->stream, s->e_cap, entries, std::min<uint64_t>(kSliceMaxEntries, entries + entries / 4),
                    alloc_entries));
  return sort_scratch_ensure(s->sort, entries, s->stream);
}

// a call's timer over `phases` words of s->phase_us from word `first` on
PhaseTimer phase_timer(gs_slices_s* s, int first, int phases) {
  return PhaseTimer(s->stream, testing_value(GS_TESTING_SLICE_PROFILE, 0) == 1, s->phase_us + first, phases);
}

void set_empty(gs_slices_s* s, int dir) {
  s->n = s->entries = s->nv = 0;
  s->dir = dir;
  s->has_val = true;  // (no value is ever read)
  s->skey = nullptr;
  s->spay = nullptr;
}

int window_guard(gs_slices s, const void* src, const void* dst, size_t n, int dir) {
  if (int rc = check_handle(s, kWhat)) return rc;
  if (dir < 0 || dir >= gs::kSliceDirs) return fail(GS_ERR_INVALID, "unknown slice direction");
  if (n && (!src || !dst)) return fail(GS_ERR_INVALID, "null edge arrays");
  if ((uint64_t)n > kSliceMaxEntries || gs::slice_entries(n, dir) > kSliceMaxEntries)
    return fail(GS_ERR_CAPACITY, "slice window: " + std::to_string(n) +
                                     " edges pass 2^32 - 1 entries, the sort payload's range");
  return GS_OK;
}

// n > 0 device edges on s->stream, arrays of ensure_window(n, entries)
int window_impl(gs_slices_s* s, const int64_t* src, const int64_t* dst, const int64_t* val, uint64_t n,
                uint64_t stride, int dir) {
  const uint64_t entries = gs::slice_entries(n, dir);
  set_empty(s, dir);  // (a failure below leaves an empty window)
  PhaseTimer timer = phase_timer(s, PH_EXPAND, 3);
  timer.mark(PH_EXPAND);
  GS_LAUNCH(gs::launch_slice_expand(src, dst, val, n, stride, dir, s->esrc, s->edst, s->eval, s->kid, s->stream));
  timer.mark(PH_SORT);
  gs::SortSrc cur;
  if (int rc = sort_by_key(s->sort, s->kid, entries, nullptr, &cur, s->stream, "slice window")) return rc;
  timer.mark(PH_HEADS);
  GS_LAUNCH(gs::launch_slice_heads(cur.key, entries, s->flags, s->tbase, s->ctl, s->vtx, s->off, s->e_cap, s->stream));
  // the window's one host synchronisation: the vertex count
  unsigned long long nv = 0;
  GS_HIP(hipMemcpyAsync(&nv, s->ctl + gs::SLICE_NV, 8, hipMemcpyDeviceToHost, s->stream));
  GS_HIP(hipStreamSynchronize(s->stream));
  timer.mark(PH_HEADS + 1);
  timer.finish();
  if (nv == 0 || nv > entries) return fail(GS_ERR_HIP, "slice window: vertex count out of range");
  s->n = n;
  s->entries = entries;
  s->nv = nv;
  s->has_val = val != nullptr;
  s->skey = cur.key;
  s->spay = cur.pay;
  return GS_OK;
}

int reduce_impl(gs_slices_s* s, int op, int64_t* v, int64_t* out, size_t cap, size_t* n, bool to_host) {
  if (int rc = check_handle(s, kWhat)) return rc;
  if (!n) return fail(GS_ERR_INVALID, "n is null");
  if (op < 0 || op >= gs::kSliceOps) return fail(GS_ERR_INVALID, "unknown slice op");
  DeviceGuard g(s->device);
  *n = s->nv;
  if (op != GS_SLICE_COUNT && !s->has_val)
    return fail(GS_ERR_INVALID, "the window has no values: only the count op applies");
  if (cap < s->nv) return truncated(cap, s->nv);
  if (s->nv == 0) return GS_OK;
  if (!v || !out) return fail(GS_ERR_INVALID, "null arrays");
  if (to_host) GS_HIP(s->out.ensure(2, s->nv, s->stream));
  int64_t* const dout = s->out.dev(0, out, to_host);
  PhaseTimer timer = phase_timer(s, PH_REDUCE, 1);
  timer.mark(0);
  if (op == GS_SLICE_COUNT) {
    GS_LAUNCH(gs::launch_slice_count(s->off, s->nv, dout, s->stream));
  } else {
    s->reduce_tiles = gs::slice_tiles(s->entries, gs::SLICE_TILE);
    GS_LAUNCH(gs::launch_slice_reduce(op, s->flags, s->spay, s->eval, s->entries, s->n, s->dir, s->tbase, dout, s->nv,
                                      s->lead, s->trail, s->carry, s->stream));
  }
  timer.mark(1);
  timer.finish();
  GS_HIP(ColumnCopy(s->stream, to_host).col(v, s->vtx.get(), s->nv));
  if (to_host) GS_HIP(s->out.finish(s->stream, s->nv, out));
  return GS_OK;
}

int neighborhoods_impl(gs_slices_s* s, int64_t* v, uint64_t* offset, int64_t* neighbor, int64_t* val, size_t cap_v,
                       size_t cap_e, size_t* nv, size_t* ne, bool to_host) {
  if (int rc = check_handle(s, kWhat)) return rc;
  if (!nv || !ne) return fail(GS_ERR_INVALID, "null count pointers");
  DeviceGuard g(s->device);
  *nv = s->nv;
  *ne = s->entries;
  if (val && !s->has_val) return fail(GS_ERR_INVALID, "the window has no values: pass a null val array");
  if (cap_v < s->nv || cap_e < s->entries)
    return fail(GS_ERR_TRUNCATED, "output capacities " + std::to_string(cap_v) + ", " + std::to_string(cap_e) + " < " +
                                      std::to_string(s->nv) + ", " + std::to_string(s->entries));
  if (!offset) return fail(GS_ERR_INVALID, "null arrays");
  if (s->nv == 0) {  // offset[0] = 0
    if (to_host) offset[0] = 0;
    else GS_HIP(hipMemsetAsync(offset, 0, 8, s->stream));
    return GS_OK;
  }
  if (!v || !neighbor) return fail(GS_ERR_INVALID, "null arrays");
  if (to_host) GS_HIP(s->out.ensure(2, s->entries, s->stream));
  int64_t *const dn = s->out.dev(0, neighbor, to_host), *const dv = s->out.dev(1, val, to_host);
  PhaseTimer timer = phase_timer(s, PH_GATHER, 1);
  timer.mark(0);
  GS_LAUNCH(gs::launch_slice_gather(s->spay, s->entries, s->n, s->dir, s->esrc, s->edst, s->eval, dn, dv, s->entries,
                                    s->stream));
  timer.mark(1);
  timer.finish();
  const ColumnCopy copy(s->stream, to_host);
  GS_HIP(copy.col(v, s->vtx.get(), s->nv));
  GS_HIP(copy.col(reinterpret_cast<unsigned long long*>(offset), s->off.get(), s->nv + 1));
  if (to_host) GS_HIP(s->out.finish(s->stream, s->entries, neighbor, val));
  return GS_OK;
}

}  // namespace

extern "C" {

int gs_slice_destroy(gs_slices s) { return owner_destroy(s); }

int gs_slice_create(gs_slices* out, int device, uint64_t edge_hint) {
  if (!out) return fail(GS_ERR_INVALID, "out is null");
  *out = nullptr;
  if (int rc = check_device_index(device)) return rc;
  if (edge_hint > kSliceMaxEntries) return fail(GS_ERR_CAPACITY, "edge hint beyond 2^32 - 1 entries");
  return owner_create(out, device, [&](gs_slices_s* s) -> int {
    GS_HIP(s->ctl.alloc(gs::SLICE_CTL_WORDS));
    GS_HIP(hipMemsetAsync(s->ctl, 0, gs::SLICE_CTL_WORDS * 8, s->stream));
    return edge_hint ? ensure_window(s, edge_hint, edge_hint) : GS_OK;
  });
}

int gs_slice_window_device(gs_slices s, const int64_t* src, const int64_t* dst, const int64_t* val, size_t n,
                           size_t stride, int dir) {
  if (int rc = window_guard(s, src, dst, n, dir)) return rc;
  if (stride == 0 || stride > 0xFFFFFFFFull) return fail(GS_ERR_INVALID, "stride must be >= 1");
  if (n == 0) {
    set_empty(s, dir);
    return GS_OK;
  }
  DeviceGuard g(s->device);
  if (int rc = ensure_window(s, n, gs::slice_entries(n, dir))) return rc;
  return window_impl(s, src, dst, val, n, stride, dir);
}

int gs_slice_window(gs_slices s, const int64_t* src, const int64_t* dst, const int64_t* val, size_t n, int dir) {
  if (int rc = window_guard(s, src, dst, n, dir)) return rc;
  if (n == 0) {
    set_empty(s, dir);
    return GS_OK;
  }
  DeviceGuard g(s->device);
  if (int rc = ensure_window(s, n, gs::slice_entries(n, dir))) return rc;
  GS_HIP(hipMemcpyAsync(s->esrc, src, n * 8, hipMemcpyHostToDevice, s->stream));
  GS_HIP(hipMemcpyAsync(s->edst, dst, n * 8, hipMemcpyHostToDevice, s->stream));
  if (val) GS_HIP(hipMemcpyAsync(s->eval, val, n * 8, hipMemcpyHostToDevice, s->stream));
  // (the edges are in place; window_impl waits for the stream before it returns)
  return window_impl(s, s->esrc, s->edst, val ? s->eval.get() : nullptr, n, 1, dir);
}

int gs_slice_size(gs_slices s, uint64_t* vertices, uint64_t* entries) {
  if (int rc = check_handle(s, kWhat)) return rc;
  if (!vertices || !entries) return fail(GS_ERR_INVALID, "null count pointers");
  *vertices = s->nv;
  *entries = s->entries;
  return GS_OK;
}

int gs_slice_reduce_device(gs_slices s, int op, int64_t* v, int64_t* out, size_t cap, size_t* n) {
  return reduce_impl(s, op, v, out, cap, n, false);
}

int gs_slice_reduce(gs_slices s, int op, int64_t* v, int64_t* out, size_t cap, size_t* n) {
  return reduce_impl(s, op, v, out, cap, n, true);
}

int gs_slice_neighborhoods_device(gs_slices s, int64_t* v, uint64_t* offset, int64_t* neighbor, int64_t* val,
                                  size_t cap_v, size_t cap_e, size_t* nv, size_t* ne) {
  return neighborhoods_impl(s, v, offset, neighbor, val, cap_v, cap_e, nv, ne, false);
}

int gs_slice_neighborhoods(gs_slices s, int64_t* v, uint64_t* offset, int64_t* neighbor, int64_t* val, size_t cap_v,
                           size_t cap_e, size_t* nv, size_t* ne) {
  return neighborhoods_impl(s, v, offset, neighbor, val, cap_v, cap_e, nv, ne, true);
}

int gs_slice_sync(gs_slices s) { return owner_sync(s, kWhat); }
int gs_slice_get_stream(gs_slices s, void** stream) { return owner_get_stream(s, kWhat, stream); }
int gs_slice_wait_stream(gs_slices s, void* stream) { return owner_wait_stream(s, kWhat, stream); }

// gs_testing.h: out[0] = tiles of the last reduce (0: none, or only the count op), out[1] = tiles
// of the current window without a head (carry records that pass a run on), out[2] = its longest
// segment, out[3..7] = microseconds of the last profiled expand / sort / heads / reduce / gather
// phases. Synchronises.
int gs_testing_slice_stats(void* handle, uint64_t* out) {
  gs_slices s = static_cast<gs_slices>(handle);
  if (int rc = check_handle(s, kWhat)) return rc;
  if (!out) return fail(GS_ERR_INVALID, "out is null");
  DeviceGuard g(s->device);
  unsigned long long w[2] = {0, 0};
  if (s->nv) {
    static_assert(gs::SLICE_NOHEAD == gs::SLICE_LONGEST + 1, "the two diagnostic words are adjacent");
    GS_HIP(hipMemsetAsync(s->ctl + gs::SLICE_LONGEST, 0, 16, s->stream));
    GS_LAUNCH(gs::launch_slice_stats(s->off, s->nv, s->tbase, gs::slice_tiles(s->entries, gs::SLICE_TILE), s->ctl,
                                     s->stream));
    GS_HIP(hipMemcpyAsync(w, s->ctl + gs::SLICE_LONGEST, sizeof(w), hipMemcpyDeviceToHost, s->stream));
  }
  GS_HIP(hipStreamSynchronize(s->stream));
  out[0] = s->reduce_tiles;
  out[1] = w[1];
  out[2] = w[0];
  for (int i = 0; i < 5; ++i) out[3 + i] = s->phase_us[i];
  return GS_OK;
}

}  // extern "C"
