// gs_matching.cpp -- the weighted matching summary behind include/gs_summary.h's gs_matching_*
// section: example/CentralizedWeightedMatching.java with util/MatchingEvent.java. State layout
// and kernels are described in gs_matching.hpp / gs_matching_k.hip, the exactness argument of
// the fold by rounds in DESIGN.md section 6g and, executable, in gs_matching_seq.hpp
// (MatchingRounds).
//
// A fold of n arrivals: growth is decided first from host-known totals (worst case + 2 n
// vertices), so nothing grows inside the fold; the distinct streams' vertex phase
// (launch_dist_vertices) gives every new id its rank; the gather reads the ranks; rounds run
// while the pending arrivals are many (the host reads two words per round: the pending count and
// the error word); the tail finishes; the event rows are counted, the counts read (the fold's
// last wait), the rows written.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "gs_internal.hpp"
#include "gs_matching.hpp"
#include "gs_vtable.hpp"

using namespace gsi;

struct gs_matching_s : StreamOwner, VertexTable {  // (the vertex table and the vertices in rank order)
  DevBuf<unsigned long long> ctl;   // gs::MtCtl words
  DevBuf<unsigned long long> dctl;  // gs::DistCtl words of the vertex phase
  DevBuf<gs::MtVertex> st;          // [dist_vid_cap(vcap)] the state record of every rank
  // fold scratch for n_cap arrivals
  uint64_t n_cap = 0;
  DevBuf<uint32_t> vslot;  // [2 n] slot of every entry
  DevBuf<uint8_t> flags;   // whole tiles of 2 n positions (the vertex phase)
  DevBuf<uint32_t> tbase;  // [tiles + 1]: the vertex phase's tile counts, then the event rows'
  DevBuf<uint32_t> entry;  // [2 n] entries of the new vertices (the vertex phase writes them)
  DevBuf<uint32_t> ru, rv;
  DevBuf<int64_t> w;
  DevBuf<uint8_t> mark, acc;
  DevBuf<gs::MtRec> rec;
  DevBuf<uint32_t> list[2];
  // device staging of a host fold
  FoldStage stage;  // (src, dst, val)
  // the last fold's events
  uint64_t ev_cap = 0, ev_rows = 0;
  bool ev_kept = true;  // false after a fold the library cut into pieces
  DevBuf<uint32_t> ev_arrival;
  DevBuf<uint8_t> ev_type;
  DevBuf<int64_t> ev_src, ev_dst, ev_val;
  // export: compacted (stamp, rank) rows, the sort's scratch, staging of the host-array form
  SortScratch sort;
  uint64_t x_cap = 0;
  DevBuf<int64_t> x_stamp;
  DevBuf<uint32_t> x_rank;
  OutStage out;  // four columns
  // mate probe
  uint64_t q_cap = 0;
  DevBuf<int64_t> q_rank;
  // host-known totals (nv: VertexTable)
  uint64_t folded = 0, edges = 0;
  int64_t weight = 0;
  bool safe = true;
  // gs_testing_matching_tune (< 0: product) and gs_testing_matching_stats
  int64_t tune[3] = {-1, -1, -1};
  uint64_t stats[5] = {0, 0, 0, 0, 0};
};

namespace {

constexpr const char* kWhat = "matching";  // check_handle: "null matching handle"

// The vertex table grows (VertexTable::grow) and the state records with it, inside the same wait.
int grow_vertices(gs_matching_s* m, uint64_t cap) {
  DevBuf<gs::MtVertex> st;
  const uint64_t ranks = gs::dist_vid_cap(cap);
  const int rc = m->grow(cap, m->dctl, m->stream, [&](bool rebuild) -> int {
    GS_HIP(st.alloc(ranks));
    GS_LAUNCH(gs::launch_mt_init(st, rebuild ? m->nv : 0, ranks, m->stream));
    if (rebuild && m->nv)
      GS_HIP(hipMemcpyAsync(st, m->st, m->nv * sizeof(gs::MtVertex), hipMemcpyDeviceToDevice, m->stream));
    return GS_OK;
  });
  if (rc) return rc;
  m->st.swap(st);
  return GS_OK;
}

int ensure_scratch(gs_matching_s* m, uint64_t n) {
  static_assert(2 * gs::MATCHING_TILE == gs::DISTINCT_TILE, "tbase serves both compactions: n / 1024 tiles");
  const auto alloc_scratch = [&](uint64_t c) {
    const uint64_t tiles = gs::dist_tiles(2 * c, gs::DISTINCT_TILE);
    hipError_t e = alloc_each(2 * c, m->vslot, m->entry);
    if (e == hipSuccess) e = m->flags.alloc(tiles * gs::DISTINCT_TILE);
    if (e == hipSuccess) e = m->tbase.alloc(tiles + 1);
    if (e == hipSuccess) e = alloc_each(c, m->ru, m->rv, m->w, m->mark, m->acc, m->rec, m->list[0], m->list[1]);
    return e;
  };
  GS_HIP(grow_group(m->stream, m->n_cap, n, std::min<uint64_t>(gs::kMtMaxFold, n + n / 4), alloc_scratch));
  return GS_OK;
}

int ensure_events(gs_matching_s* m, uint64_t rows) {
  GS_HIP(grow_group(m->stream, m->ev_cap, rows, rows + rows / 4, [&](uint64_t c) {
    return alloc_each(c, m->ev_arrival, m->ev_type, m->ev_src, m->ev_dst, m->ev_val);
  }));
  return GS_OK;
}

int fold_guard(gs_matching_s* m, const void* src, const void* dst, const void* val, size_t n) {
  if (n && (!src || !dst || !val)) return fail(GS_ERR_INVALID, "null edge arrays");
  return m->fold_guard_vertices(n, std::min<uint64_t>(n, gs::kMtMaxFold), kWhat);
}

// 0 < n <= kMtMaxFold device arrivals on m->stream; on return m->acc[i] is the accepted byte of
// arrival i and the event rows are queued
int fold_piece(gs_matching_s* m, const int64_t* src, const int64_t* dst, const int64_t* val, uint64_t n,
               uint64_t stride) {
  hipStream_t st = m->stream;
  if (int rc = m->ensure_for(n, [&](uint64_t slots) { return grow_vertices(m, slots); })) return rc;
  if (int rc = ensure_scratch(m, n)) return rc;
  const gs::DistVTable vt = m->vtable();
  const uint64_t ranks = gs::dist_vid_cap(m->vcap);
  // ranks
  GS_HIP(hipMemsetAsync(m->dctl, 0, gs::DIST_CTL_WORDS * 8, st));
  GS_LAUNCH(gs::launch_dist_vertices(src, dst, n, stride, vt, m->vslot, m->flags, m->tbase, m->nv, m->vid, ranks,
                                     m->entry, m->dctl, st));
  static_assert(gs::MT_UNSAFE == 2 && gs::kMtFoldWords == 10, "the fold's words lie around MT_UNSAFE");
  GS_HIP(hipMemsetAsync(m->ctl, 0, gs::MT_UNSAFE * 8, st));
  GS_HIP(hipMemsetAsync(m->ctl + gs::MT_UNSAFE + 1, 0, (gs::kMtFoldWords - gs::MT_UNSAFE - 1) * 8, st));
  GS_LAUNCH(gs::launch_mt_gather(m->vslot, vt, ranks, val, stride, n, m->ru, m->rv, m->w, m->list[0], m->acc, m->ctl,
                                 st));
  gs::MtFold F;
  F.st = m->st;
  F.ru = m->ru;
  F.rv = m->rv;
  F.w = m->w;
  F.mark = m->mark;
  F.accepted = m->acc;
  F.rec = m->rec;
  F.base = m->folded;
  F.n = (uint32_t)n;
  F.sharpen = 0;  // (the kernels set it from `sharpen` and ctl[MT_UNSAFE])
  const int sharpen = m->tune[2] > 0 ? 0 : 1;
  const uint32_t iter_cap = (uint32_t)std::min<int64_t>(
      gs::kMatchingMaxIterCap, std::max<int64_t>(1, m->tune[1] < 0 ? (int64_t)gs::kMatchingIterCap : m->tune[1]));
  // rounds: a set cap fixes their number alone; the product also hands a short list to the tail
  const bool fixed = m->tune[0] >= 0;
  const uint64_t round_cap = fixed ? (uint64_t)m->tune[0] : gs::kMatchingRoundCap;
  uint64_t np = n, rounds = 0;
  int side = 0;
  while (np && rounds < round_cap && (fixed || np >= gs::kMatchingTailThreshold)) {
    GS_LAUNCH(gs::launch_mt_round(F, m->list[side], np, m->list[side ^ 1], iter_cap, sharpen, m->ctl, st));
    unsigned long long w2[2] = {0, 0};
    GS_HIP(hipMemcpyAsync(w2, m->ctl + gs::MT_NEXT, sizeof(w2), hipMemcpyDeviceToHost, st));
    GS_HIP(hipStreamSynchronize(st));
    if (w2[1]) return fail(GS_ERR_HIP, "matching fold: a rank or list index out of range (the handle's state is undefined)");
    if (w2[0] >= np) return fail(GS_ERR_HIP, "matching round: no arrival decided");
    np = w2[0];
    side ^= 1;
    ++rounds;
  }
  const uint64_t tail = np;
  if (np) {
    GS_LAUNCH(gs::launch_mt_tail(F, m->list[side], m->list[side ^ 1], np, iter_cap, sharpen, m->ctl, st));
  }
  // events: rows per tile, their scan, the counts (the fold's last wait), the rows
  const uint64_t nt = gs::mt_tiles(n);
  GS_LAUNCH(gs::launch_mt_event_count(m->acc, m->rec, m->w, n, m->tbase, m->ctl, st));
  GS_LAUNCH(gs::launch_tile_scan(m->tbase, nt, m->ctl + gs::MT_ROWS, st));
  unsigned long long c[gs::kMtFoldWords], d[gs::DIST_CTL_WORDS];
  GS_HIP(hipMemcpyAsync(c, m->ctl, sizeof(c), hipMemcpyDeviceToHost, st));
  GS_HIP(hipMemcpyAsync(d, m->dctl, sizeof(d), hipMemcpyDeviceToHost, st));
  GS_HIP(hipStreamSynchronize(st));
  if (d[gs::DIST_OVERFLOW]) return fail(GS_ERR_HIP, "matching fold: the vertex table overflowed (the handle's state is undefined)");
  if (c[gs::MT_ERR]) return fail(GS_ERR_HIP, "matching fold: a rank or list index out of range (the handle's state is undefined)");
  if (d[gs::DIST_NEW_V] > 2 * n || c[gs::MT_ACC] > n || c[gs::MT_ROWS] > 3 * n)
    return fail(GS_ERR_HIP, "matching fold: counts out of range");
  m->nv += d[gs::DIST_NEW_V];
  m->folded += n;
  m->edges += c[gs::MT_EDGES];  // (wrapping: the change may be negative)
  m->weight = gs::mt_wrap_add(m->weight, (int64_t)c[gs::MT_WEIGHT]);
  m->safe = c[gs::MT_UNSAFE] == 0;
  m->stats[0] = rounds + c[gs::MT_TAIL_ROUNDS];
  m->stats[1] = c[gs::MT_ITERS];
  m->stats[2] = tail;
  m->stats[3] = c[gs::MT_ACC];
  m->stats[4] = c[gs::MT_FALLBACKS];
  m->ev_rows = c[gs::MT_ROWS];
  if (m->ev_rows) {
    if (int rc = ensure_events(m, m->ev_rows)) return rc;
    GS_LAUNCH(gs::launch_mt_event_write(m->acc, m->rec, m->ru, m->rv, m->w, n, m->tbase, m->vid, m->nv, m->ev_arrival,
                                        m->ev_type, m->ev_src, m->ev_dst, m->ev_val, m->ev_cap, st));
  }
  return GS_OK;
}

void forget_last(gs_matching_s* m) {
  std::fill(m->stats, m->stats + 5, 0);
  m->ev_rows = 0;
  m->ev_kept = true;
}

// the whole fold, cut into pieces of at most kMtMaxFold arrivals; host: the arrays are HOST arrays
int fold_all(gs_matching_s* m, const int64_t* src, const int64_t* dst, const int64_t* val, size_t n,
             uint8_t* accepted, uint64_t stride, bool host) {
  forget_last(m);
  if (n == 0) return GS_OK;
  DeviceGuard g(m->device);
  uint64_t sum[5] = {0, 0, 0, 0, 0};
  for (uint64_t at = 0; at < n; at += gs::kMtMaxFold) {
    const uint64_t len = std::min<uint64_t>(gs::kMtMaxFold, n - at);
    const int64_t* col[3] = {src + at * stride, dst + at * stride, val + at * stride};
    if (host) GS_HIP(m->stage.put(m->stream, len, gs::kMtMaxFold, col));
    if (int rc = fold_piece(m, col[0], col[1], col[2], len, host ? 1 : stride)) return rc;
    if (accepted)
      GS_HIP(hipMemcpyAsync(accepted + at, m->acc, len, host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice,
                            m->stream));
    for (int i = 0; i < 5; ++i) sum[i] += m->stats[i];
  }
  if (n > gs::kMtMaxFold) {
    std::copy(sum, sum + 5, m->stats);
    m->ev_rows = 0;
    m->ev_kept = false;
  }
  if (host) GS_HIP(hipStreamSynchronize(m->stream));
  return GS_OK;
}

int events_impl(gs_matching_s* m, uint32_t* arrival, uint8_t* type, int64_t* src, int64_t* dst, int64_t* val,
                size_t cap, size_t* n, bool to_host) {
  if (int rc = check_handle(m, kWhat)) return rc;
  if (!n) return fail(GS_ERR_INVALID, "n is null");
  DeviceGuard g(m->device);
  if (!m->ev_kept) return fail(GS_ERR_INVALID, "matching events: the last fold was cut into pieces, its events were not kept");
  const uint64_t rows = m->ev_rows;
  *n = rows;
  if (cap < rows) return truncated(cap, rows);
  if (rows == 0) return GS_OK;
  const ColumnCopy copy(m->stream, to_host);
  GS_HIP(copy.col(arrival, m->ev_arrival.get(), rows));
  GS_HIP(copy.col(type, m->ev_type.get(), rows));
  GS_HIP(copy.col(src, m->ev_src.get(), rows));
  GS_HIP(copy.col(dst, m->ev_dst.get(), rows));
  GS_HIP(copy.col(val, m->ev_val.get(), rows));
  GS_HIP(copy.done());
  return GS_OK;
}

// scan the state, compact the source vertices of M's edges, sort by stamp, decode
int export_impl(gs_matching_s* m, int64_t* src, int64_t* dst, int64_t* val, uint64_t* first, size_t cap, size_t* n,
                bool to_host) {
  if (int rc = check_handle(m, kWhat)) return rc;
  if (!n) return fail(GS_ERR_INVALID, "n is null");
  DeviceGuard g(m->device);
  const uint64_t ne = m->edges;
  *n = ne;
  if (cap < ne) return truncated(cap, ne);
  if (ne == 0) return GS_OK;
  GS_HIP(grow_group(m->stream, m->x_cap, ne, ne + ne / 4,
                    [&](uint64_t c) { return alloc_each(c, m->x_stamp, m->x_rank); }));
  if (int rc = sort_scratch_ensure(m->sort, ne, m->stream)) return rc;
  if (to_host) GS_HIP(m->out.ensure(4, ne, m->stream));
  GS_HIP(hipMemsetAsync(m->ctl + gs::MT_EXPORT, 0, 8, m->stream));
  GS_LAUNCH(gs::launch_mt_export(m->st, m->nv, m->x_stamp, m->x_rank, ne, m->ctl, m->stream));
  // every stamp is below folded (not 0: M has edges): the digits above its bits are equal in all keys
  bool skip[gs::kSortPasses];
  sort_skip_above(m->folded, skip);
  gs::SortSrc cur;
  if (int rc = sort_by_key(m->sort, m->x_stamp, ne, skip, &cur, m->stream, "matching export")) return rc;
  GS_LAUNCH(gs::launch_mt_decode(cur.key, cur.pay, m->x_rank, ne, m->st, m->vid, m->nv, m->out.dev(0, src, to_host),
                                 m->out.dev(1, dst, to_host), m->out.dev(2, val, to_host),
                                 m->out.dev(3, reinterpret_cast<unsigned long long*>(first), to_host), m->stream));
  if (to_host) GS_HIP(m->out.finish(m->stream, ne, src, dst, val, first));
  return GS_OK;
}

}  // namespace

extern "C" {

int gs_matching_destroy(gs_matching m) { return owner_destroy(m); }

int gs_matching_create(gs_matching* out, int device, uint64_t vertex_hint) {
  if (!out) return fail(GS_ERR_INVALID, "out is null");
  *out = nullptr;
  if (vertex_hint > gs::kDistMaxVertices || gs::dist_slots_for(vertex_hint) > gs::kDistMaxSlots)
    return fail(GS_ERR_CAPACITY, "matching create: the hint passes 2^31 table slots");
  if (int rc = check_device_index(device)) return rc;
  return owner_create(out, device, [&](gs_matching_s* m) -> int {
    GS_HIP(m->ctl.alloc(gs::MT_CTL_WORDS));
    GS_HIP(hipMemsetAsync(m->ctl, 0, gs::MT_CTL_WORDS * 8, m->stream));
    GS_HIP(m->dctl.alloc(gs::DIST_CTL_WORDS));
    GS_HIP(hipMemsetAsync(m->dctl, 0, gs::DIST_CTL_WORDS * 8, m->stream));
    return grow_vertices(m, gs::dist_slots_for(vertex_hint));
  });
}

int gs_matching_reset(gs_matching m) {
  if (int rc = check_handle(m, kWhat)) return rc;
  DeviceGuard g(m->device);
  GS_LAUNCH(gs::launch_dist_init(m->vtable(), m->stream));
  GS_LAUNCH(gs::launch_mt_init(m->st, 0, gs::dist_vid_cap(m->vcap), m->stream));
  GS_HIP(hipMemsetAsync(m->ctl, 0, gs::MT_CTL_WORDS * 8, m->stream));
  m->nv = m->folded = m->edges = 0;
  m->weight = 0;
  m->safe = true;
  forget_last(m);
  return GS_OK;
}

int gs_matching_fold_device(gs_matching m, const int64_t* src, const int64_t* dst, const int64_t* val, size_t n,
                            uint8_t* accepted, size_t stride) {
  if (int rc = check_handle(m, kWhat)) return rc;
  if (stride == 0 || stride > 0xFFFFFFFFull) return fail(GS_ERR_INVALID, "stride must be >= 1");
  if (int rc = fold_guard(m, src, dst, val, n)) return rc;
  return fold_all(m, src, dst, val, n, accepted, stride, false);
}

int gs_matching_fold(gs_matching m, const int64_t* src, const int64_t* dst, const int64_t* val, size_t n,
                     uint8_t* accepted) {
  if (int rc = check_handle(m, kWhat)) return rc;
  if (int rc = fold_guard(m, src, dst, val, n)) return rc;
  return fold_all(m, src, dst, val, n, accepted, 1, true);
}

int gs_matching_events_device(gs_matching m, uint32_t* arrival, uint8_t* type, int64_t* src, int64_t* dst,
                              int64_t* val, size_t cap, size_t* n) {
  return events_impl(m, arrival, type, src, dst, val, cap, n, false);
}

int gs_matching_events(gs_matching m, uint32_t* arrival, uint8_t* type, int64_t* src, int64_t* dst, int64_t* val,
                       size_t cap, size_t* n) {
  return events_impl(m, arrival, type, src, dst, val, cap, n, true);
}

int gs_matching_count(gs_matching m, uint64_t* edges, uint64_t* vertices_seen, int64_t* weight) {
  if (int rc = check_handle(m, kWhat)) return rc;
  if (!edges || !vertices_seen || !weight) return fail(GS_ERR_INVALID, "null count pointers");
  *edges = m->edges;
  *vertices_seen = m->nv;
  *weight = m->weight;
  return GS_OK;
}

int gs_matching_export_device(gs_matching m, int64_t* src, int64_t* dst, int64_t* val, uint64_t* first, size_t cap,
                              size_t* n) {
  return export_impl(m, src, dst, val, first, cap, n, false);
}

int gs_matching_export(gs_matching m, int64_t* src, int64_t* dst, int64_t* val, uint64_t* first, size_t cap,
                       size_t* n) {
  return export_impl(m, src, dst, val, first, cap, n, true);
}

int gs_matching_mate_device(gs_matching m, const int64_t* v, size_t n, int64_t* mate, int64_t* val, uint8_t* found) {
  if (int rc = check_handle(m, kWhat)) return rc;
  if (n == 0) return GS_OK;
  if (!v) return fail(GS_ERR_INVALID, "null arrays");
  DeviceGuard g(m->device);
  GS_HIP(grow_group(m->stream, m->q_cap, n, n + n / 4, [&](uint64_t c) { return m->q_rank.alloc(c); }));
  GS_LAUNCH(gs::launch_dist_rank(m->vtable(), v, n, m->q_rank, nullptr, m->stream));
  GS_LAUNCH(gs::launch_mt_mate(m->q_rank, n, m->st, m->vid, m->nv, mate, val, found, m->stream));
  return GS_OK;
}

int gs_matching_sync(gs_matching m) { return owner_sync(m, kWhat); }
int gs_matching_get_stream(gs_matching m, void** stream) { return owner_get_stream(m, kWhat, stream); }
int gs_matching_wait_stream(gs_matching m, void* stream) { return owner_wait_stream(m, kWhat, stream); }

// gs_testing.h: the last fold. No device call.
int gs_testing_matching_stats(void* handle, uint64_t* out) {
  gs_matching m = static_cast<gs_matching>(handle);
  if (int rc = check_handle(m, kWhat)) return rc;
  if (!out) return fail(GS_ERR_INVALID, "out is null");
  for (int i = 0; i < 5; ++i) out[i] = m->stats[i];
  out[5] = m->safe ? 1 : 0;
  return GS_OK;
}

int gs_testing_matching_tune(void* handle, int what, int64_t value) {
  gs_matching m = static_cast<gs_matching>(handle);
  if (int rc = check_handle(m, kWhat)) return rc;
  if (what < 0 || what > 2) return fail(GS_ERR_INVALID, "matching tune: unknown control");
  m->tune[what] = value < 0 ? -1 : value;
  return GS_OK;
}

}  // extern "C"
