// gs_spanner.cpp -- the k-spanner summary behind include/gs_summary.h's gs_spanner_* section:
// library/Spanner.java over summaries/AdjacencyListGraph.java. State layout and kernels are
// described in gs_spanner.hpp / gs_spanner_k.hip, the exactness argument of the fold by rounds in
// DESIGN.md section 6f and, executable, in gs_spanner_seq.hpp (SpannerSeq::fold_rounds).
//
// A fold of n arrivals on the graph G0: the filter pass searches every arrival in G0 (within k:
// dropped for good); the survivors, in arrival order, are the pending edges, whose directed
// entries are sorted by (x, y) once; rounds decide them from the statuses of the round before
// (the host reads the heavy and undecided counts of each round); what the rounds leave goes to
// the serial tail; the entries of the accepted edges, already in order, are merged into the
// other adjacency buffer.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "gs_internal.hpp"
#include "gs_spanner.hpp"

using namespace gsi;

struct gs_spanner_s : StreamOwner {
  int k = 3;
  DevBuf<unsigned long long> ctl;  // gs::SpCtl words
  // adjacency: two buffers, the merge of a fold reads one and writes the other
  DevBuf<int64_t> ax[2];
  DevBuf<int64_t> ay[2];
  uint64_t acap[2] = {0, 0};
  int cur = 0;
  uint64_t entries = 0;  // live entries of buffer `cur`
  uint64_t edges = 0;    // |G|, exact after every fold
  // fold scratch for f_cap arrivals (2 f_cap pending entries)
  uint64_t f_cap = 0;
  DevBuf<int64_t> stage;    // [2][f_cap] host folds and host queries
  DevBuf<uint8_t> res;      // the filter's verdicts / a query's answers; later the accepted bytes
  DevBuf<uint32_t> heavy;   // the heavy list of the current launch
  DevBuf<uint32_t> pidx;    // arrival index of pending edge j
  DevBuf<int64_t> ps, pt;   // its endpoints
  DevBuf<int64_t> ex, ey;   // directed entries, unsorted; later the accepted entries in order
  DevBuf<int64_t> px, py;   // directed entries sorted by (x, y)
  DevBuf<uint32_t> pj;      // their pending index (or gs::kSpDead)
  DevBuf<uint8_t> status[2];
  DevBuf<uint32_t> und[2];  // the undecided lists of two consecutive rounds
  SortScratch sort;
  // flag / tile-count scratch of the compactions, sized for g_cap elements
  uint64_t g_cap = 0;
  DevBuf<uint8_t> flags;
  DevBuf<uint32_t> blk;
  // the heavy search's arenas (first use: a search that overflows its on-chip sets, or a tail)
  DevBuf<uint32_t> stamp;
  DevBuf<int64_t> alist;
  uint64_t arena_h = 0;
  uint32_t arena_count = 0;
  uint32_t gen = 0;  // generations used since the stamps were last cleared
  // device staging of the host export and of a combine's source
  OutStage out;  // two columns: lo, hi
  // gs_testing_spanner_stats: the last fold
  uint64_t stats[6] = {0, 0, 0, 0, 0, 0};

  gs::SpGraph base() const {
    gs::SpGraph g;
    g.ax = ax[cur];
    g.ay = ay[cur];
    g.n0 = entries;
    return g;
  }
};

namespace {

// Adjacency and pending entries are row indices of 32 bits (the sort's payload, the lists).
constexpr uint64_t kSpMaxEntries = 0xFFFFFFFEull;
constexpr uint64_t kSpMaxFold = 0x7FFFFFFFull;  // arrivals of one fold: one workgroup each
constexpr uint64_t kSpMinCap = 64;

constexpr const char* kWhat = "spanner";  // check_handle: "null spanner handle"

int check_k(int k) {
  if (k < 1 || k > gs::kSpannerMaxK) return fail(GS_ERR_INVALID, "spanner: k must be in 1..16");
  return GS_OK;
}

uint32_t lds_set() { return gs::sp_clamp_set(testing_value(GS_TESTING_SPANNER_LDS_SET, gs::kSpannerLdsSet)); }

int ensure_adj(gs_spanner_s* s, int side, uint64_t need) {
  if (s->acap[side] >= need) return GS_OK;
  if (need > kSpMaxEntries) return fail(GS_ERR_CAPACITY, "spanner adjacency would pass 2^32 - 2 entries");
  GS_HIP(grow_group(s->stream, s->acap[side], need, std::min<uint64_t>(kSpMaxEntries, need + need / 2),
                    [&](uint64_t c) { return alloc_each(c, s->ax[side], s->ay[side]); }));
  return GS_OK;
}

int ensure_flags(gs_spanner_s* s, uint64_t n) {
  GS_HIP(grow_group(s->stream, s->g_cap, n, n + n / 4, [&](uint64_t c) {
    const hipError_t e = s->flags.alloc(c);
    return e != hipSuccess ? e : s->blk.alloc(gs::sp_blocks(c) + 1);
  }));
  return GS_OK;
}

int ensure_fold_scratch(gs_spanner_s* s, uint64_t n) {
  if (int rc = ensure_flags(s, 2 * n)) return rc;
  if (int rc = sort_scratch_ensure(s->sort, 2 * n, s->stream)) return rc;
  GS_HIP(grow_group(s->stream, s->f_cap, n, n + n / 4, [&](uint64_t c) {
    const hipError_t e = alloc_each(2 * c, s->stage, s->ex, s->ey, s->px, s->py, s->pj);
    return e != hipSuccess ? e : alloc_each(c, s->res, s->heavy, s->pidx, s->ps, s->pt, s->status[0], s->und[0],
                                            s->status[1], s->und[1]);
  }));
  return GS_OK;
}

// The pool with room for H dense vertex numbers per arena and `gens` more generations (one per
// search of the launch, however the searches are dealt to the arenas): *ar names it with gen0
// set, and the generations are taken.
int take_arenas(gs_spanner_s* s, uint64_t H, uint64_t gens, gs::SpArenas* ar) {
  const uint32_t want = (uint32_t)std::min<int64_t>(
      64, std::max<int64_t>(1, testing_value(GS_TESTING_SPANNER_ARENAS, gs::kSpannerArenas)));
  H = std::max<uint64_t>(H, 1);
  if (s->arena_h < H || s->arena_count != want) {
    GS_HIP(hipStreamSynchronize(s->stream));
    s->arena_h = 0;
    s->arena_count = 0;
    const uint64_t c = H + H / 2;
    GS_HIP(s->stamp.alloc(c * want));
    GS_HIP(s->alist.alloc(2 * c * want));
    s->arena_h = c;
    s->arena_count = want;
    s->gen = gs::kSpMaxGen;  // (cleared below)
  }
  if ((uint64_t)s->gen + gens >= gs::kSpMaxGen) {
    if (gens >= gs::kSpMaxGen) return fail(GS_ERR_CAPACITY, "spanner: too many searches for one launch");
    GS_HIP(hipMemsetAsync(s->stamp, 0, s->arena_h * s->arena_count * 4, s->stream));
    s->gen = 0;
  }
  ar->stamp = s->stamp;
  ar->list = s->alist;
  ar->H = s->arena_h;
  ar->count = s->arena_count;
  ar->gen0 = s->gen;
  s->gen += (uint32_t)gens;
  return GS_OK;
}

int read_words(gs_spanner_s* s, int first, int count, unsigned long long* out) {
  GS_HIP(hipMemcpyAsync(out, s->ctl + first, (size_t)count * 8, hipMemcpyDeviceToHost, s->stream));
  GS_HIP(hipStreamSynchronize(s->stream));
  return GS_OK;
}

int check_err(gs_spanner_s* s) {
  unsigned long long e = 0;
  if (int rc = read_words(s, gs::SP_ERR, 1, &e)) return rc;
  if (e) return fail(GS_ERR_HIP, "spanner: a heavy search ran out of its arena");
  return GS_OK;
}

// out[i] = within(src[i * stride], dst[i * stride], k) on G for n > 0 device elements (out: n
// device bytes); *nheavy (optional) += the searches that took the heavy path
int query_impl(gs_spanner_s* s, const int64_t* src, const int64_t* dst, uint64_t n, uint64_t stride, int k,
               uint8_t* out, uint64_t* nheavy) {
  const gs::SpGraph g = s->base();
  GS_HIP(hipMemsetAsync(s->ctl + gs::SP_HEAVY, 0, 8, s->stream));
  GS_LAUNCH(gs::launch_sp_query(g, src, dst, n, stride, k, out, s->heavy, s->ctl, lds_set(), s->stream));
  unsigned long long h = 0;
  if (int rc = read_words(s, gs::SP_HEAVY, 1, &h)) return rc;
  if (h > n) return fail(GS_ERR_HIP, "spanner: heavy list longer than its launch");
  if (h) {
    gs::SpArenas ar;
    if (int rc = take_arenas(s, g.n0, h, &ar)) return rc;
    GS_LAUNCH(gs::launch_sp_query_heavy(g, src, dst, n, stride, k, out, s->heavy, h, s->ctl, ar, s->stream));
    if (nheavy) *nheavy += h;
  }
  return GS_OK;
}

// n > 0 device elements src[i * stride], dst[i * stride] on s->stream; on return s->res[i] is
// the accepted byte of arrival i (queued, not waited for beyond the fold's own reads)
int fold_impl(gs_spanner_s* s, const int64_t* src, const int64_t* dst, uint64_t n, uint64_t stride, int k) {
  if (int rc = ensure_fold_scratch(s, n)) return rc;
  hipStream_t st = s->stream;
  uint64_t* S = s->stats;
  std::fill(S, S + 6, 0);
  GS_HIP(hipMemsetAsync(s->ctl + gs::SP_ROWMAX, 0, 8, st));
  // 1. the filter pass
  if (int rc = query_impl(s, src, dst, n, stride, k, s->res, &S[4])) return rc;
  // 2. the pending edges, in arrival order
  GS_LAUNCH(gs::launch_sp_flag_pending(s->res, n, s->flags, s->blk, st));
  GS_LAUNCH(gs::launch_tile_scan(s->blk, gs::sp_blocks(n), s->ctl + gs::SP_PEND, st));
  GS_LAUNCH(gs::launch_sp_pending(src, dst, n, stride, s->flags, s->blk, s->pidx, s->ps, s->pt, s->ex, s->ey, s->und[0],
                                  s->f_cap, st));
  GS_HIP(hipMemsetAsync(s->res, 0, n, st));  // from here on: the accepted bytes
  unsigned long long np = 0;
  if (int rc = read_words(s, gs::SP_PEND, 1, &np)) return rc;
  if (np > n) return fail(GS_ERR_HIP, "spanner fold: more pending edges than arrivals");
  S[0] = n - np;
  S[1] = np;
  if (np == 0) return check_err(s);
  // 3. their entries sorted by (x, y): by y, then stably by x
  const uint64_t ne = 2 * np;
  gs::SortSrc cur;
  if (int rc = sort_by_pair(s->sort, s->ex, s->ey, ne, &cur, st)) return rc;
  GS_LAUNCH(gs::launch_sp_gather(cur.pay, s->ex, s->ey, ne, s->px, s->py, s->pj, st));
  GS_HIP(hipMemsetAsync(s->status[0], 0, np, st));
  // 4. rounds
  gs::SpGraph g = s->base();
  g.px = s->px;
  g.py = s->py;
  g.pj = s->pj;
  g.np = ne;
  const int64_t cap_knob = testing_value(GS_TESTING_SPANNER_ROUND_CAP, -1);
  const uint64_t round_cap = cap_knob < 0 ? gs::kSpannerRoundCap : (uint64_t)cap_knob;
  int sc = 0;  // the status buffer (and undecided list) the next round reads
  uint64_t und = np, rounds = 0;
  while (und && rounds < round_cap) {
    GS_HIP(hipMemcpyAsync(s->status[sc ^ 1], s->status[sc], np, hipMemcpyDeviceToDevice, st));
    GS_HIP(hipMemsetAsync(s->ctl + gs::SP_HEAVY, 0, 16, st));
    g.status = s->status[sc];
    GS_LAUNCH(gs::launch_sp_round(g, s->ps, s->pt, s->und[sc], und, k, s->status[sc ^ 1], s->und[sc ^ 1], s->heavy,
                                  s->ctl, lds_set(), st));
    unsigned long long w[2] = {0, 0};
    if (int rc = read_words(s, gs::SP_HEAVY, 2, w)) return rc;
    if (w[0] > und) return fail(GS_ERR_HIP, "spanner round: heavy list longer than its launch");
    if (w[0]) {
      gs::SpArenas ar;
      if (int rc = take_arenas(s, g.n0 + ne, 2 * w[0], &ar)) return rc;
      GS_LAUNCH(gs::launch_sp_round_heavy(g, s->ps, s->pt, s->heavy, w[0], k, s->status[sc ^ 1], s->und[sc ^ 1], s->ctl,
                                          ar, st));
      if (int rc = read_words(s, gs::SP_UND, 1, w + 1)) return rc;
      S[4] += w[0];
    }
    if (w[1] >= und) return fail(GS_ERR_HIP, "spanner round: no edge decided");
    const bool slow = cap_knob < 0 && gs::sp_slow_round(und, w[1]);  // (a set cap fixes the rounds)
    und = w[1];
    sc ^= 1;
    ++rounds;
    if (slow) break;
  }
  S[2] = rounds;
  // 5. the tail
  if (und) {
    gs::SpArenas ar;
    if (int rc = take_arenas(s, g.n0 + ne, und, &ar)) return rc;
    g.status = s->status[sc];
    GS_LAUNCH(gs::launch_sp_tail(g, s->ps, s->pt, np, k, s->status[sc], s->ctl, ar, st));
    S[3] = und;
  }
  // 6. the accepted edges: their bytes, their entries (in order already), the merge
  GS_HIP(hipMemsetAsync(s->ctl + gs::SP_ENT, 0, 16, st));
  GS_LAUNCH(gs::launch_sp_mark(s->status[sc], s->pidx, np, s->res, s->ctl, st));
  GS_LAUNCH(gs::launch_sp_flag_accepted(s->pj, s->status[sc], ne, s->flags, s->blk, st));
  GS_LAUNCH(gs::launch_tile_scan(s->blk, gs::sp_blocks(ne), s->ctl + gs::SP_ENT, st));
  GS_LAUNCH(gs::launch_sp_compact_pairs(s->px, s->py, ne, s->flags, s->blk, s->ex, s->ey, 2 * s->f_cap, st));
  unsigned long long w[2] = {0, 0};
  if (int rc = read_words(s, gs::SP_ENT, 2, w)) return rc;
  const uint64_t nd = w[0], m = w[1];
  if (nd > ne || m > np || m == 0) return fail(GS_ERR_HIP, "spanner fold: accepted counts out of range");
  const int other = s->cur ^ 1;
  if (int rc = ensure_adj(s, other, s->entries + nd)) return rc;
  GS_LAUNCH(gs::launch_sp_merge(s->ax[s->cur], s->ay[s->cur], s->entries, s->ex, s->ey, nd, s->ax[other], s->ay[other],
                                s->acap[other], st));
  s->cur = other;
  s->entries += nd;
  s->edges += m;
  GS_HIP(hipMemsetAsync(s->ctl + gs::SP_VERT, 0, 8, st));
  GS_LAUNCH(gs::launch_sp_count_rows(s->ax[s->cur], s->entries, s->ctl + gs::SP_VERT, st));
  unsigned long long rm = 0;
  if (int rc = read_words(s, gs::SP_ROWMAX, 1, &rm)) return rc;
  S[5] = rm;
  return check_err(s);
}

int fold_guard(gs_spanner_s* s, const void* src, const void* dst, size_t n) {
  if (n && (!src || !dst)) return fail(GS_ERR_INVALID, "null edge arrays");
  if ((uint64_t)n > kSpMaxFold || s->entries + 2 * (uint64_t)n > kSpMaxEntries)
    return fail(GS_ERR_CAPACITY, "spanner adjacency: " + std::to_string(s->edges) + " + " + std::to_string(n) +
                                     " edges could pass 2^32 - 2 entries, the sort payload's range");
  return GS_OK;
}

// the edges ascending by (lo, hi): the entries with x <= y, in the adjacency's order
int export_impl(gs_spanner_s* s, int64_t* lo, int64_t* hi, size_t cap, size_t* n, bool to_host) {
  if (int rc = check_handle(s, kWhat)) return rc;
  if (!n) return fail(GS_ERR_INVALID, "n is null");
  DeviceGuard g(s->device);
  *n = s->edges;
  GS_HIP(hipStreamSynchronize(s->stream));
  if (cap < s->edges) return truncated(cap, s->edges);
  if (s->edges == 0) return GS_OK;
  if (!lo || !hi) return fail(GS_ERR_INVALID, "null arrays");
  if (int rc = ensure_flags(s, s->entries)) return rc;
  if (to_host) GS_HIP(s->out.ensure(2, s->edges, s->stream));
  GS_LAUNCH(gs::launch_sp_flag_edges(s->ax[s->cur], s->ay[s->cur], s->entries, s->flags, s->blk, s->stream));
  GS_LAUNCH(gs::launch_tile_scan(s->blk, gs::sp_blocks(s->entries), s->ctl + gs::SP_ROWS, s->stream));
  GS_LAUNCH(gs::launch_sp_compact_pairs(s->ax[s->cur], s->ay[s->cur], s->entries, s->flags, s->blk,
                                        s->out.dev(0, lo, to_host), s->out.dev(1, hi, to_host), s->edges, s->stream));
  if (to_host) GS_HIP(s->out.finish(s->stream, s->edges, lo, hi));
  else GS_HIP(hipStreamSynchronize(s->stream));  // (the device form waits too)
  return GS_OK;
}

// to_host: src, dst and out are host arrays (staged through s->stage, answered through s->res)
int within_impl(gs_spanner s, const int64_t* src, const int64_t* dst, size_t n, int k, uint8_t* out, bool to_host) {
  if (int rc = check_handle(s, kWhat)) return rc;
  if (int rc = check_k(k)) return rc;
  if (n && (!src || !dst || !out)) return fail(GS_ERR_INVALID, "null arrays");
  if ((uint64_t)n > kSpMaxFold) return fail(GS_ERR_CAPACITY, "spanner: too many queries for one call");
  if (n == 0) return GS_OK;
  DeviceGuard g(s->device);
  if (int rc = ensure_fold_scratch(s, n)) return rc;  // (the heavy list)
  if (to_host) {
    int64_t *ds = s->stage, *dd = s->stage + s->f_cap;
    GS_HIP(hipMemcpyAsync(ds, src, n * 8, hipMemcpyHostToDevice, s->stream));
    GS_HIP(hipMemcpyAsync(dd, dst, n * 8, hipMemcpyHostToDevice, s->stream));
    src = ds;
    dst = dd;
  }
  if (int rc = query_impl(s, src, dst, n, 1, k, to_host ? s->res.get() : out, nullptr)) return rc;
  if (to_host) GS_HIP(hipMemcpyAsync(out, s->res, n, hipMemcpyDeviceToHost, s->stream));
  return check_err(s);
}

}  // namespace

extern "C" {

int gs_spanner_destroy(gs_spanner s) { return owner_destroy(s); }

int gs_spanner_create(gs_spanner* out, int device, int k, uint64_t edge_hint) {
  if (!out) return fail(GS_ERR_INVALID, "out is null");
  *out = nullptr;
  if (int rc = check_k(k)) return rc;
  if (int rc = check_device_index(device)) return rc;
  if (2 * edge_hint > kSpMaxEntries) return fail(GS_ERR_CAPACITY, "edge hint beyond 2^31 - 1 edges");
  return owner_create(out, device, [&](gs_spanner_s* s) -> int {
    s->k = k;
    GS_HIP(s->ctl.alloc(gs::SP_CTL_WORDS));
    GS_HIP(hipMemsetAsync(s->ctl, 0, gs::SP_CTL_WORDS * 8, s->stream));
    return ensure_adj(s, 0, 2 * std::max<uint64_t>(edge_hint, kSpMinCap / 2));
  });
}

int gs_spanner_reset(gs_spanner s) {
  if (int rc = check_handle(s, kWhat)) return rc;
  DeviceGuard g(s->device);
  GS_HIP(hipMemsetAsync(s->ctl, 0, gs::SP_CTL_WORDS * 8, s->stream));
  s->entries = 0;
  s->edges = 0;
  std::fill(s->stats, s->stats + 6, 0);
  return GS_OK;
}

int gs_spanner_fold_device(gs_spanner s, const int64_t* src, const int64_t* dst, size_t n, uint8_t* accepted,
                           size_t stride) {
  if (int rc = check_handle(s, kWhat)) return rc;
  if (stride == 0 || stride > 0xFFFFFFFFull) return fail(GS_ERR_INVALID, "stride must be >= 1");
  if (int rc = fold_guard(s, src, dst, n)) return rc;
  if (n == 0) return GS_OK;
  DeviceGuard g(s->device);
  if (int rc = fold_impl(s, src, dst, n, stride, s->k)) return rc;
  if (accepted) GS_HIP(hipMemcpyAsync(accepted, s->res, n, hipMemcpyDeviceToDevice, s->stream));
  return GS_OK;
}

namespace {
int fold_host(gs_spanner s, const int64_t* src, const int64_t* dst, size_t n, uint8_t* accepted, int k) {
  if (int rc = fold_guard(s, src, dst, n)) return rc;
  if (n == 0) return GS_OK;
  DeviceGuard g(s->device);
  if (int rc = ensure_fold_scratch(s, n)) return rc;
  int64_t *ds = s->stage, *dd = s->stage + s->f_cap;
  GS_HIP(hipMemcpyAsync(ds, src, n * 8, hipMemcpyHostToDevice, s->stream));
  GS_HIP(hipMemcpyAsync(dd, dst, n * 8, hipMemcpyHostToDevice, s->stream));
  if (int rc = fold_impl(s, ds, dd, n, 1, k)) return rc;
  if (accepted) GS_HIP(hipMemcpyAsync(accepted, s->res, n, hipMemcpyDeviceToHost, s->stream));
  GS_HIP(hipStreamSynchronize(s->stream));
  return GS_OK;
}
}  // namespace

int gs_spanner_fold(gs_spanner s, const int64_t* src, const int64_t* dst, size_t n, uint8_t* accepted) {
  if (int rc = check_handle(s, kWhat)) return rc;
  return fold_host(s, src, dst, n, accepted, s->k);
}

// AdjacencyListGraph.addEdge over a batch: an edge joins G unless G holds it already, which is
// the fold with k = 1 (within 1 edge = the edge, or the loop, is there).
int gs_spanner_add(gs_spanner s, const int64_t* src, const int64_t* dst, size_t n) {
  if (int rc = check_handle(s, kWhat)) return rc;
  return fold_host(s, src, dst, n, nullptr, 1);
}

int gs_spanner_within_device(gs_spanner s, const int64_t* src, const int64_t* dst, size_t n, int k, uint8_t* out) {
  return within_impl(s, src, dst, n, k, out, false);
}

int gs_spanner_within(gs_spanner s, const int64_t* src, const int64_t* dst, size_t n, int k, uint8_t* out) {
  return within_impl(s, src, dst, n, k, out, true);
}

int gs_spanner_combine(gs_spanner into, gs_spanner from) {
  if (int rc = check_handle(into, kWhat)) return rc;
  if (int rc = check_handle(from, kWhat)) return rc;
  if (into->device != from->device) return fail(GS_ERR_INVALID, "spanner combine: handles on different devices");
  DeviceGuard g(into->device);
  const uint64_t m = from->edges;
  if (m == 0) return GS_OK;
  // from's edges ascending by (lo, hi) in from's own staging; the fold reads them on into's stream
  GS_HIP(from->out.ensure(2, m, from->stream));
  int64_t *const lo = from->out.column[0], *const hi = from->out.column[1];
  if (int rc = fold_guard(into, lo, hi, m)) return rc;
  size_t got = 0;
  if (int rc = export_impl(from, lo, hi, m, &got, false)) return rc;
  if (int rc = fold_impl(into, lo, hi, m, 1, into->k)) return rc;
  GS_HIP(hipStreamSynchronize(into->stream));
  return GS_OK;
}

int gs_spanner_count(gs_spanner s, uint64_t* edges, uint64_t* vertices) {
  if (int rc = check_handle(s, kWhat)) return rc;
  if (!edges || !vertices) return fail(GS_ERR_INVALID, "null count pointers");
  DeviceGuard g(s->device);
  unsigned long long v = 0;
  if (int rc = read_words(s, gs::SP_VERT, 1, &v)) return rc;
  *edges = s->edges;
  *vertices = v;
  return GS_OK;
}

int gs_spanner_export_device(gs_spanner s, int64_t* lo, int64_t* hi, size_t cap, size_t* n) {
  return export_impl(s, lo, hi, cap, n, false);
}

int gs_spanner_export(gs_spanner s, int64_t* lo, int64_t* hi, size_t cap, size_t* n) {
  return export_impl(s, lo, hi, cap, n, true);
}

int gs_spanner_neighbors(gs_spanner s, int64_t* v, uint64_t* offset, int64_t* neighbor, size_t cap_v, size_t cap_e,
                         size_t* nv, size_t* ne) {
  if (int rc = check_handle(s, kWhat)) return rc;
  if (!nv || !ne) return fail(GS_ERR_INVALID, "null count pointers");
  DeviceGuard g(s->device);
  unsigned long long verts = 0;
  if (int rc = read_words(s, gs::SP_VERT, 1, &verts)) return rc;
  *nv = verts;
  *ne = s->entries;
  if (cap_v < verts || cap_e < s->entries)
    return fail(GS_ERR_TRUNCATED, "output capacity " + std::to_string(cap_v) + " / " + std::to_string(cap_e) + " < " +
                                      std::to_string(verts) + " / " + std::to_string(s->entries));
  if (!offset) return fail(GS_ERR_INVALID, "null arrays");
  offset[0] = 0;
  if (s->entries == 0) return GS_OK;
  if (!v || !neighbor) return fail(GS_ERR_INVALID, "null arrays");
  // the y column is the neighbour array as it stands; the rows of the x column give v and offset
  std::vector<int64_t> x(s->entries);
  GS_HIP(hipMemcpyAsync(x.data(), s->ax[s->cur], s->entries * 8, hipMemcpyDeviceToHost, s->stream));
  GS_HIP(hipMemcpyAsync(neighbor, s->ay[s->cur], s->entries * 8, hipMemcpyDeviceToHost, s->stream));
  GS_HIP(hipStreamSynchronize(s->stream));
  uint64_t r = 0;
  for (uint64_t i = 0; i < s->entries; ++i)
    if (i == 0 || x[i - 1] != x[i]) {
      if (r >= verts) return fail(GS_ERR_HIP, "spanner: more rows than vertices");
      v[r] = x[i];
      offset[r++] = i;
    }
  offset[r] = s->entries;
  return GS_OK;
}

int gs_spanner_sync(gs_spanner s) { return owner_sync(s, kWhat); }
int gs_spanner_get_stream(gs_spanner s, void** stream) { return owner_get_stream(s, kWhat, stream); }
int gs_spanner_wait_stream(gs_spanner s, void* stream) { return owner_wait_stream(s, kWhat, stream); }

// gs_testing.h: the last fold. No device call.
int gs_testing_spanner_stats(void* handle, uint64_t* out) {
  gs_spanner s = static_cast<gs_spanner>(handle);
  if (int rc = check_handle(s, kWhat)) return rc;
  if (!out) return fail(GS_ERR_INVALID, "out is null");
  for (int i = 0; i < 6; ++i) out[i] = s->stats[i];
  return GS_OK;
}

// gs_testing.h: the generation counter of the heavy search's arenas, read and (set >= 0) moved,
// so that a test reaches the clear of take_arenas without 2^31 searches. No device call.
int gs_testing_spanner_generation(void* handle, int64_t set, uint64_t* out) {
  gs_spanner s = static_cast<gs_spanner>(handle);
  if (int rc = check_handle(s, kWhat)) return rc;
  if (!out) return fail(GS_ERR_INVALID, "out is null");
  if (set >= 0) s->gen = (uint32_t)std::min<int64_t>(set, gs::kSpMaxGen);
  *out = s->gen;
  return GS_OK;
}

}  // extern "C"
