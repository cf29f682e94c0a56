// gs_matching_seq.hpp -- the rules of the weighted matching summary (gs_matching_k.hip,
// gs_matching.cpp): the acceptance test in wrapping arithmetic, the per-vertex state record, the
// cells an arrival reads and writes, the may-accept rule with its sharpening, the weight-safety
// predicate, the phases of a round as plain functions of one pending arrival, and -- host only --
// the sequential definition (MatchingSeq, mt_fold_seq) and a restatement of the fold by rounds
// that calls the very phase functions the kernels call (MatchingRounds, mt_fold_rounds).
// Standard headers only: the kernels include it, and a host compiler builds
// tests/cpp/matching_seq_sanitize.cpp, which checks it against brute force under the address and
// UB sanitizers.
//
// The contract (example/CentralizedWeightedMatching.java:79-106, util/MatchingEvent.java): M is a
// set of edges (src, dst, value), at most one per vertex. An arrival (u, v, w) collides with the
// edges of M at u and at v (one edge that touches both counts once); it is accepted iff
// w > 2 * (sum of their values), in Java long arithmetic; accepted, it removes them and joins M.
//
// The round scheme. S is the committed state, P the pending arrivals of
// the fold, e their index in the fold. A round:
//   reset   T[c] = Rd[c] = far for every cell c of every pending e (mt_cells on S)
//   seed    a(e) = the decision of e on S; an e with a(e) lowers T[c] to e over its cells
//   pass    (to a fixpoint, at most iter_cap times) an e not yet marked whose endpoint is dirty
//           (T < e) and that passes the sharpened test becomes may-accept and lowers T likewise
//   lower   (only when the cap was hit before the fixpoint) every pending e lowers T over its
//           cells: plain deterministic reservations
//   remain  e stays pending iff a(e), or an endpoint is dirty and the sharpened test passes; every
//           other e is rejected for good. A remaining e lowers Rd[u], Rd[v] to e
//   commit  a remaining e with a(e) and e <= T[c], e <= Rd[c] on all its cells commits
// T[c] is a lower bound of the first pending arrival that truly writes c; every truly accepted
// pending arrival is marked (induction on e: its decision differs from a(e) only if an earlier
// truly accepted one wrote u or v, whose true writes lie in cells with T <= its index < e).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GS_MT_HD __host__ __device__ inline
#else
#define GS_MT_HD inline
#endif

namespace gs {

// the values of include/gs_summary.h's gs_matching_event, in the order of MatchingEvent.Type
enum MatchingEventType : uint8_t { kMatchAdd = 0, kMatchRemove = 1 };

// ---- product constants (gsamd.MATCHING_*)
constexpr uint32_t kMatchingRoundCap = 32;          // rounds of a fold before the tail takes the rest
constexpr uint32_t kMatchingTailThreshold = 4096;   // pending arrivals below which the tail takes them
constexpr uint32_t kMatchingIterCap = 6;            // fixpoint passes of a round before plain reservations
constexpr uint32_t kMatchingMaxIterCap = 64;        // (a tuned cap is clamped to 1 .. this)
constexpr int kMatchingSafeBits = 61;               // sharpening holds while every value is in [0, 2^61)

constexpr uint32_t kMtNone = 0xFFFFFFFFu;  // no partner; no removed edge in a record slot
constexpr uint32_t kMtFar = 0xFFFFFFFFu;   // T / Rd: no pending arrival (every index is below)
// arrivals of one device fold (the host cuts longer ones): at most three event rows each, and the
// row count of a fold has 32 bits
constexpr uint64_t kMtMaxFold = 1ull << 30;

// ---- Java long arithmetic
GS_MT_HD int64_t mt_wrap_add(int64_t a, int64_t b) { return (int64_t)((uint64_t)a + (uint64_t)b); }
GS_MT_HD int64_t mt_wrap_sub(int64_t a, int64_t b) { return (int64_t)((uint64_t)a - (uint64_t)b); }
GS_MT_HD int64_t mt_wrap_twice(int64_t a) { return (int64_t)((uint64_t)a << 1); }
// w > 2 * sum, the product wrapping
GS_MT_HD bool mt_accepts(int64_t w, int64_t sum) { return w > mt_wrap_twice(sum); }
// A handle is weight-safe while every value folded since its reset satisfies this: two values
// then sum below 2^62 and twice that below 2^63, so no sum and no product wraps.
GS_MT_HD bool mt_weight_safe(int64_t w) { return w >= 0 && w < ((int64_t)1 << kMatchingSafeBits); }

// ---- the per-vertex state record, indexed by the vertex's rank (32 bytes: one sector)
struct alignas(32) MtVertex {
  uint32_t partner;  // rank of the other endpoint of this vertex's edge of M (itself: a loop), or kMtNone
  uint32_t is_src;   // this vertex is the edge's source (the loop's vertex: 1)
  int64_t value;     // the edge's value
  uint64_t stamp;    // global arrival number at which the edge was accepted
  uint32_t T;        // batch-local: least index of a pending arrival that may write this cell
  uint32_t Rd;       // batch-local: least index of a remaining pending arrival incident to it
};
GS_MT_HD MtVertex mt_vertex_init() {
  MtVertex v;
  v.partner = kMtNone;
  v.is_src = 0;
  v.value = 0;
  v.stamp = 0;
  v.T = kMtFar;
  v.Rd = kMtFar;
  return v;
}

// T and Rd only fall inside a round. On the device: an atomic minimum, and a load that is not
// served from a wave's own cache (the tail's waves read what other waves lowered in the same launch).
GS_MT_HD void mt_lower(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicMin(p, v);
#else
  if (v < *p) *p = v;
#endif
}
GS_MT_HD uint32_t mt_peek(const uint32_t* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  return *p;
#endif
}

// ---- the cells of arrival (u, v) on a state: u, v and their current partners, each once.
// An accepted arrival writes exactly these; its decision reads u and v.
struct MtCells {
  uint32_t c[4];
  uint32_t n;
  uint32_t pu, pv;  // partner of u, of v (kMtNone: unmatched)
};
GS_MT_HD MtCells mt_cells(const MtVertex* st, uint32_t u, uint32_t v) {
  MtCells k;
  k.pu = st[u].partner;
  k.pv = v == u ? k.pu : st[v].partner;
  k.n = 0;
  k.c[k.n++] = u;
  if (v != u) k.c[k.n++] = v;
  if (k.pu != kMtNone && k.pu != u && k.pu != v) k.c[k.n++] = k.pu;
  if (k.pv != kMtNone && k.pv != u && k.pv != v && k.pv != k.pu) k.c[k.n++] = k.pv;
  return k;
}
// does v carry a collision of its own (v is matched, is not u, and its edge is not u's edge)?
GS_MT_HD bool mt_second_collision(uint32_t u, uint32_t v, const MtCells& k) {
  return v != u && k.pv != kMtNone && k.pv != u;
}
// the wrapping sum of the collisions' values
GS_MT_HD int64_t mt_collision_sum(const MtVertex* st, uint32_t u, uint32_t v, const MtCells& k) {
  int64_t s = 0;
  if (k.pu != kMtNone) s = st[u].value;
  if (mt_second_collision(u, v, k)) s = mt_wrap_add(s, st[v].value);
  return s;
}
// Sharpening, weight-safe handles only: a lower bound of the sum arrival e will truly meet --
// the S-values of the matched edges at its clean endpoints (nobody writes a clean endpoint
// before e, so its edge is still there; a dirty endpoint contributes at least 0).
GS_MT_HD int64_t mt_lower_bound(const MtVertex* st, uint32_t u, uint32_t v, const MtCells& k, bool clean_u,
                                bool clean_v) {
  int64_t s = 0;
  if (clean_u && k.pu != kMtNone) s = st[u].value;
  if (v != u && clean_v && k.pv != kMtNone && !(clean_u && k.pv == u)) s += st[v].value;
  return s;
}
// the may-accept rule for an arrival that S rejects
GS_MT_HD bool mt_may_accept(int64_t w, bool dirty_u, bool dirty_v, bool sharpen, int64_t lower_bound) {
  if (!dirty_u && !dirty_v) return false;
  return !sharpen || mt_accepts(w, lower_bound);
}

// ---- one fold's view: what the phase functions work on
struct MtRec {  // what an accepted arrival removed: slot 0 the edge at its source, slot 1 at its target
  uint32_t s0, d0, s1, d1;  // ranks (src, dst) of the removed edges, kMtNone: none
  int64_t v0, v1;
};
enum MtMark : uint8_t { kMtAcceptS = 1, kMtMay = 2 };
struct MtFold {
  MtVertex* st;
  const uint32_t* ru;  // rank of arrival e's source
  const uint32_t* rv;  // ... target
  const int64_t* w;    // its value
  uint8_t* mark;       // MtMark bits
  uint8_t* accepted;   // the fold's output bytes (zero before the rounds)
  MtRec* rec;
  uint64_t base;       // global arrival number of arrival 0
  uint32_t n;          // arrivals of the fold
  int sharpen;        // the handle is weight-safe and sharpening is on
};

GS_MT_HD void mt_lower_cells(const MtFold& F, const MtCells& k, uint32_t e) {
  for (uint32_t i = 0; i < k.n; ++i) mt_lower(&F.st[k.c[i]].T, e);
}

GS_MT_HD void mt_ph_reset(const MtFold& F, uint32_t e) {
  const MtCells k = mt_cells(F.st, F.ru[e], F.rv[e]);
  for (uint32_t i = 0; i < k.n; ++i) {
    F.st[k.c[i]].T = kMtFar;
    F.st[k.c[i]].Rd = kMtFar;
  }
}

GS_MT_HD void mt_ph_seed(const MtFold& F, uint32_t e) {
  const uint32_t u = F.ru[e], v = F.rv[e];
  const MtCells k = mt_cells(F.st, u, v);
  const bool a = mt_accepts(F.w[e], mt_collision_sum(F.st, u, v, k));
  F.mark[e] = a ? (uint8_t)(kMtAcceptS | kMtMay) : (uint8_t)0;
  if (a) mt_lower_cells(F, k, e);
}

// is e, which S rejects, may-accept under the current T?
GS_MT_HD bool mt_dirty_may(const MtFold& F, uint32_t e, uint32_t u, uint32_t v, const MtCells& k) {
  const bool du = mt_peek(&F.st[u].T) < e, dv = mt_peek(&F.st[v].T) < e;
  if (!du && !dv) return false;
  const int64_t lb = F.sharpen ? mt_lower_bound(F.st, u, v, k, !du, !dv) : 0;
  return mt_may_accept(F.w[e], du, dv, F.sharpen != 0, lb);
}

// one fixpoint pass over e: true when e became may-accept now
GS_MT_HD bool mt_ph_pass(const MtFold& F, uint32_t e) {
  if (F.mark[e] & kMtMay) return false;
  const uint32_t u = F.ru[e], v = F.rv[e];
  const MtCells k = mt_cells(F.st, u, v);
  if (!mt_dirty_may(F, e, u, v, k)) return false;
  F.mark[e] |= kMtMay;
  mt_lower_cells(F, k, e);
  return true;
}

// plain reservations: e is a possible writer of its cells whatever it is marked
GS_MT_HD void mt_ph_lower(const MtFold& F, uint32_t e) {
  mt_lower_cells(F, mt_cells(F.st, F.ru[e], F.rv[e]), e);
}

// T is final for the round: does e stay pending? (at a fixpoint this is its kMtMay bit)
GS_MT_HD bool mt_ph_remain(const MtFold& F, uint32_t e) {
  const uint32_t u = F.ru[e], v = F.rv[e];
  const uint8_t m = F.mark[e];
  bool stay = (m & kMtAcceptS) != 0;
  if (!stay) stay = mt_dirty_may(F, e, u, v, mt_cells(F.st, u, v));
  F.mark[e] = stay ? (uint8_t)(m | kMtMay) : (uint8_t)0;
  if (stay) {
    mt_lower(&F.st[u].Rd, e);
    if (v != u) mt_lower(&F.st[v].Rd, e);
  }
  return stay;
}

// Rd is final: commit e if it may; true when e is still pending afterwards
GS_MT_HD bool mt_ph_commit(const MtFold& F, uint32_t e) {
  const uint8_t m = F.mark[e];
  if (!(m & kMtMay)) return false;  // rejected by mt_ph_remain
  if (!(m & kMtAcceptS)) return true;
  const uint32_t u = F.ru[e], v = F.rv[e];
  const MtCells k = mt_cells(F.st, u, v);
  for (uint32_t i = 0; i < k.n; ++i)
    if (mt_peek(&F.st[k.c[i]].T) < e || mt_peek(&F.st[k.c[i]].Rd) < e) return true;
  // no earlier pending arrival writes or reads a cell of e: S is what e truly meets
  MtRec r;
  r.s0 = r.d0 = r.s1 = r.d1 = kMtNone;
  r.v0 = r.v1 = 0;
  if (k.pu != kMtNone) {
    const bool s = F.st[u].is_src != 0;
    r.s0 = s ? u : k.pu;
    r.d0 = s ? k.pu : u;
    r.v0 = F.st[u].value;
  }
  if (mt_second_collision(u, v, k)) {
    const bool s = F.st[v].is_src != 0;
    r.s1 = s ? v : k.pv;
    r.d1 = s ? k.pv : v;
    r.v1 = F.st[v].value;
  }
  if (k.pu != kMtNone) F.st[k.pu].partner = kMtNone;
  if (k.pv != kMtNone) F.st[k.pv].partner = kMtNone;
  const int64_t w = F.w[e];
  F.st[u].partner = v;
  F.st[u].is_src = 1;
  F.st[u].value = w;
  F.st[u].stamp = F.base + e;
  if (v != u) {
    F.st[v].partner = u;
    F.st[v].is_src = 0;
    F.st[v].value = w;
    F.st[v].stamp = F.base + e;
  }
  F.rec[e] = r;
  F.accepted[e] = 1;
  return false;
}

// rows of arrival e in the event stream: its REMOVEs, then its ADD
GS_MT_HD uint32_t mt_event_rows(uint8_t accepted, const MtRec& r) {
  return accepted ? 1u + (r.s0 != kMtNone ? 1u : 0u) + (r.s1 != kMtNone ? 1u : 0u) : 0u;
}

}  // namespace gs

// (the library's own sources want the rules above only: gs_matching.hpp defines the macro)
#if !defined(GS_MATCHING_SEQ_RULES_ONLY)
#include <algorithm>
#include <unordered_map>
#include <vector>

namespace gs {

struct MtEvent {
  uint32_t arrival;
  uint8_t type;
  int64_t src, dst, val;
  bool operator==(const MtEvent& o) const {
    return arrival == o.arrival && type == o.type && src == o.src && dst == o.dst && val == o.val;
  }
};
struct MtEdge {
  int64_t src, dst, val;
  uint64_t first;  // global arrival number of its acceptance
  bool operator==(const MtEdge& o) const { return src == o.src && dst == o.dst && val == o.val && first == o.first; }
};

// The definition: CentralizedWeightedMatching.flatMap over a stream, M kept per vertex.
class MatchingSeq {
 public:
  // arrival (u, v, w) with number `arrival` of its fold; events (optional) receive its rows
  bool step(int64_t u, int64_t v, int64_t w, uint32_t arrival, std::vector<MtEvent>* events) {
    const auto iu = at_.find(u);
    auto iv = at_.find(v);
    const bool cu = iu != at_.end();
    const bool cv = iv != at_.end() && v != u && !(cu && iu->second.mate == v);
    int64_t sum = cu ? iu->second.val : 0;
    if (cv) sum = mt_wrap_add(sum, iv->second.val);
    ++folded_;
    if (!mt_accepts(w, sum)) return false;
    if (cu) remove(u, arrival, events);
    if (cv) remove(v, arrival, events);
    at_[u] = Cell{v, w, true, folded_ - 1};
    if (v != u) at_[v] = Cell{u, w, false, folded_ - 1};
    weight_ = mt_wrap_add(weight_, w);
    ++edges_;
    if (events) events->push_back(MtEvent{arrival, kMatchAdd, u, v, w});
    return true;
  }
  uint64_t edges() const { return edges_; }
  int64_t weight() const { return weight_; }
  uint64_t folded() const { return folded_; }
  // M ascending by acceptance
  std::vector<MtEdge> sorted_edges() const {
    std::vector<MtEdge> out;
    for (const auto& kv : at_)
      if (kv.second.is_src) out.push_back(MtEdge{kv.first, kv.second.mate, kv.second.val, kv.second.first});
    std::sort(out.begin(), out.end(), [](const MtEdge& a, const MtEdge& b) { return a.first < b.first; });
    return out;
  }

 private:
  struct Cell {
    int64_t mate, val;
    bool is_src;
    uint64_t first;
  };
  void remove(int64_t x, uint32_t arrival, std::vector<MtEvent>* events) {
    const Cell c = at_.find(x)->second;
    if (events)
      events->push_back(MtEvent{arrival, kMatchRemove, c.is_src ? x : c.mate, c.is_src ? c.mate : x, c.val});
    at_.erase(x);
    if (c.mate != x) at_.erase(c.mate);
    weight_ = mt_wrap_sub(weight_, c.val);
    --edges_;
  }
  std::unordered_map<int64_t, Cell> at_;
  uint64_t edges_ = 0, folded_ = 0;
  int64_t weight_ = 0;
};

// accepted[i] (optional) = arrival i joined M; returns the accepted count
inline uint64_t mt_fold_seq(MatchingSeq& m, const int64_t* src, const int64_t* dst, const int64_t* val, uint64_t n,
                            uint8_t* accepted, std::vector<MtEvent>* events) {
  uint64_t kept = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const bool a = m.step(src[i], dst[i], val[i], (uint32_t)i, events);
    if (accepted) accepted[i] = a ? 1 : 0;
    kept += a ? 1 : 0;
  }
  return kept;
}

// The fold by rounds as the device runs it, one arrival at a time through the phase functions
// above; ids get their rank at first sight, the state is indexed by rank.
struct MtRoundStats {
  uint64_t rounds = 0, iterations = 0, accepted = 0, fallbacks = 0;
};
class MatchingRounds {
 public:
  uint32_t iter_cap = kMatchingIterCap;
  bool sharpen = true;
  bool weight_safe = true;
  MtRoundStats stats;  // of the last fold

  uint64_t fold(const int64_t* src, const int64_t* dst, const int64_t* val, uint64_t n, uint8_t* accepted,
                std::vector<MtEvent>* events) {
    stats = MtRoundStats();
    std::vector<uint32_t> ru(n), rv(n);
    for (uint64_t i = 0; i < n; ++i) {
      ru[i] = rank_of(src[i]);
      rv[i] = rank_of(dst[i]);
      if (!mt_weight_safe(val[i])) weight_safe = false;
    }
    std::vector<uint8_t> mark(n, 0), acc(n, 0);
    std::vector<MtRec> rec(n);
    MtFold F;
    F.st = st_.data();
    F.ru = ru.data();
    F.rv = rv.data();
    F.w = val;
    F.mark = mark.data();
    F.accepted = acc.data();
    F.rec = rec.data();
    F.base = folded_;
    F.n = (uint32_t)n;
    F.sharpen = (sharpen && weight_safe) ? 1 : 0;
    std::vector<uint32_t> pend(n), next;
    // (any order inside a phase: descending here, where a kernel's threads run in no order at all)
    for (uint64_t i = 0; i < n; ++i) pend[i] = (uint32_t)(n - 1 - i);
    const uint32_t cap = std::min(std::max(iter_cap, 1u), kMatchingMaxIterCap);
    while (!pend.empty()) {
      for (uint32_t e : pend) mt_ph_reset(F, e);
      for (uint32_t e : pend) mt_ph_seed(F, e);
      bool changed = true;
      for (uint32_t it = 0; it < cap && changed; ++it) {
        changed = false;
        for (uint32_t e : pend) changed |= mt_ph_pass(F, e);
        ++stats.iterations;
      }
      if (changed) {
        for (uint32_t e : pend) mt_ph_lower(F, e);
        ++stats.fallbacks;
      }
      for (uint32_t e : pend) mt_ph_remain(F, e);
      next.clear();
      for (uint32_t e : pend)
        if (mt_ph_commit(F, e)) next.push_back(e);
      if (next.size() >= pend.size()) return ~0ull;  // (cannot happen: the earliest pending arrival leaves)
      pend.swap(next);
      ++stats.rounds;
    }
    uint64_t kept = 0;
    for (uint64_t i = 0; i < n; ++i) {
      if (accepted) accepted[i] = acc[i];
      if (!acc[i]) continue;
      ++kept;
      const MtRec& r = rec[i];
      if (events) {
        if (r.s0 != kMtNone) events->push_back(MtEvent{(uint32_t)i, kMatchRemove, id_[r.s0], id_[r.d0], r.v0});
        if (r.s1 != kMtNone) events->push_back(MtEvent{(uint32_t)i, kMatchRemove, id_[r.s1], id_[r.d1], r.v1});
        events->push_back(MtEvent{(uint32_t)i, kMatchAdd, src[i], dst[i], val[i]});
      }
    }
    stats.accepted = kept;
    folded_ += n;
    return kept;
  }

  std::vector<MtEdge> sorted_edges() const {
    std::vector<MtEdge> out;
    for (uint32_t r = 0; r < st_.size(); ++r)
      if (st_[r].partner != kMtNone && st_[r].is_src)
        out.push_back(MtEdge{id_[r], id_[st_[r].partner], st_[r].value, st_[r].stamp});
    std::sort(out.begin(), out.end(), [](const MtEdge& a, const MtEdge& b) { return a.first < b.first; });
    return out;
  }

 private:
  uint32_t rank_of(int64_t id) {
    const auto it = rank_.find(id);
    if (it != rank_.end()) return it->second;
    const uint32_t r = (uint32_t)id_.size();
    rank_[id] = r;
    id_.push_back(id);
    st_.push_back(mt_vertex_init());
    return r;
  }
  std::unordered_map<int64_t, uint32_t> rank_;
  std::vector<int64_t> id_;
  std::vector<MtVertex> st_;
  uint64_t folded_ = 0;
};

inline uint64_t mt_fold_rounds(MatchingRounds& m, const int64_t* src, const int64_t* dst, const int64_t* val,
                               uint64_t n, uint8_t* accepted, std::vector<MtEvent>* events) {
  return m.fold(src, dst, val, n, accepted, events);
}

}  // namespace gs
#endif
