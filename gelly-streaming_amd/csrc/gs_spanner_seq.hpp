// gs_spanner_seq.hpp -- the sequential definitions of the k-spanner summary (gs_spanner_k.hip,
// gs_spanner.cpp): the status bytes of a pending edge, which pending entries a search may walk,
// the capacity arithmetic of the on-chip sets, the step rule of the two-sided search, the verdict
// of a round, and -- host only -- a plain restatement of within, of the fold and of the fold by
// rounds. Standard headers only: the kernels include it, and a host compiler builds
// tests/cpp/spanner_seq_sanitize.cpp, which checks every function against brute force under the
// address and UB sanitizers.
//
// The contract (library/Spanner.java, summaries/AdjacencyListGraph.java): within(s, t, k) is
// true iff t is reached from s by 1..k edges of G; for s == t iff the loop {s, s} is in G. An
// arrival is accepted (added to G) iff within is false on the graph the arrivals before it left.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GS_SP_HD __host__ __device__ inline
#else
#define GS_SP_HD inline
#endif

namespace gs {

constexpr int kSpannerMaxK = 16;  // 1 <= k <= 16 (gs_spanner_create, gs_spanner_within)

// status byte of a pending edge (an arrival the filter pass did not drop)
enum SpannerStatus : uint8_t { kSpUndecided = 0, kSpAccepted = 1, kSpDropped = 2 };

// the graph a search walks: G0 alone, or G0 and some of the pending edges before edge i
enum SpannerView : int {
  kSpBase = 0,   // G0 (within queries, the filter pass)
  kSpUpper = 1,  // G0 + pending j < i not dropped: contains the true graph before i
  kSpLower = 2   // G0 + pending j < i accepted: contained in the true graph before i
};

// A directed pending entry carries the pending index j of its edge; the second entry of a
// self-loop carries kSpDead (a loop is one entry of its row) and is never walked.
constexpr uint32_t kSpDead = 0xFFFFFFFFu;

// May the search of pending edge i walk an entry of pending edge j whose status is st?
GS_SP_HD bool sp_traversable(int view, uint32_t j, uint32_t i, uint8_t st) {
  if (j >= i) return false;  // (kSpDead too)
  return view == kSpUpper ? st != kSpDropped : view == kSpLower ? st == kSpAccepted : false;
}

// Verdict of a round from the two searches (the lower one is only needed when the upper one
// found the endpoints within k): accepted when even the upper graph keeps them apart, dropped
// when already the lower graph joins them, undecided otherwise.
GS_SP_HD uint8_t sp_round_verdict(bool upper_within, bool lower_within) {
  if (!upper_within) return kSpAccepted;
  return lower_within ? kSpDropped : kSpUndecided;
}

// The two-sided search expands the side with the smaller frontier (side 0, the source's, on a
// tie) and ends when that frontier is empty: its ball is complete and did not meet the other.
GS_SP_HD int sp_pick_side(uint32_t frontier0, uint32_t frontier1) { return frontier1 < frontier0 ? 1 : 0; }

// On-chip sets of one wave: `entries` vertices per side, in an open-addressing table of
// sp_set_slots(entries) 8-byte keys (load <= 1/2) beside the list of the vertices in discovery
// order (8 bytes each). Product: kSpannerLdsSet entries per side, 12 KiB per wave, so 13 waves
// share the 160 KiB of a CU.
constexpr uint32_t kSpannerLdsSet = 256;
GS_SP_HD uint32_t sp_set_slots(uint32_t entries) {
  uint32_t s = 2;
  while (s < 2 * entries) s <<= 1;
  return s;
}
GS_SP_HD uint32_t sp_set_bytes(uint32_t entries) { return 2 * (sp_set_slots(entries) + entries) * 8; }
static_assert(kSpannerLdsSet >= 1 && kSpannerLdsSet <= 1024, "the sets of a wave stay below 64 KiB");
GS_SP_HD uint32_t sp_clamp_set(int64_t entries) {
  return entries < 1 ? 1u : entries > (int64_t)kSpannerLdsSet ? kSpannerLdsSet : (uint32_t)entries;
}

// home slot of an id in a table of `slots` (a power of two) keys
GS_SP_HD uint32_t sp_hash(int64_t id, uint32_t slots) {
  uint64_t x = (uint64_t)id * 0x9E3779B97F4A7C15ull;
  x ^= x >> 29;
  return (uint32_t)(x >> 11) & (slots - 1);
}

// Round control: after a round that began with `before` undecided edges and left `after`, go to
// the serial tail when it decided less than one in eight.
GS_SP_HD bool sp_slow_round(uint64_t before, uint64_t after) { return (before - after) * 8 < before; }

// stamp of side `side` (0, 1) in search number gen of an arena; 0 is never a stamp
GS_SP_HD uint32_t sp_stamp(uint32_t gen, int side) { return 2 * gen + 1 + (uint32_t)side; }
constexpr uint32_t kSpMaxGen = 0x7FFFFFF0u;  // the arenas are cleared before gen passes this

}  // namespace gs

// (the library's own sources want the rules above only: gs_spanner.hpp defines the macro)
#if !defined(GS_SPANNER_SEQ_RULES_ONLY)
#include <algorithm>
#include <map>
#include <set>
#include <utility>
#include <vector>

namespace gs {

// AdjacencyListGraph and Spanner.UpdateLocal restated: the truth of every test and the baseline
// of tools/spanner_bench.py.
class SpannerSeq {
 public:
  explicit SpannerSeq(int k) : k_(k) {}

  // AdjacencyListGraph.boundedBFS: level by level from s, t found at level 1..k
  bool within(int64_t s, int64_t t, int k) const {
    auto it = adj_.find(s);
    if (it == adj_.end()) return false;
    if (s == t) return it->second.count(s) != 0;  // (s is never revisited: only its own loop reaches it)
    std::set<int64_t> visited{s};
    std::vector<int64_t> frontier{s}, next;
    for (int level = 1; level <= k && !frontier.empty(); ++level) {
      next.clear();
      for (int64_t u : frontier)
        for (int64_t y : adj_.find(u)->second) {
          if (y == t) return true;
          if (visited.insert(y).second) next.push_back(y);
        }
      frontier.swap(next);
    }
    return false;
  }

  // the same answer by the two-sided search the kernels run, with this header's step rule
  bool within_two_sided(int64_t s, int64_t t, int k) const {
    if (s == t) {
      auto it = adj_.find(s);
      return it != adj_.end() && it->second.count(s) != 0;
    }
    std::set<int64_t> seen[2] = {{s}, {t}};
    std::vector<int64_t> frontier[2] = {{s}, {t}}, next;
    for (int step = 0; step < k; ++step) {
      const int side = sp_pick_side((uint32_t)frontier[0].size(), (uint32_t)frontier[1].size());
      if (frontier[side].empty()) return false;
      next.clear();
      for (int64_t u : frontier[side]) {
        auto it = adj_.find(u);
        if (it == adj_.end()) continue;
        for (int64_t y : it->second) {
          if (seen[side ^ 1].count(y)) return true;
          if (seen[side].insert(y).second) next.push_back(y);
        }
      }
      frontier[side].swap(next);
    }
    return false;
  }

  void add(int64_t s, int64_t t) {
    const bool fresh = adj_[s].insert(t).second;
    adj_[t].insert(s);
    if (fresh) ++edges_;
  }

  // Spanner.UpdateLocal over a batch in arrival order; accepted[i] (optional) = arrival i was added
  uint64_t fold(const int64_t* src, const int64_t* dst, uint64_t n, uint8_t* accepted) {
    uint64_t kept = 0;
    for (uint64_t i = 0; i < n; ++i) {
      const bool keep = !within(src[i], dst[i], k_);
      if (keep) add(src[i], dst[i]);
      if (accepted) accepted[i] = keep ? 1 : 0;
      kept += keep ? 1 : 0;
    }
    return kept;
  }

  // The fold by rounds, as the device runs it but one search at a time: the filter pass on G0,
  // then rounds over the pending edges with the statuses of the round before, then -- after
  // round_cap rounds -- the serial tail. *rounds (optional) = rounds run. Equal to fold().
  uint64_t fold_rounds(const int64_t* src, const int64_t* dst, uint64_t n, uint8_t* accepted, uint32_t round_cap,
                       uint32_t* rounds) {
    std::vector<uint32_t> pend;
    for (uint64_t i = 0; i < n; ++i) {
      if (accepted) accepted[i] = 0;
      if (!within_two_sided(src[i], dst[i], k_)) pend.push_back((uint32_t)i);
    }
    const uint32_t np = (uint32_t)pend.size();
    std::vector<uint8_t> st(np, kSpUndecided), nst;
    auto view_within = [&](int view, uint32_t i, const std::vector<uint8_t>& status) {
      SpannerSeq g(*this);
      for (uint32_t j = 0; j < np; ++j)
        if (sp_traversable(view, j, i, status[j])) g.add(src[pend[j]], dst[pend[j]]);
      return g.within_two_sided(src[pend[i]], dst[pend[i]], k_);
    };
    uint32_t r = 0;
    uint64_t und = np;
    while (und && r < round_cap) {
      nst = st;
      for (uint32_t i = 0; i < np; ++i) {
        if (st[i] != kSpUndecided) continue;
        const bool up = view_within(kSpUpper, i, st);
        nst[i] = sp_round_verdict(up, up && view_within(kSpLower, i, st));
      }
      st.swap(nst);
      und = (uint64_t)std::count(st.begin(), st.end(), (uint8_t)kSpUndecided);
      ++r;
    }
    for (uint32_t i = 0; i < np && und; ++i) {  // the tail: arrival order, statuses in place
      if (st[i] != kSpUndecided) continue;
      st[i] = view_within(kSpLower, i, st) ? kSpDropped : kSpAccepted;
    }
    if (rounds) *rounds = r;
    uint64_t kept = 0;
    for (uint32_t i = 0; i < np; ++i) {
      if (st[i] != kSpAccepted) continue;
      add(src[pend[i]], dst[pend[i]]);
      if (accepted) accepted[pend[i]] = 1;
      ++kept;
    }
    return kept;
  }

  uint64_t edges() const { return edges_; }
  uint64_t vertices() const { return adj_.size(); }
  // the edges ascending by (lo, hi), each once
  std::vector<std::pair<int64_t, int64_t>> sorted_edges() const {
    std::vector<std::pair<int64_t, int64_t>> e;
    for (const auto& row : adj_)
      for (int64_t y : row.second)
        if (row.first <= y) e.emplace_back(row.first, y);
    return e;
  }
  const std::map<int64_t, std::set<int64_t>>& adjacency() const { return adj_; }

 private:
  int k_;
  uint64_t edges_ = 0;
  std::map<int64_t, std::set<int64_t>> adj_;
};

}  // namespace gs
#endif
