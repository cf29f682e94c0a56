// gs_trisample_seq.hpp -- the rules of the sampling triangle estimate (gs_trisample_k.hip,
// gs_trisample.cpp): java.util.Random's 48-bit LCG with its jump-ahead, the seeding of the
// instances, the coin, the counter-based third-vertex draw, the per-instance candidate record,
// the estimate with Java's double-to-int cast, the per-lane bodies of the kernels, and -- host
// only -- the sequential definition (TsSeq, ts_fold_seq) and a restatement of the decomposition
// the kernels use that calls the very lane functions they call (ts_fold_parts).
// Standard headers only: the kernels include it, and a host compiler builds
// tests/cpp/trisample_seq_sanitize.cpp, which checks it under the address and UB sanitizers.
//
// The contract (example/BroadcastTriangleCount.java:62-174 at parallelism 1, the seeded coin of
// example/IncidenceSamplingTriangleCount.java's EdgeSampleMapper). S instances; for arrival number
// t (from 1) and every instance i:
//   coin    nextDouble() * (double)t <= 1.0 on instance i's own java.util.Random, whose seed is
//           (long) master.nextInt(), drawn in instance order from new Random(seed). One
//           nextDouble per instance and arrival, success or not: the coin of instance i at t is
//           a function of (seed, i, t).
//   sample  on success the candidate becomes (src, trg, third), flags and beta cleared; third is
//           this project's own draw (the reference uses the unseeded Math.random()):
//             h = mix64(third_seed + 0x9E3779B97F4A7C15 * (i + 1)); h = mix64(h ^ t);
//             attempt a = 0, 1, ..: x = mix64(h ^ a), third = floor((x >> 11) * 2^-53 * vertices),
//             the first third that differs from src and trg.
//   observe while beta == 0 the arrival is compared in either direction with {src, third} and
//           {trg, third}; beta = 1 once both were seen (so beta == srcFound && trgFound).
//   rows    betaSum(t) = the instances with beta == 1 after arrival t. A row
//           (t, estimate(t), betaSum(t)) is emitted iff betaSum(t) != betaSum(t - 1) and
//           estimate(t) differs from the estimate at the previous arrival whose betaSum changed
//           (0 before any); estimate = (int)((((1.0 / S) * betaSum) * t) * (vertices - 2)).
// Not built: parallelism above 1 (per-subtask sample shares, the per-source result map),
// IncidenceSampling's intermediate emissions (the sums it emits while only some instances have
// seen the current edge; its instance states after every edge equal Broadcast's under the same
// draws, and those are reproduced), combine, serialization, multi-GPU groups, the JNI glue.
//
// The decomposition. A fold of n arrivals at edge counts t0 + 1 .. t0 + n:
//   coin     over (instance, chunk of arrivals): jump the stored LCG state to the chunk's start
//            (one affine map for all instances), two steps per arrival, successes appended as
//            keys (instance << 32 | position) in any order
//   segments the keys sorted; instance i's fold is its carried-in candidate on [0, first
//            resample) -- segment i -- and one segment S + j per sorted key j, up to the next key
//            of the same instance or n
//   search   over (instance, tile of arrivals): a lane walks its instance's segments inside the
//            tile and lowers each segment's first position of {src, third} and of {trg, third}
//   finish   per segment: +1 at the later of the two firsts, -1 at the segment's end when a
//            resample ends a complete candidate; the instance's last segment is its new state
//   rows     betaSum by a scan of those deltas, the changed arrivals compacted in order, the row
//            rule over neighbours of that list.
#pragma once
#include <math.h>
#include <stdint.h>

#if !defined(GS_TRISAMPLE_SEQ_RULES_ONLY)
#include <algorithm>
#include <vector>
#endif

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GS_TS_HD __host__ __device__ inline
#else
#define GS_TS_HD inline
#endif

namespace gs {

// ---- product constants (gsamd.TRISAMPLE_*)
constexpr uint32_t kTsChunk = 256;               // arrivals per workgroup of the coin pass
constexpr uint32_t kTsTile = 1024;               // arrivals per workgroup of the search pass (staged in LDS)
constexpr uint32_t kTsMaxSamples = 1u << 20;     // instances of a handle
constexpr int64_t kTsMinVertices = 3;
constexpr int64_t kTsMaxVertices = 2147483647;   // the reference's vertex count is a Java int
constexpr uint64_t kTsMaxArrivals = 2147483647;  // and so is its edge count
constexpr int64_t kTsDefaultSeed = -559038737;   // the Java int literal 0xDEADBEEF, widened
constexpr uint64_t kTsMaxFold = 1ull << 20;      // arrivals of one device fold (the host cuts longer ones)

constexpr uint32_t kTsNever = 0xFFFFFFFFu;  // a first position: not seen (every position is below)

// ---- java.util.Random
constexpr uint64_t kTsMult = 0x5DEECE66Dull;
constexpr uint64_t kTsAdd = 0xBull;
constexpr uint64_t kTsMask = (1ull << 48) - 1;

GS_TS_HD uint64_t ts_scramble(int64_t seed) { return ((uint64_t)seed ^ kTsMult) & kTsMask; }
GS_TS_HD uint64_t ts_step(uint64_t s) { return (s * kTsMult + kTsAdd) & kTsMask; }
// next(32) of the state AFTER a step, read as a signed int
GS_TS_HD int32_t ts_int_of(uint64_t s) { return (int32_t)(uint32_t)(s >> 16); }

// s -> (a * s + c) mod 2^48
struct TsAffine {
  uint64_t a, c;
};
GS_TS_HD uint64_t ts_apply(const TsAffine& f, uint64_t s) { return (f.a * s + f.c) & kTsMask; }
// f, then g
GS_TS_HD TsAffine ts_then(const TsAffine& f, const TsAffine& g) {
  TsAffine r;
  r.a = (g.a * f.a) & kTsMask;
  r.c = (g.a * f.c + g.c) & kTsMask;
  return r;
}
// k steps at once: (A^k, C_k), by squaring
GS_TS_HD TsAffine ts_jump(uint64_t k) {
  TsAffine r = {1, 0}, p = {kTsMult, kTsAdd};
  while (k) {
    if (k & 1) r = ts_then(r, p);
    p = ts_then(p, p);
    k >>= 1;
  }
  return r;
}
// the LCG state instance i starts from: its seed is (long) master.nextInt(), draw i + 1 of the master
GS_TS_HD int64_t ts_instance_seed(int64_t master_seed, uint32_t i) {
  return (int64_t)ts_int_of(ts_apply(ts_jump((uint64_t)i + 1), ts_scramble(master_seed)));
}
GS_TS_HD uint64_t ts_instance_state(int64_t master_seed, uint32_t i) {
  return ts_scramble(ts_instance_seed(master_seed, i));
}

// ---- the coin. nextDouble() = ((next(26) << 27) + next(27)) * 2^-53: hi is next(26) of the
// state after the first step, lo next(27) of the state after the second.
GS_TS_HD uint32_t ts_hi_of(uint64_t s1) { return (uint32_t)(s1 >> 22); }
GS_TS_HD uint32_t ts_lo_of(uint64_t s2) { return (uint32_t)(s2 >> 21); }
GS_TS_HD double ts_double_of(uint32_t hi, uint32_t lo) {
  return (double)(((uint64_t)hi << 27) + lo) * 0x1.0p-53;
}
GS_TS_HD bool ts_coin(uint32_t hi, uint32_t lo, uint32_t t) { return ts_double_of(hi, lo) * (double)t <= 1.0; }
// A sure failure from the high bits alone: hi * t >= 2^26 + 2 t gives nextDouble() * t >=
// hi * t * 2^-26 > 1 + 2^-26, which no rounding of the double product brings down to 1.0.
GS_TS_HD bool ts_coin_rejects(uint32_t hi, uint32_t t) {
  return (uint64_t)hi * t >= (1ull << 26) + 2ull * t;
}
// One lane of the coin pass: `count` arrivals at edge counts t_first .., from LCG state s;
// emit(k, success) for every one of them, in order. Returns the state after them.
template <class Emit>
GS_TS_HD uint64_t ts_coin_lane(uint64_t s, uint32_t t_first, uint32_t count, Emit emit) {
  for (uint32_t k = 0; k < count; ++k) {
    const uint64_t s1 = ts_step(s);
    s = ts_step(s1);
    const uint32_t t = t_first + k, hi = ts_hi_of(s1);
    emit(k, !ts_coin_rejects(hi, t) && ts_coin(hi, ts_lo_of(s), t));
  }
  return s;
}

// ---- the third vertex (mix64: the finaliser of gs_gen.hip's generators)
GS_TS_HD uint64_t ts_mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
GS_TS_HD int64_t ts_third(uint64_t third_seed, uint32_t instance, uint32_t t, int64_t vertices, int64_t src,
                          int64_t trg, uint32_t* attempts) {
  uint64_t h = ts_mix64(third_seed + 0x9E3779B97F4A7C15ull * ((uint64_t)instance + 1));
  h = ts_mix64(h ^ (uint64_t)t);
  for (uint64_t a = 0;; ++a) {  // (vertices >= 3: two of three values fail at worst)
    const uint64_t x = ts_mix64(h ^ a);
    const int64_t third = (int64_t)floor(((double)(x >> 11) * 0x1.0p-53) * (double)vertices);
    if (third != src && third != trg) {
      *attempts = (uint32_t)(a + 1);
      return third;
    }
  }
}

// ---- the candidate of an instance (SampleTriangleState)
enum TsFlags : uint32_t { kTsSrcFound = 1, kTsTrgFound = 2, kTsBeta = 4 };
struct TsState {
  int64_t src, trg, third;
  int32_t sampled_at;  // the edge count at which the candidate was sampled (0: none yet)
  uint32_t flags;
};
GS_TS_HD TsState ts_state_init() {
  TsState s;
  s.src = 0;
  s.trg = 0;
  s.third = -1;
  s.sampled_at = 0;
  s.flags = 0;
  return s;
}
GS_TS_HD bool ts_closes(int64_t a, int64_t b, int64_t v, int64_t third) {
  return (a == v && b == third) || (a == third && b == v);
}
GS_TS_HD void ts_observe(TsState& s, int64_t a, int64_t b) {
  if (s.flags & kTsBeta) return;
  if (ts_closes(a, b, s.src, s.third)) s.flags |= kTsSrcFound;
  if (ts_closes(a, b, s.trg, s.third)) s.flags |= kTsTrgFound;
  if ((s.flags & 3u) == 3u) s.flags |= kTsBeta;
}

// ---- the estimate
GS_TS_HD int32_t ts_java_int(double x) {  // (int) x of Java: truncate, saturate, NaN -> 0
  if (x != x) return 0;
  if (x >= 2147483647.0) return 2147483647;
  if (x <= -2147483648.0) return -2147483647 - 1;
  return (int32_t)x;
}
// inv_s = 1.0 / (double)S
GS_TS_HD int32_t ts_estimate(double inv_s, int32_t beta_sum, int32_t edges, int32_t vertices) {
  return ts_java_int(((inv_s * (double)beta_sum) * (double)edges) * (double)(vertices - 2));
}

// ---- segments. Segment i < S is instance i's carried-in candidate; segment S + j belongs to
// sorted key j. flags: what the candidate had found before the fold (immutable in the search);
// fs / ft: the first position in the fold, inside the segment, of {src, third} / {trg, third},
// lowered by the search; end: the position of the instance's next resample, or n.
struct TsSeg {
  int64_t src, trg, third;
  uint32_t fs, ft;
  uint32_t end;
  int32_t sampled_at;
  uint32_t flags;
  uint32_t pad_;
};
GS_TS_HD TsSeg ts_seg_carried(const TsState& s, uint32_t n) {
  TsSeg g;
  g.src = s.src;
  g.trg = s.trg;
  g.third = s.third;
  g.fs = g.ft = kTsNever;
  g.end = n;
  g.sampled_at = s.sampled_at;
  g.flags = s.flags;
  g.pad_ = 0;
  return g;
}
GS_TS_HD uint32_t ts_key_instance(uint64_t key) { return (uint32_t)(key >> 32); }
GS_TS_HD uint32_t ts_key_position(uint64_t key) { return (uint32_t)key; }
GS_TS_HD uint64_t ts_key(uint32_t instance, uint32_t pos) { return ((uint64_t)instance << 32) | pos; }
// Sorted key j of K: its segment (the arrival at its position is (src, trg)).
GS_TS_HD TsSeg ts_seg_sampled(const uint64_t* keys, uint64_t K, uint64_t j, uint32_t n, int64_t src, int64_t trg,
                              uint32_t t0, uint64_t third_seed, int64_t vertices, uint32_t* attempts) {
  const uint32_t inst = ts_key_instance(keys[j]), pos = ts_key_position(keys[j]);
  TsSeg g;
  g.src = src;
  g.trg = trg;
  g.third = ts_third(third_seed, inst, t0 + pos + 1, vertices, src, trg, attempts);
  g.fs = g.ft = kTsNever;
  g.end = (j + 1 < K && ts_key_instance(keys[j + 1]) == inst) ? ts_key_position(keys[j + 1]) : n;
  g.sampled_at = (int32_t)(t0 + pos + 1);
  g.flags = 0;
  g.pad_ = 0;
  return g;
}
GS_TS_HD bool ts_key_first_of_instance(const uint64_t* keys, uint64_t j) {
  return j == 0 || ts_key_instance(keys[j - 1]) != ts_key_instance(keys[j]);
}

// fs / ft only fall inside a search. On the device: an atomic minimum.
GS_TS_HD void ts_lower(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicMin(p, v);
#else
  if (v < *p) *p = v;
#endif
}
// the first index in keys[0 .. K) whose key is greater than x
GS_TS_HD uint64_t ts_upper_bound(const uint64_t* keys, uint64_t K, uint64_t x) {
  uint64_t lo = 0, hi = K;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (keys[mid] <= x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

struct TsEdge {
  int64_t a, b;
};
// One lane of the search pass: instance inst over the arrivals [lo, hi) of a tile; edge_at(pos)
// is the arrival at fold position pos. The lane finds the segment that holds lo, walks on at
// every resample of its instance inside the tile, and lowers a segment's fs / ft to the first
// closing arrival it saw of each side that segment still needs.
template <class EdgeAt>
GS_TS_HD void ts_search_lane(TsSeg* seg, const uint64_t* keys, uint64_t K, uint32_t S, uint32_t inst, uint32_t lo,
                             uint32_t hi, EdgeAt edge_at) {
  uint64_t j = ts_upper_bound(keys, K, ts_key(inst, lo));
  uint32_t cur = (j > 0 && ts_key_instance(keys[j - 1]) == inst) ? S + (uint32_t)(j - 1) : inst;
  uint32_t next = (j < K && ts_key_instance(keys[j]) == inst) ? ts_key_position(keys[j]) : kTsNever;
  int64_t src = seg[cur].src, trg = seg[cur].trg, third = seg[cur].third;
  uint32_t need = (seg[cur].flags & kTsBeta) ? 0u : (~seg[cur].flags & 3u);
  for (uint32_t pos = lo; pos < hi; ++pos) {
    if (pos == next) {
      cur = S + (uint32_t)j;
      ++j;
      next = (j < K && ts_key_instance(keys[j]) == inst) ? ts_key_position(keys[j]) : kTsNever;
      src = seg[cur].src;
      trg = seg[cur].trg;
      third = seg[cur].third;
      need = 3u;
    }
    if (need) {
      const TsEdge e = edge_at(pos);
      if (e.a == third || e.b == third) {
        if ((need & kTsSrcFound) && ts_closes(e.a, e.b, src, third)) {
          ts_lower(&seg[cur].fs, pos);
          need &= ~(uint32_t)kTsSrcFound;
        }
        if ((need & kTsTrgFound) && ts_closes(e.a, e.b, trg, third)) {
          ts_lower(&seg[cur].ft, pos);
          need &= ~(uint32_t)kTsTrgFound;
        }
      }
    }
  }
}

// What a searched segment does to betaSum and to its instance's state.
struct TsOutcome {
  uint32_t plus;   // position of a +1 (kTsNever: none)
  uint32_t minus;  // position of a -1 (kTsNever: none)
  uint32_t flags;  // the candidate's flags at the segment's end
};
GS_TS_HD TsOutcome ts_outcome(const TsSeg& g, uint32_t n) {
  TsOutcome o;
  o.plus = o.minus = kTsNever;
  o.flags = g.flags;
  if (!(g.flags & kTsBeta)) {
    const uint32_t ps = (g.flags & kTsSrcFound) ? 0u : g.fs, pt = (g.flags & kTsTrgFound) ? 0u : g.ft;
    if (ps != kTsNever) o.flags |= kTsSrcFound;
    if (pt != kTsNever) o.flags |= kTsTrgFound;
    if (ps != kTsNever && pt != kTsNever) {
      o.flags |= kTsBeta;
      o.plus = ps > pt ? ps : pt;
    }
  }
  if (g.end < n && (o.flags & kTsBeta)) o.minus = g.end;
  return o;
}
GS_TS_HD TsState ts_state_of(const TsSeg& g, uint32_t flags) {
  TsState s;
  s.src = g.src;
  s.trg = g.trg;
  s.third = g.third;
  s.sampled_at = g.sampled_at;
  s.flags = flags;
  return s;
}

// One row of a fold.
struct TsRow {
  int32_t edges, estimate, beta_sum;
};

#if !defined(GS_TRISAMPLE_SEQ_RULES_ONLY)
// ---- host only: the sequential definition
struct TsSeq {
  uint32_t samples;
  int32_t vertices;
  uint64_t third_seed;
  std::vector<uint64_t> lcg;  // every instance's java.util.Random state
  std::vector<TsState> st;
  uint32_t folded = 0;
  int32_t beta_sum = 0;       // TriangleSampler.previousResult
  int32_t last_estimate = 0;  // TriangleSummer.previousResult
  // the last fold
  uint64_t coins = 0;
  uint32_t max_attempts = 0;

  TsSeq(uint32_t samples_, int32_t vertices_, int64_t seed, uint64_t third_seed_)
      : samples(samples_), vertices(vertices_), third_seed(third_seed_), lcg(samples_), st(samples_, ts_state_init()) {
    uint64_t m = ts_scramble(seed);
    for (uint32_t i = 0; i < samples; ++i) {
      m = ts_step(m);
      lcg[i] = ts_scramble((int64_t)ts_int_of(m));
    }
  }
  double inv_s() const { return 1.0 / (double)samples; }
};

// a literal per-edge loop over the instances; appends the fold's rows
inline void ts_fold_seq(TsSeq& q, const int64_t* src, const int64_t* dst, size_t n, std::vector<TsRow>* rows) {
  q.coins = 0;
  q.max_attempts = 0;
  for (size_t e = 0; e < n; ++e) {
    const uint32_t t = ++q.folded;
    int32_t local = 0;
    for (uint32_t i = 0; i < q.samples; ++i) {
      const uint64_t s1 = ts_step(q.lcg[i]);
      q.lcg[i] = ts_step(s1);
      TsState& s = q.st[i];
      if (ts_coin(ts_hi_of(s1), ts_lo_of(q.lcg[i]), t)) {
        uint32_t attempts = 0;
        s.src = src[e];
        s.trg = dst[e];
        s.third = ts_third(q.third_seed, i, t, q.vertices, src[e], dst[e], &attempts);
        s.flags = 0;
        s.sampled_at = (int32_t)t;
        ++q.coins;
        q.max_attempts = std::max(q.max_attempts, attempts);
      }
      ts_observe(s, src[e], dst[e]);
      if (s.flags & kTsBeta) ++local;
    }
    if (local != q.beta_sum) {
      q.beta_sum = local;
      const int32_t est = ts_estimate(q.inv_s(), local, (int32_t)t, q.vertices);
      if (est != q.last_estimate) {
        q.last_estimate = est;
        if (rows) rows->push_back({(int32_t)t, est, local});
      }
    }
  }
}

// The decomposition of the kernels, on the host: coin by chunks of `chunk` arrivals, the sorted
// keys, the segments, the search by tiles of `tile` arrivals, the outcomes, the scan, the rows.
inline void ts_fold_parts(TsSeq& q, const int64_t* src, const int64_t* dst, size_t n_, uint32_t chunk, uint32_t tile,
                          std::vector<TsRow>* rows) {
  q.coins = 0;
  q.max_attempts = 0;
  const uint32_t n = (uint32_t)n_, S = q.samples, t0 = q.folded;
  if (n == 0) return;
  // coin
  std::vector<uint64_t> keys;
  for (uint32_t c0 = 0; c0 < n; c0 += chunk) {
    const uint32_t len = std::min(chunk, n - c0);
    const TsAffine to_chunk = ts_jump(2ull * c0);
    for (uint32_t i = 0; i < S; ++i) {
      const uint64_t after = ts_coin_lane(ts_apply(to_chunk, q.lcg[i]), t0 + c0 + 1, len, [&](uint32_t k, bool ok) {
        if (ok) keys.push_back(ts_key(i, c0 + k));
      });
      if (c0 + len == n) q.lcg[i] = after;  // (the last chunk reads the stored state last)
    }
  }
  // segments
  std::sort(keys.begin(), keys.end());
  const uint64_t K = keys.size();
  q.coins = K;
  std::vector<TsSeg> seg(S + K);
  for (uint32_t i = 0; i < S; ++i) seg[i] = ts_seg_carried(q.st[i], n);
  for (uint64_t j = 0; j < K; ++j) {
    const uint32_t pos = ts_key_position(keys[j]);
    uint32_t attempts = 0;
    seg[S + j] = ts_seg_sampled(keys.data(), K, j, n, src[pos], dst[pos], t0, q.third_seed, q.vertices, &attempts);
    q.max_attempts = std::max(q.max_attempts, attempts);
    if (ts_key_first_of_instance(keys.data(), j)) seg[ts_key_instance(keys[j])].end = pos;
  }
  // search
  for (uint32_t lo = 0; lo < n; lo += tile)
    for (uint32_t i = 0; i < S; ++i)
      ts_search_lane(seg.data(), keys.data(), K, S, i, lo, std::min(n, lo + tile), [&](uint32_t pos) {
        return TsEdge{src[pos], dst[pos]};
      });
  // finish
  std::vector<int32_t> delta(n, 0);
  for (uint64_t g = 0; g < S + K; ++g) {
    const TsOutcome o = ts_outcome(seg[g], n);
    if (o.plus != kTsNever) ++delta[o.plus];
    if (o.minus != kTsNever) --delta[o.minus];
    if (seg[g].end == n) q.st[g < S ? g : ts_key_instance(keys[g - S])] = ts_state_of(seg[g], o.flags);
  }
  // rows
  for (uint32_t p = 0; p < n; ++p) {
    if (delta[p] == 0) continue;
    q.beta_sum += delta[p];
    const int32_t est = ts_estimate(q.inv_s(), q.beta_sum, (int32_t)(t0 + p + 1), q.vertices);
    if (est != q.last_estimate) {
      q.last_estimate = est;
      if (rows) rows->push_back({(int32_t)(t0 + p + 1), est, q.beta_sum});
    }
  }
  q.folded += n;
}
#endif

}  // namespace gs
