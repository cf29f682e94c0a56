// The tile / carry arithmetic of the window slices (csrc/gs_slice_seg.hpp) on the host, against
// brute force, built with -fsanitize=address,undefined (tests/test_slice_seg.py). The program
// walks a window the way gs_slice_k.hip does -- tiles of T positions, threads of P consecutive
// positions, waves of W threads joined by the same doubling scan, a carry record per tile, an
// exclusive scan of the records, a fix-up per tile -- with every decision (what a position
// emits, where it lands, which tile fixes up) taken by the header's functions, and checks that
// every row of the output is written exactly once, inside its array, with the right value.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "gs_slice_seg.hpp"

using namespace gs;

static long checks = 0;

#define REQUIRE(cond)                                                       \
  do {                                                                      \
    ++checks;                                                               \
    if (!(cond)) {                                                          \
      std::printf("FAILED %s (line %d)\n", #cond, __LINE__);                \
      std::exit(1);                                                         \
    }                                                                       \
  } while (0)

// exclusive prefixes of `agg` (one stretch per thread, in order) the way a workgroup forms
// them: a doubling inclusive scan inside each wave of W lanes, then the waves before it
template <int OP>
static std::vector<SegPair> block_excl(const std::vector<SegPair>& agg, size_t W, SegPair* total) {
  const size_t n = agg.size(), waves = (n + W - 1) / W;
  std::vector<SegPair> inc(waves * W, seg_identity<OP>());
  for (size_t i = 0; i < n; ++i) inc[i] = agg[i];
  for (size_t o = 1; o < W; o <<= 1) {
    const std::vector<SegPair> prev = inc;
    for (size_t i = 0; i < inc.size(); ++i)
      if (i % W >= o) inc[i] = seg_combine<OP>(prev[i - o], prev[i]);
  }
  std::vector<SegPair> ex(n);
  SegPair all = seg_identity<OP>();
  for (size_t w = 0; w < waves; ++w) {
    for (size_t l = 0; l < W && w * W + l < n; ++l)
      ex[w * W + l] = seg_combine<OP>(all, l ? inc[w * W + l - 1] : seg_identity<OP>());
    all = seg_combine<OP>(all, inc[w * W + W - 1]);
  }
  *total = all;
  return ex;
}

template <int OP>
static std::vector<int64_t> brute(const std::vector<uint8_t>& head, const std::vector<int64_t>& val) {
  std::vector<int64_t> out;
  for (size_t i = 0; i < head.size(); ++i) {
    if (head[i]) out.push_back(val[i]);
    else out.back() = slice_op<OP>(out.back(), val[i]);
  }
  return out;
}

// head[0] must be 1 when there is an entry
template <int OP>
static void run_window(const std::vector<uint8_t>& head, const std::vector<int64_t>& val, uint32_t T, uint32_t P,
                       size_t W) {
  const uint64_t E = head.size();
  const uint64_t nt = slice_tiles(E, T);
  REQUIRE(nt * T >= E && (nt == 0 || (nt - 1) * T < E));
  std::vector<uint8_t> flags(nt * T, 0);  // whole tiles, zero past E
  for (uint64_t i = 0; i < E; ++i) flags[i] = head[i];
  std::vector<uint32_t> tbase(nt + 1, 0);
  for (uint64_t t = 0; t < nt; ++t) {
    uint32_t c = 0;
    for (uint64_t i = slice_tile_begin(t, T); i < slice_tile_end(t, T, E); ++i) c += flags[i];
    tbase[t + 1] = tbase[t] + c;
  }
  const uint64_t nv = tbase[nt];
  const std::vector<int64_t> want = brute<OP>(head, val);
  REQUIRE(want.size() == nv);
  std::vector<int64_t> out(nv, 0);
  std::vector<int> written(nv, 0);
  std::vector<int64_t> lead(nt, 0), trail(nt, 0), carry(nt, 0);
  std::vector<int> lead_set(nt, 0), trail_set(nt, 0);
  const uint32_t threads = T / P;
  REQUIRE(threads * P == T);
  // the reduce launch
  for (uint64_t t = 0; t < nt; ++t) {
    const uint64_t tile_end = slice_tile_end(t, T, E);
    std::vector<SegPair> agg(threads);
    std::vector<std::vector<int64_t>> v(threads, std::vector<int64_t>(P));
    for (uint32_t th = 0; th < threads; ++th) {
      const uint64_t i0 = slice_tile_begin(t, T) + (uint64_t)th * P;
      SegPair run = seg_identity<OP>();
      for (uint32_t k = 0; k < P; ++k) {
        if (i0 + k < E) {
          seg_push<OP>(run, flags[i0 + k] != 0, val[i0 + k]);
          v[th][k] = run.val;
        }
      }
      agg[th] = run;
    }
    SegPair total;
    const std::vector<SegPair> before = block_excl<OP>(agg, W, &total);
    REQUIRE(total.heads == tbase[t + 1] - tbase[t]);
    for (uint32_t th = 0; th < threads; ++th) {
      const uint64_t i0 = slice_tile_begin(t, T) + (uint64_t)th * P;
      uint32_t own = 0;
      for (uint32_t k = 0; k < P; ++k) {
        const uint64_t i = i0 + k;
        if (i >= E) continue;
        own += flags[i];
        const uint32_t heads_incl = before[th].heads + own;
        const int64_t incl = own ? v[th][k] : slice_op<OP>(before[th].val, v[th][k]);
        const bool next_head = i + 1 < E && flags[i + 1] != 0;  // (inside the flag array: i + 1 < E)
        const bool last = i + 1 == tile_end;
        const int emit = slice_emit(heads_incl, slice_closed(i, E, next_head), last);
        if (emit == kSliceEmitOut) {
          const uint64_t pos = slice_out_rank(tbase[t], heads_incl);
          REQUIRE(pos < nv);
          out[pos] = incl;
          ++written[pos];
        } else if (emit == kSliceEmitLead) {
          REQUIRE(!lead_set[t]);
          lead[t] = incl;
          lead_set[t] = 1;
        }
        if (last) {
          REQUIRE(!trail_set[t]);
          trail[t] = incl;
          trail_set[t] = 1;
        }
      }
    }
    REQUIRE(trail_set[t]);
  }
  // the carry launch: one workgroup, chunks of `threads` records
  SegPair run = seg_identity<OP>();
  for (uint64_t c0 = 0; c0 < nt; c0 += threads) {
    std::vector<SegPair> a(threads, seg_identity<OP>());
    for (uint32_t th = 0; th < threads && c0 + th < nt; ++th) {
      a[th].heads = tbase[c0 + th + 1] - tbase[c0 + th];
      a[th].val = trail[c0 + th];
    }
    SegPair total;
    const std::vector<SegPair> ex = block_excl<OP>(a, W, &total);
    for (uint32_t th = 0; th < threads && c0 + th < nt; ++th) carry[c0 + th] = seg_combine<OP>(run, ex[th]).val;
    run = seg_combine<OP>(run, total);
  }
  // the fix-up launch
  for (uint64_t t = 0; t < nt; ++t) {
    const uint64_t begin = slice_tile_begin(t, T), end = slice_tile_end(t, T, E);
    REQUIRE(begin < end);
    const bool closed = slice_closed(end - 1, E, end < E && flags[end] != 0);
    if (!slice_fixup(t, flags[begin] != 0, tbase[t + 1] - tbase[t], closed)) continue;
    REQUIRE(tbase[t] > 0 && lead_set[t]);
    const uint64_t pos = slice_fixup_rank(tbase[t]);
    REQUIRE(pos < nv);
    out[pos] = slice_op<OP>(carry[t], lead[t]);
    ++written[pos];
  }
  for (uint64_t k = 0; k < nv; ++k) {
    REQUIRE(written[k] == 1);
    REQUIRE(out[k] == want[k]);
  }
}

static void run_all_ops(const std::vector<uint8_t>& head, const std::vector<int64_t>& val, uint32_t T, uint32_t P,
                        size_t W) {
  run_window<kSliceSum>(head, val, T, P, W);
  run_window<kSliceMin>(head, val, T, P, W);
  run_window<kSliceMax>(head, val, T, P, W);
}

int main() {
  std::mt19937_64 rng(0x51CE);
  auto values = [&rng](size_t n) {
    std::vector<int64_t> v(n);
    for (auto& x : v) x = (int64_t)rng();
    return v;
  };
  // the operator itself
  REQUIRE(slice_op<kSliceSum>(kSliceI64Max, 1) == kSliceI64Min);  // wraps
  REQUIRE(slice_op<kSliceSum>(kSliceI64Min, -1) == kSliceI64Max);
  REQUIRE(slice_op<kSliceMin>(kSliceI64Min, kSliceI64Max) == kSliceI64Min);
  REQUIRE(slice_op<kSliceMax>(kSliceI64Min, kSliceI64Max) == kSliceI64Max);
  REQUIRE(slice_op<kSliceMin>(slice_identity<kSliceMin>(), 7) == 7);
  REQUIRE(slice_op<kSliceMax>(slice_identity<kSliceMax>(), -7) == -7);
  for (int it = 0; it < 2000; ++it) {  // seg_combine is associative
    SegPair p[3];
    for (auto& q : p) {
      q.heads = (uint32_t)(rng() % 3);
      q.val = (int64_t)rng();
    }
    const SegPair l = seg_combine<kSliceSum>(seg_combine<kSliceSum>(p[0], p[1]), p[2]);
    const SegPair r = seg_combine<kSliceSum>(p[0], seg_combine<kSliceSum>(p[1], p[2]));
    REQUIRE(l.heads == r.heads && l.val == r.val);
    const SegPair lm = seg_combine<kSliceMin>(seg_combine<kSliceMin>(p[0], p[1]), p[2]);
    const SegPair rm = seg_combine<kSliceMin>(p[0], seg_combine<kSliceMin>(p[1], p[2]));
    REQUIRE(lm.heads == rm.heads && lm.val == rm.val);
  }
  // entries, edges, keys
  REQUIRE(slice_entries(5, kSliceOut) == 5 && slice_entries(5, kSliceIn) == 5 && slice_entries(5, kSliceAll) == 10);
  REQUIRE(slice_edge_of(7, kSliceOut) == 7 && slice_edge_of(7, kSliceAll) == 3 && slice_edge_of(6, kSliceAll) == 3);
  REQUIRE(slice_key_is_src(7, kSliceOut) && !slice_key_is_src(7, kSliceIn));
  REQUIRE(slice_key_is_src(6, kSliceAll) && !slice_key_is_src(7, kSliceAll));
  REQUIRE(slice_tiles(0, 8) == 0 && slice_tiles(1, 8) == 1 && slice_tiles(8, 8) == 1 && slice_tiles(9, 8) == 2);
  REQUIRE(slice_tiles(0xFFFFFFFFull, 2048) == (1ull << 21));
  REQUIRE(slice_tile_end((1ull << 21) - 1, 2048, 0xFFFFFFFFull) == 0xFFFFFFFFull);

  // empty input and one entry
  run_all_ops({}, {}, 8, 2, 2);
  run_all_ops({1}, {42}, 8, 2, 2);
  run_all_ops({1}, {kSliceI64Min}, 8, 2, 2);
  // every head pattern over 2 tiles of 6 (position 0 is a head), and every shorter window
  for (uint32_t E = 1; E <= 12; ++E) {
    const std::vector<int64_t> val = values(E);
    for (uint32_t m = 0; m < (1u << (E - 1)); ++m) {
      std::vector<uint8_t> head(E);
      head[0] = 1;
      for (uint32_t i = 1; i < E; ++i) head[i] = (m >> (i - 1)) & 1;
      run_all_ops(head, val, 6, 2, 2);
      if (E == 12) run_all_ops(head, val, 6, 3, 2);
    }
  }
  // 10^4 random patterns over 5 tiles of 8, heads sparse to dense
  for (int it = 0; it < 10000; ++it) {
    const uint32_t E = 33 + (uint32_t)(rng() % 8);
    const uint32_t density = 1 + (uint32_t)(rng() % 16);
    std::vector<uint8_t> head(E);
    for (auto& h : head) h = rng() % 16 < density ? 1 : 0;
    head[0] = 1;
    run_all_ops(head, values(E), 8, 2, 2);
  }
  // one segment covering all tiles (3 of 8, whole and with a ragged end)
  for (uint32_t E : {17u, 23u, 24u}) {
    std::vector<uint8_t> head(E, 0);
    head[0] = 1;
    run_all_ops(head, values(E), 8, 2, 2);
    run_all_ops(head, values(E), 8, 4, 2);
  }
  // a head exactly on a tile's first position: the run before it ends with its tile, whole
  // tiles long (its carry must not leak) or not
  for (uint32_t first : {8u, 16u}) {
    for (uint32_t start : {0u, 3u, 8u}) {
      if (start >= first) continue;
      std::vector<uint8_t> head(24, 0);
      head[0] = 1;
      head[start] = 1;
      head[first] = 1;
      run_all_ops(head, values(24), 8, 2, 2);
      head[first + 1] = 1;
      run_all_ops(head, values(24), 8, 2, 2);
    }
  }
  // the int64 extremes as values under each op
  {
    const int64_t ext[4] = {kSliceI64Min, kSliceI64Max, -1, 0};
    for (int it = 0; it < 2000; ++it) {
      const uint32_t E = 1 + (uint32_t)(rng() % 24);
      std::vector<uint8_t> head(E);
      std::vector<int64_t> val(E);
      for (uint32_t i = 0; i < E; ++i) {
        head[i] = rng() % 4 == 0;
        val[i] = ext[rng() % 4];
      }
      head[0] = 1;
      run_all_ops(head, val, 8, 2, 2);
    }
  }
  // the kernels' own shape at a small scale: waves of 64 threads, 8 positions each
  for (int it = 0; it < 20; ++it) {
    const uint32_t E = 2048 * 2 + (uint32_t)(rng() % 2049);
    std::vector<uint8_t> head(E);
    const uint32_t every = 1 + (uint32_t)(rng() % 3000);
    for (auto& h : head) h = rng() % every == 0;
    head[0] = 1;
    run_all_ops(head, values(E), 2048, 8, 64);
  }
  std::printf("all checks passed (%ld)\n", checks);
  return 0;
}
