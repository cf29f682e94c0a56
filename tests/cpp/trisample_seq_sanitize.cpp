// The rules header of the sampling triangle estimate (csrc/gs_trisample_seq.hpp) in a stand-alone
// host program, built with the address and undefined-behaviour sanitizers by
// tests/test_trisample_seq.py: three published values of java.util.Random, the jump-ahead against
// stepping, the Java int cast, the sure-failure test of the coin against the coin, and
// ts_fold_parts against ts_fold_seq under chunk and tile sizes 1, 2, 64 and n. The pinned values
// are printed as "PIN <name> <values>" lines; the Python test compares them with
// tests/golden/trisample_pins.json. Exit status 0 and "all checks passed" when every check holds.
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "gs_trisample_seq.hpp"

using namespace gs;

static int failures = 0;

static void expect(bool ok, const std::string& what) {
  if (!ok) {
    std::printf("FAIL %s\n", what.c_str());
    ++failures;
  }
}

static bool same_state(const TsState& a, const TsState& b) {
  return a.src == b.src && a.trg == b.trg && a.third == b.third && a.sampled_at == b.sampled_at && a.flags == b.flags;
}

static bool same(const TsSeq& a, const TsSeq& b, const std::vector<TsRow>& ra, const std::vector<TsRow>& rb) {
  if (a.folded != b.folded || a.beta_sum != b.beta_sum || a.last_estimate != b.last_estimate) return false;
  if (a.coins != b.coins || a.max_attempts != b.max_attempts || a.lcg != b.lcg || ra.size() != rb.size()) return false;
  for (size_t i = 0; i < a.st.size(); ++i)
    if (!same_state(a.st[i], b.st[i])) return false;
  for (size_t i = 0; i < ra.size(); ++i)
    if (ra[i].edges != rb[i].edges || ra[i].estimate != rb[i].estimate || ra[i].beta_sum != rb[i].beta_sum) return false;
  return true;
}

struct Stream {
  std::vector<int64_t> s, d;
};

static Stream complete_graph(int v, int times) {
  Stream e;
  for (int r = 0; r < times; ++r)
    for (int a = 0; a < v; ++a)
      for (int b = a + 1; b < v; ++b) {
        e.s.push_back(a);
        e.d.push_back(b);
      }
  return e;
}

// parts == seq on the stream cut at `cuts`, under the given chunk and tile
static void check_parts(const Stream& e, uint32_t S, int32_t V, const std::vector<size_t>& cuts, uint32_t chunk,
                        uint32_t tile, const std::string& name) {
  TsSeq a(S, V, kTsDefaultSeed, 7), b(S, V, kTsDefaultSeed, 7);
  std::vector<size_t> bounds = {0};
  for (size_t c : cuts) bounds.push_back(c);
  bounds.push_back(e.s.size());
  for (size_t k = 0; k + 1 < bounds.size(); ++k) {
    const size_t lo = bounds[k], n = bounds[k + 1] - lo;
    std::vector<TsRow> ra, rb;
    ts_fold_seq(a, e.s.data() + lo, e.d.data() + lo, n, &ra);
    ts_fold_parts(b, e.s.data() + lo, e.d.data() + lo, n, chunk ? chunk : (uint32_t)(n ? n : 1),
                  tile ? tile : (uint32_t)(n ? n : 1), &rb);
    expect(same(a, b, ra, rb), name + " fold " + std::to_string(k));
  }
}

int main() {
  // java.util.Random
  {
    const uint64_t s0 = ts_step(ts_scramble(0));
    std::printf("PIN random0_next_int %d\n", ts_int_of(s0));
    std::printf("PIN random42_next_int %d\n", ts_int_of(ts_step(ts_scramble(42))));
    std::printf("PIN random0_next_double %.15f\n", ts_double_of(ts_hi_of(s0), ts_lo_of(ts_step(s0))));
    std::printf("PIN instance_seeds");
    TsSeq q(8, 5, kTsDefaultSeed, 0);
    for (uint32_t i = 0; i < 8; ++i) {
      std::printf(" %lld", (long long)ts_instance_seed(kTsDefaultSeed, i));
      expect(q.lcg[i] == ts_instance_state(kTsDefaultSeed, i), "instance state by jump == by stepping");
    }
    std::printf("\n");
    for (uint32_t i = 0; i < 4; ++i) {
      std::printf("PIN coin_successes_%u", i);
      ts_coin_lane(q.lcg[i], 1, 2000, [&](uint32_t k, bool ok) {
        if (ok) std::printf(" %u", k + 1);
      });
      std::printf("\n");
    }
  }
  // jump-ahead against stepping
  for (uint64_t k : {0ull, 1ull, 2ull, (1ull << 20) + 1, 1ull << 47}) {
    const TsAffine f = ts_jump(k);
    uint64_t s = ts_scramble(12345);
    if (k <= (1ull << 20) + 1) {
      uint64_t w = s;
      for (uint64_t i = 0; i < k; ++i) w = ts_step(w);
      expect(ts_apply(f, s) == w, "jump == steps, k = " + std::to_string(k));
    } else {  // 2^47 = (2^20 + 1 steps) cannot be stepped: jump(k) == jump(k / 2) twice, and the LCG's period is 2^48
      const TsAffine h = ts_jump(k / 2);
      expect(ts_apply(f, s) == ts_apply(h, ts_apply(h, s)), "jump(2^47) == jump(2^46) twice");
      expect(ts_apply(f, ts_apply(f, s)) == s, "jump(2^47) twice is the identity (period 2^48)");
      expect(ts_apply(f, s) != s, "jump(2^47) is not the identity");
    }
    const TsAffine g = ts_then(f, ts_jump(3));
    expect(ts_apply(g, s) == ts_step(ts_step(ts_step(ts_apply(f, s)))), "composition, k = " + std::to_string(k));
  }
  // the Java int cast
  expect(ts_java_int(2147483648.0) == 2147483647 && ts_java_int(1e300) == 2147483647, "cast saturates above");
  expect(ts_java_int(2147483646.9) == 2147483646 && ts_java_int(3.99) == 3, "cast truncates");
  expect(ts_java_int(-3.99) == -3 && ts_java_int(-0.5) == 0, "cast truncates towards zero");
  expect(ts_java_int(-2147483649.0) == -2147483647 - 1 && ts_java_int(-1e300) == -2147483647 - 1, "cast saturates below");
  expect(ts_java_int(std::nan("")) == 0, "NaN -> 0");
  expect(ts_java_int(std::numeric_limits<double>::infinity()) == 2147483647, "inf saturates");
  expect(ts_estimate(1.0 / 4, 3, 19, 5) == 42, "estimate of pin 3's last row");
  expect(ts_estimate(1.0, 1 << 20, 2147483647, 2147483647) == 2147483647, "estimate saturates");
  // a sure failure is a failure: hi at and around the threshold for many t, lo at both ends
  for (uint32_t t = 1; t <= 5000; ++t) {
    const uint32_t thr = (uint32_t)((1ull << 26) / t);
    for (uint32_t d = 0; d < 6; ++d) {
      const uint32_t hi = thr + d < (1u << 26) ? thr + d : (1u << 26) - 1;
      for (uint32_t lo : {0u, (1u << 27) - 1})
        if (ts_coin_rejects(hi, t)) expect(!ts_coin(hi, lo, t), "rejects implies fails, t = " + std::to_string(t));
    }
    expect(!ts_coin_rejects(thr > 0 ? thr - 1 : 0, t) || t > (1u << 26), "no rejection below the threshold");
  }
  expect(!ts_coin_rejects((1u << 26) - 1, 1) && ts_coin((1u << 26) - 1, (1u << 27) - 1, 1), "always true at t = 1");
  expect(ts_coin_rejects(3, 2147483647u) && !ts_coin(3, 0, 2147483647u) && !ts_coin(1, 0, 2147483647u) &&
             ts_coin(0, 0, 2147483647u),
         "t = 2^31 - 1");
  // pin 3: K5 twice
  {
    const Stream e = complete_graph(5, 2);
    TsSeq q(4, 5, kTsDefaultSeed, 0);
    std::vector<TsRow> rows;
    ts_fold_seq(q, e.s.data(), e.d.data(), e.s.size(), &rows);
    std::printf("PIN k5_rows");
    for (const TsRow& r : rows) std::printf(" %d %d", r.edges, r.estimate);
    std::printf("\nPIN k5_beta_sum %d\nPIN k5_max_attempts %u\n", q.beta_sum, q.max_attempts);
    for (uint32_t i = 0; i < 4; ++i)
      std::printf("PIN k5_state_%u %lld %lld %lld %u %u %u %d\n", i, (long long)q.st[i].src, (long long)q.st[i].trg,
                  (long long)q.st[i].third, q.st[i].flags & 1u, (q.st[i].flags >> 1) & 1u, (q.st[i].flags >> 2) & 1u,
                  q.st[i].sampled_at);
  }
  // parts == seq
  {
    const Stream k5 = complete_graph(5, 2), k16 = complete_graph(16, 1), k7 = complete_graph(7, 4);
    for (uint32_t chunk : {1u, 2u, 64u, 0u})  // 0: n
      for (uint32_t tile : {1u, 2u, 64u, 0u}) {
        const std::string tag = " chunk " + std::to_string(chunk) + " tile " + std::to_string(tile);
        check_parts(k5, 4, 5, {}, chunk, tile, "k5" + tag);
        check_parts(k5, 4, 5, {1, 2, 7, 8, 15}, chunk, tile, "k5 cut" + tag);
        check_parts(k16, 200, 16, {}, chunk, tile, "k16" + tag);
        check_parts(k16, 65, 16, {63, 64, 65}, chunk, tile, "k16 cut" + tag);
        check_parts(k7, 33, 7, {40}, chunk, tile, "k7 x4" + tag);
      }
    // corners: a self-loop sampled at t = 1 and one edge to its third vertex; ids outside [0, vertices)
    for (uint64_t third_seed = 0; third_seed < 4; ++third_seed) {
      TsSeq a(3, 3, kTsDefaultSeed, third_seed), b(3, 3, kTsDefaultSeed, third_seed);
      const int64_t third = [&] {
        uint32_t att;
        return ts_third(third_seed, 0, 1, 3, 1, 1, &att);
      }();
      Stream e;
      e.s = {1, third, -5, 1000};
      e.d = {1, 1, 1000, -5};
      std::vector<TsRow> ra, rb;
      ts_fold_seq(a, e.s.data(), e.d.data(), 4, &ra);
      ts_fold_parts(b, e.s.data(), e.d.data(), 4, 2, 1, &rb);
      expect(same(a, b, ra, rb), "self-loop stream");
      // instance 0 sampled (1, 1) at t = 1 unless resampled at t = 2; the one edge sets both flags
      if (a.st[0].sampled_at == 1) expect(a.st[0].flags == 7u, "one edge closes a self-loop candidate");
    }
  }
  if (failures == 0) std::printf("all checks passed\n");
  return failures ? 1 : 0;
}
