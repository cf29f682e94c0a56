// TriangleEstimate and BroadcastTriangleCount on the C++ host mirror (gelly_streaming.hpp ->
// libgs_summary.so) against the sequential definition of csrc/gs_trisample_seq.hpp
// (ts_fold_seq): the reference's default stream -- (k, (k + 2) % 1000) and (k, (k + 4) % 1000),
// k = 0 .. 999 -- at 256 samples, K16 at 2048 samples, batch sizes 1, 7 and the whole stream, and
// the K5 pin of tests/golden/trisample_pins.json. Exit status 0 when every check passes.
#include <cstdio>
#include <string>
#include <vector>

#include "gelly_streaming.hpp"
#include "gs_trisample_seq.hpp"

using namespace gelly;

static int failures = 0;

static void expect(bool ok, const std::string& name) {
  std::printf("%s %s\n", ok ? "PASS" : "FAIL", name.c_str());
  if (!ok) ++failures;
}

using Rows = std::vector<std::pair<int, int>>;
using Stream = EdgeStream<int64_t, NullValue>;

static Stream default_stream() {
  Stream s;
  for (int64_t k = 0; k < 1000; ++k) {
    s.edges.push_back({k, (k + 2) % 1000, NullValue()});
    s.edges.push_back({k, (k + 4) % 1000, NullValue()});
  }
  return s;
}

static Stream complete_graph(int v, int times) {
  Stream s;
  for (int r = 0; r < times; ++r)
    for (int64_t a = 0; a < v; ++a)
      for (int64_t b = a + 1; b < v; ++b) s.edges.push_back({a, b, NullValue()});
  return s;
}

static Rows model(const Stream& s, uint32_t samples, int32_t vertices, gs::TsSeq* out = nullptr) {
  gs::TsSeq q(samples, vertices, gs::kTsDefaultSeed, 0);
  std::vector<int64_t> a, b;
  for (const auto& e : s.edges) {
    a.push_back(e.f0);
    b.push_back(e.f1);
  }
  std::vector<gs::TsRow> rows;
  gs::ts_fold_seq(q, a.data(), b.data(), a.size(), &rows);
  Rows r;
  for (const gs::TsRow& x : rows) r.push_back({x.edges, x.estimate});
  if (out) *out = q;
  return r;
}

int main() {
  try {
    {
      const Stream s = default_stream();
      gs::TsSeq q(1, 3, 0, 0);
      const Rows want = model(s, 256, 1000, &q);
      BroadcastTriangleCount c(256, 1000);
      const Rows got = c.run(s);
      expect(got == want, "BroadcastTriangleCount.defaultStream");
      const auto e = c.estimate();
      expect(std::get<0>(e) == 2000 && std::get<1>(e) == q.beta_sum && std::get<2>(e) == q.last_estimate,
             "BroadcastTriangleCount.defaultStream.estimate");
      BroadcastTriangleCount c7(256, 1000);
      expect(c7.run(s, 7) == want, "BroadcastTriangleCount.defaultStream.batch7");
    }
    {
      const Stream s = complete_graph(16, 1);
      const Rows want = model(s, 2048, 16);
      BroadcastTriangleCount c(2048, 16);
      const Rows got = c.run(s);
      expect(got == want && want.size() == 100, "BroadcastTriangleCount.k16");
      bool same = c.estimates().size() == got.size();
      for (size_t i = 0; same && i < got.size(); ++i)
        same = c.estimates()[i].getSource() == 0 && c.estimates()[i].getEdgeCount() == got[i].first &&
               c.estimates()[i].getBeta() >= 0;
      expect(same, "TriangleEstimate.accessors");
      BroadcastTriangleCount c1(2048, 16);
      expect(c1.run(s, 1) == want, "BroadcastTriangleCount.k16.batch1");
    }
    {
      BroadcastTriangleCount c(4, 5);
      const Rows want = {{8, 6}, {13, 19}, {15, 11}, {16, 24}, {19, 42}};
      expect(c.run(complete_graph(5, 2), 3) == want, "BroadcastTriangleCount.k5Pin");
    }
    {
      bool threw = false;
      try {
        BroadcastTriangleCount bad(10, 2);
      } catch (const GsException& e) {
        threw = e.code() == GS_ERR_INVALID;
      }
      expect(threw, "BroadcastTriangleCount.rejectsTwoVertices");
    }
  } catch (const std::exception& e) {
    std::printf("FAIL exception: %s\n", e.what());
    ++failures;
  }
  std::printf("%d failure(s)\n", failures);
  return failures ? 1 : 0;
}
