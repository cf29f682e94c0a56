// SimpleEdgeStream::distinct and getVertices on the C++ host mirror (gelly_streaming.hpp ->
// libgs_summary.so). The expected values are the reference's own, the same numbers as
// tests/golden/distinct_pins.json:
//   the seven edges   GraphStreamTestUtils.java:56-67
//   distinct          TestDistinct.java:38-51 (the input twice, the seven expected rows)
//   getVertices       TestGetVertices.java:38-42
// The reference compares sorted lines; the mirror emits in arrival order, which for these inputs
// is the sorted order, so the rows are compared as they come.
// Exit status 0 when every check passes.
#include <cstdio>
#include <string>
#include <vector>

#include "gelly_streaming.hpp"

using namespace gelly;

static int failures = 0;

static void expect(bool ok, const std::string& name) {
  std::printf("%s %s\n", ok ? "PASS" : "FAIL", name.c_str());
  if (!ok) ++failures;
}

template <typename EV>
static bool same_rows(const EdgeStream<int64_t, EV>& got, const std::vector<std::vector<int64_t>>& want) {
  if (got.edges.size() != want.size()) return false;
  for (size_t i = 0; i < want.size(); ++i)
    if (got.edges[i].f0 != want[i][0] || got.edges[i].f1 != want[i][1] || (int64_t)got.edges[i].f2 != want[i][2])
      return false;
  return true;
}

int main() {
  try {
    const std::vector<std::vector<int64_t>> rows = {{1, 2, 12}, {1, 3, 13}, {2, 3, 23}, {3, 4, 34},
                                                    {3, 5, 35}, {4, 5, 45}, {5, 1, 51}};
    // TestDistinct: edges.addAll(getLongLongEdges()) -- the seven edges twice
    EdgeStream<int64_t, int64_t> twice;
    for (int rep = 0; rep < 2; ++rep)
      for (const auto& r : rows) twice.edges.push_back({r[0], r[1], r[2]});
    const SimpleEdgeStream<int64_t, int64_t> graph(twice);
    expect(same_rows(graph.distinct().getEdges(), rows), "TestDistinct.test");

    // TestGetVertices: 1..5, each once
    EdgeStream<int64_t, int64_t> once;
    for (const auto& r : rows) once.edges.push_back({r[0], r[1], r[2]});
    const SimpleEdgeStream<int64_t, int64_t> g1(once);
    const auto vs = g1.getVertices();
    bool ok = vs.size() == 5;
    for (size_t k = 0; ok && k < 5; ++k) ok = vs[k].getId() == (int64_t)k + 1;
    expect(ok, "TestGetVertices.test");
    expect(graph.getVertices().size() == 5, "Distinct.getVertices.doubledStream");

    // values and timestamps of the kept edges are those of the first occurrence
    EdgeStream<int64_t, int64_t> ts;
    ts.edges = {{7, 8, 100}, {8, 7, 200}, {7, 8, 300}, {9, 9, 400}, {8, 7, 500}, {9, 9, 600}, {7, 9, 700}};
    ts.timestamps = {10, 20, 30, 40, 50, 60, 70};
    const SimpleEdgeStream<int64_t, int64_t> tg(ts);
    const SimpleEdgeStream<int64_t, int64_t> td = tg.distinct();
    expect(same_rows(td.getEdges(), {{7, 8, 100}, {8, 7, 200}, {9, 9, 400}, {7, 9, 700}}), "Distinct.values.firstKept");
    expect(td.getEdges().timestamps == std::vector<int64_t>({10, 20, 40, 70}), "Distinct.timestamps.firstKept");
    // distinct of a distinct stream is the same stream
    expect(same_rows(td.distinct().getEdges(), {{7, 8, 100}, {8, 7, 200}, {9, 9, 400}, {7, 9, 700}}),
           "Distinct.idempotent");

    // a two-fold stream through the C ABI: the second fold sees the first one's state
    gs_distinct d = nullptr;
    gs_check(gs_distinct_create(&d, 0, GS_DISTINCT_DIRECTED, 0, 0));
    const int64_t s1[3] = {1, 1, 2}, d1[3] = {2, 3, 3};
    const int64_t s2[4] = {2, 3, 1, 6}, d2[4] = {3, 4, 2, 6};
    gs_check(gs_distinct_fold(d, s1, d1, 3));
    gs_check(gs_distinct_fold(d, s2, d2, 4));
    uint32_t idx[4];
    int64_t es[4], ed[4], nvv[8];
    uint32_t ent[8];
    size_t ne = 0, nv = 0;
    gs_check(gs_distinct_new_edges(d, idx, es, ed, 4, &ne));
    gs_check(gs_distinct_new_vertices(d, nvv, ent, 8, &nv));
    expect(ne == 2 && idx[0] == 1 && idx[1] == 3 && es[0] == 3 && ed[0] == 4 && es[1] == 6 && ed[1] == 6,
           "Distinct.twoFolds.newEdges");
    expect(nv == 2 && nvv[0] == 4 && ent[0] == 3 && nvv[1] == 6 && ent[1] == 6, "Distinct.twoFolds.newVertices");
    uint64_t tv = 0, te = 0, tf = 0, lv = 0, le = 0;
    gs_check(gs_distinct_size(d, &tv, &te, &tf, &lv, &le));
    expect(tv == 5 && te == 5 && tf == 7 && lv == 2 && le == 2, "Distinct.twoFolds.size");
    int64_t as[5], ad[5];
    uint64_t first[5];
    size_t na = 0;
    gs_check(gs_distinct_edges(d, as, ad, first, 5, &na));
    const uint64_t want_first[5] = {0, 1, 2, 4, 6};
    bool fo = na == 5;
    for (size_t k = 0; fo && k < 5; ++k) fo = first[k] == want_first[k];
    expect(fo && as[3] == 3 && ad[3] == 4 && as[4] == 6 && ad[4] == 6, "Distinct.twoFolds.edges");
    gs_check(gs_distinct_destroy(d));
  } catch (const std::exception& e) {
    std::printf("FAIL exception: %s\n", e.what());
    ++failures;
  }
  std::printf("%d failure(s)\n", failures);
  return failures ? 1 : 0;
}
