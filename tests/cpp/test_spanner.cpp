// AdjacencyListGraph and Spanner on the C++ host mirror (gelly_streaming.hpp -> libgs_summary.so).
// The pinned sequences are the reference's own, the same data as tests/golden/spanner_pins.json:
//   testBoundedBFS, testAddEdge   util/AdjacencyListGraphTest.java:31-87
//   default stream, k = 3         example/SpannerExample.java:80, 123-135
// The windowed aggregation and CombineSpanners are checked against the sequential restatement of
// csrc/gs_spanner_seq.hpp driven the way SummaryBulkAggregation drives the summary: a partial
// spanner per window, reduced into the running one (library/Spanner.java:92-116).
// Exit status 0 when every check passes.
#include <cstdio>
#include <string>
#include <vector>

#include "gelly_streaming.hpp"
#include "gs_spanner_seq.hpp"

using namespace gelly;

static int failures = 0;

static void expect(bool ok, const std::string& name) {
  std::printf("%s %s\n", ok ? "PASS" : "FAIL", name.c_str());
  if (!ok) ++failures;
}

using Edges = std::vector<std::pair<int64_t, int64_t>>;

// CombineSpanners.reduce on the restatement: returns 1 when g1 took g2's edges, 2 otherwise
static int model_reduce(gs::SpannerSeq& g1, gs::SpannerSeq& g2) {
  gs::SpannerSeq& into = g1.vertices() > g2.vertices() ? g1 : g2;
  gs::SpannerSeq& from = g1.vertices() > g2.vertices() ? g2 : g1;
  for (const auto& e : from.sorted_edges()) into.fold(&e.first, &e.second, 1, nullptr);
  return &into == &g1 ? 1 : 2;
}

static void fill(AdjacencyListGraph& g, gs::SpannerSeq& m, const Edges& edges) {
  for (const auto& e : edges) {
    g.updateLocal(e.first, e.second);
    m.fold(&e.first, &e.second, 1, nullptr);
  }
}

int main() {
  try {
    {  // AdjacencyListGraphTest.testBoundedBFS
      AdjacencyListGraph g;
      g.reset();
      g.addEdge(1, 4);
      g.addEdge(4, 5);
      g.addEdge(5, 6);
      g.addEdge(4, 7);
      g.addEdge(7, 8);
      bool ok = g.boundedBFS(2, 3, 3) == false;
      g.addEdge(2, 3);
      ok = ok && g.boundedBFS(3, 4, 3) == false;
      g.addEdge(3, 4);
      ok = ok && g.boundedBFS(3, 6, 3) == true;
      ok = ok && g.boundedBFS(8, 9, 3) == false;
      g.addEdge(8, 9);
      ok = ok && g.boundedBFS(8, 6, 3) == false;
      g.addEdge(8, 6);
      ok = ok && g.boundedBFS(5, 9, 3) == true;
      expect(ok, "AdjacencyListGraphTest.testBoundedBFS");
    }
    {  // AdjacencyListGraphTest.testAddEdge
      AdjacencyListGraph g;
      g.addEdge(1, 2);
      auto m = g.getAdjacencyMap();
      bool ok = m.size() == 2 && m[1].count(2) && m[2].count(1) && m[1].size() == 1 && m[2].size() == 1;
      g.addEdge(1, 3);
      m = g.getAdjacencyMap();
      ok = ok && m.size() == 3 && m[1].count(2) && m[1].count(3) && m[3].count(1);
      g.addEdge(3, 1);
      m = g.getAdjacencyMap();
      ok = ok && m.size() == 3 && m[1].size() == 2 && m[3].size() == 1;
      g.addEdge(1, 2);
      m = g.getAdjacencyMap();
      ok = ok && m.size() == 3 && m[1].size() == 2 && m[2].size() == 1;
      // addEdge does not ask for the distance: 2 - 3 closes a triangle
      g.addEdge(2, 3);
      ok = ok && g.getAdjacencyMap()[2].size() == 2 && g.size() == 3;
      g.reset();
      ok = ok && g.getAdjacencyMap().empty() && g.size() == 0;
      expect(ok, "AdjacencyListGraphTest.testAddEdge");
    }
    const int64_t def[12][2] = {{1, 4}, {4, 7}, {7, 8}, {4, 8}, {4, 5}, {5, 6},
                                {2, 3}, {3, 4}, {3, 6}, {8, 9}, {6, 8}, {5, 9}};
    {  // the default stream as one window: UpdateLocal in arrival order
      EdgeStream<int64_t, NullValue> s;
      for (const auto& r : def) s.edges.push_back({r[0], r[1], NullValue{}});
      SimpleEdgeStream<int64_t, NullValue> edges(s);
      Spanner<NullValue> spanner(1000, 3);
      Edges got;
      int emissions = 0;
      edges.aggregate(spanner, [&](const AdjacencyListGraphRef& g) {
        got = g->edges();
        ++emissions;
      });
      const Edges want = {{1, 4}, {2, 3}, {3, 4}, {4, 5}, {4, 7}, {5, 6}, {6, 8}, {7, 8}, {8, 9}};
      expect(emissions == 1 && got == want, "SpannerExample.defaultStream");
    }
    {  // windows of 4 edges: a partial spanner per window, reduced into the running one
      EdgeStream<int64_t, NullValue> s;
      for (int i = 0; i < 12; ++i) {
        s.edges.push_back({def[i][0], def[i][1], NullValue{}});
        s.timestamps.push_back((i / 4) * 1000 + 10 * (i % 4));
      }
      SimpleEdgeStream<int64_t, NullValue> edges(s);
      Spanner<NullValue> spanner(1000, 3);
      std::vector<Edges> got;
      edges.aggregate(spanner, [&](const AdjacencyListGraphRef& g) { got.push_back(g->edges()); });
      std::vector<Edges> want;
      gs::SpannerSeq running(3);
      gs::SpannerSeq* run = &running;
      std::vector<gs::SpannerSeq> partial(3, gs::SpannerSeq(3));
      for (int w = 0; w < 3; ++w) {
        for (int i = 4 * w; i < 4 * w + 4; ++i) partial[(size_t)w].fold(&def[i][0], &def[i][1], 1, nullptr);
        run = model_reduce(partial[(size_t)w], *run) == 1 ? &partial[(size_t)w] : run;
        want.push_back(run->sorted_edges());
      }
      expect(got == want && got.size() == 3, "Spanner.aggregate.windowsOfFour");
      bool spans = true;  // the property itself: every streamed edge is within 3 in the last emission
      AdjacencyListGraph check;
      for (const auto& e : got.back()) check.addEdge(e.first, e.second);
      for (const auto& r : def) spans = spans && check.boundedBFS(r[0], r[1], 3);
      expect(spans, "Spanner.aggregate.spansTheStream");
    }
    {  // CombineSpanners.reduce: strictly more vertices takes the other's edges, a tie goes to g2
      const Edges small = {{1, 2}, {2, 3}}, big = {{3, 4}, {4, 5}, {5, 1}, {5, 6}}, other = {{7, 1}, {3, 7}};
      Spanner<NullValue>::CombineSpanners combine;
      struct Case {
        const Edges *e1, *e2;
        int taker;
        const char* name;
      } cases[] = {{&big, &small, 1, "CombineSpanners.reduce.moreVertices"},
                   {&small, &big, 2, "CombineSpanners.reduce.fewerVertices"},
                   {&small, &other, 2, "CombineSpanners.reduce.tie"}};
      for (const Case& c : cases) {
        auto g1 = std::make_shared<AdjacencyListGraph>(3), g2 = std::make_shared<AdjacencyListGraph>(3);
        gs::SpannerSeq m1(3), m2(3);
        fill(*g1, m1, *c.e1);
        fill(*g2, m2, *c.e2);
        const Edges before1 = g1->edges(), before2 = g2->edges();
        const AdjacencyListGraphRef r = combine.reduce(g1, g2);
        const int taker = model_reduce(m1, m2);
        bool ok = taker == c.taker && r == (taker == 1 ? g1 : g2);
        ok = ok && g1->edges() == m1.sorted_edges() && g2->edges() == m2.sorted_edges();
        ok = ok && (taker == 1 ? g2->edges() == before2 : g1->edges() == before1);
        ok = ok && r->edges().size() > (taker == 1 ? before1 : before2).size();
        expect(ok, c.name);
      }
    }
  } catch (const std::exception& e) {
    std::printf("FAIL exception: %s\n", e.what());
    ++failures;
  }
  std::printf("%d failure(s)\n", failures);
  return failures ? 1 : 0;
}
