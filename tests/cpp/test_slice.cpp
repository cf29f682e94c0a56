// SimpleEdgeStream::slice and its SnapshotStream on the C++ host mirror (gelly_streaming.hpp ->
// libgs_summary.so). The expected values are the reference's own, the same numbers as
// tests/golden/slice_pins.json:
//   the seven edges                GraphStreamTestUtils.java:56-64
//   foldNeighbors / reduceOnEdges  TestSlice.java:43-47 (OUT), 61-65 (IN), 79-83 (ALL)
//   applyOnNeighbors               TestSlice.java:151-155 (OUT), 169-173 (IN), 187-191 (ALL),
//                                  big when the sum of the edge values is > 50 (:231)
// The reference compares sorted lines (compareResultsByLinesInMemory); the mirror emits the
// vertices of a window in ascending order, so the rows are compared as they come.
// Exit status 0 when every check passes.
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "gelly_streaming.hpp"

using namespace gelly;

static int failures = 0;

static void expect(bool ok, const std::string& name) {
  std::printf("%s %s\n", ok ? "PASS" : "FAIL", name.c_str());
  if (!ok) ++failures;
}

using Sums = std::vector<std::pair<int64_t, int64_t>>;
using Labels = std::vector<std::pair<int64_t, std::string>>;

int main() {
  try {
    EdgeStream<int64_t, int64_t> data;
    const int64_t rows[7][3] = {{1, 2, 12}, {1, 3, 13}, {2, 3, 23}, {3, 4, 34}, {3, 5, 35}, {4, 5, 45}, {5, 1, 51}};
    for (const auto& r : rows) data.edges.push_back({r[0], r[1], r[2]});
    const SimpleEdgeStream<int64_t, int64_t> graph(data);

    const Sums sum_out = {{1, 25}, {2, 23}, {3, 69}, {4, 45}, {5, 51}};
    const Sums sum_in = {{1, 51}, {2, 12}, {3, 36}, {4, 34}, {5, 80}};
    const Sums sum_all = {{1, 76}, {2, 35}, {3, 105}, {4, 79}, {5, 131}};
    const Labels apply_out = {{1, "small"}, {2, "small"}, {3, "big"}, {4, "small"}, {5, "big"}};
    const Labels apply_in = {{1, "big"}, {2, "small"}, {3, "small"}, {4, "small"}, {5, "big"}};
    const Labels apply_all = {{1, "big"}, {2, "small"}, {3, "big"}, {4, "big"}, {5, "big"}};

    // SumEdgeValues (TestSlice.java:204-211): (vertex, running sum)
    const auto sum_fold = [](std::pair<int64_t, int64_t> acc, int64_t vertex, int64_t, int64_t value) {
      return std::make_pair(vertex, acc.second + value);
    };
    // SumEdgeValuesApply (TestSlice.java:222-238)
    const auto big_small = [](int64_t vertex, const std::vector<std::pair<int64_t, int64_t>>& nb, Labels& out) {
      int64_t sum = 0;
      for (const auto& e : nb) sum += e.second;
      out.emplace_back(vertex, sum > 50 ? "big" : "small");
    };

    struct Case {
      const char* name;
      bool dflt;
      EdgeDirection dir;
      const Sums* sums;
      const Labels* labels;
    };
    const Case cases[3] = {{"Default", true, EdgeDirection::OUT, &sum_out, &apply_out},
                           {"In", false, EdgeDirection::IN, &sum_in, &apply_in},
                           {"All", false, EdgeDirection::ALL, &sum_all, &apply_all}};
    for (const Case& c : cases) {
      const SnapshotStream<int64_t, int64_t> s = c.dflt ? graph.slice(1000) : graph.slice(1000, c.dir);
      const std::string n = c.name;
      expect(s.foldNeighbors(std::make_pair(int64_t(0), int64_t(0)), sum_fold) == *c.sums,
             "TestSlice.testFoldNeighbors" + n);
      const bool device_op = s.reduceOnEdges(GS_SLICE_SUM) == *c.sums;
      const bool lambda = s.reduceOnEdges([](int64_t a, int64_t b) { return a + b; }) == *c.sums;
      expect(device_op && lambda, "TestSlice.testReduceOnNeighbors" + n);
      expect(s.applyOnNeighbors<std::pair<int64_t, std::string>>(big_small) == *c.labels,
             "TestSlice.testApplyOnNeighbors" + n);
    }

    // two windows: edges of one window never meet those of the other, in any method
    EdgeStream<int64_t, int64_t> two;
    two.edges = {{1, 2, 10}, {1, 3, 20}, {2, 1, 5}, {1, 2, 100}, {3, 1, 7}, {1, 9, 1000}};
    two.timestamps = {0, 400, 999, 1000, 1500, 1999};
    const SimpleEdgeStream<int64_t, int64_t> tg(two);
    const Sums two_out = {{1, 30}, {2, 5}, {1, 1100}, {3, 7}};
    expect(tg.slice(1000).reduceOnEdges(GS_SLICE_SUM) == two_out, "Slice.twoWindows.reduce");
    expect(tg.slice(1000).foldNeighbors(std::make_pair(int64_t(0), int64_t(0)), sum_fold) == two_out,
           "Slice.twoWindows.fold");
    const Sums two_count_all = {{1, 3}, {2, 2}, {3, 1}, {1, 3}, {2, 1}, {3, 1}, {9, 1}};
    expect(tg.slice(1000, EdgeDirection::ALL).reduceOnEdges(GS_SLICE_COUNT) == two_count_all,
           "Slice.twoWindows.countAll");
    const Sums one_window = {{1, 1130}, {2, 5}, {3, 7}};
    expect(tg.slice(0).reduceOnEdges(GS_SLICE_SUM) == one_window, "Slice.noWindowTime.oneWindow");
    // arrival order inside a neighbourhood: the neighbours of 1 as they came
    std::vector<int64_t> seen;
    tg.slice(0).applyOnNeighbors<int>(
        [&seen](int64_t v, const std::vector<std::pair<int64_t, int64_t>>& nb, std::vector<int>&) {
          if (v == 1)
            for (const auto& e : nb) seen.push_back(e.first);
        });
    expect(seen == std::vector<int64_t>({2, 3, 2, 9}), "Slice.arrivalOrder");

    // a NullValue stream: the count op and the neighbour lists
    EdgeStream<int64_t, NullValue> plain;
    for (const auto& r : rows) plain.edges.push_back({r[0], r[1], NullValue{}});
    const SimpleEdgeStream<int64_t, NullValue> pg(plain);
    const Sums out_degree = {{1, 2}, {2, 1}, {3, 2}, {4, 1}, {5, 1}};
    expect(pg.slice(1000).reduceOnEdges(GS_SLICE_COUNT) == out_degree, "Slice.nullValue.count");
    const auto degree =
        pg.slice(1000).foldNeighbors<int64_t>(0, [](int64_t acc, int64_t, int64_t, NullValue) { return acc + 1; });
    expect(degree == std::vector<int64_t>({2, 1, 2, 1, 1}), "Slice.nullValue.fold");
    bool threw = false;
    try {
      pg.slice(1000).reduceOnEdges(GS_SLICE_SUM);
    } catch (const GsException& e) {
      threw = e.code() == GS_ERR_INVALID;
    }
    expect(threw, "Slice.nullValue.sumIsInvalid");
  } catch (const std::exception& e) {
    std::printf("FAIL exception: %s\n", e.what());
    ++failures;
  }
  std::printf("%d failure(s)\n", failures);
  return failures ? 1 : 0;
}
