// SimpleEdgeStream.getDegrees / getInDegrees / getOutDegrees / numberOfVertices /
// numberOfEdges on the C++ host mirror (gelly_streaming.hpp -> libgs_summary.so), and the
// DegreeDistribution example's final state through the C ABI. The expected values are the
// reference's own, the same numbers as tests/golden/degree_pins.json:
//   sample edges       test/GraphStreamTestUtils.java:58-64
//   degree outputs     test/operations/TestGetDegrees.java:38-51, 68-74, 92-98 -- every value
//                      the continuous stream emits, {(v, i) : 1 <= i <= degree(v)}; the mirror
//                      returns the last value per key, expanded here to the pinned lines
//   DEGREES_DATA, DEGREES_RESULT, DEGREES_DATA_ZERO, DEGREES_RESULT_ZERO
//                      util/ExamplesTestData.java:36-60 -- the final distribution is the last
//                      emitted count per degree: {1:2, 2:1} and {1:1, 2:1}
// Exit status 0 when every check passes.
#include <algorithm>
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

static std::vector<std::string> expand(const std::vector<Vertex<int64_t, long>>& deg) {
  std::vector<std::string> lines;
  for (const auto& v : deg)
    for (long i = 1; i <= v.getValue(); ++i) lines.push_back(std::to_string(v.getId()) + "," + std::to_string(i));
  std::sort(lines.begin(), lines.end());
  return lines;
}

static bool ascending(const std::vector<Vertex<int64_t, long>>& deg) {
  for (size_t i = 1; i < deg.size(); ++i)
    if (!(deg[i - 1].getId() < deg[i].getId())) return false;
  return true;
}

struct Event {
  int64_t src, dst;
  uint8_t del;
};

// fold the events (all at once, or one per call) and compare the final distribution
static bool distribution_is(const std::vector<Event>& ev, bool per_edge,
                            const std::vector<std::pair<int64_t, int64_t>>& want) {
  gs_handle h = nullptr;
  gs_check(gs_create(&h, 0, GS_KIND_DEGREE, 16));
  std::vector<int64_t> s, d;
  std::vector<uint8_t> e;
  for (const Event& x : ev) s.push_back(x.src), d.push_back(x.dst), e.push_back(x.del);
  if (per_edge) {
    for (size_t i = 0; i < ev.size(); ++i) gs_check(gs_degree_fold(h, &s[i], &d[i], &e[i], 1, GS_DEGREE_ALL));
  } else {
    gs_check(gs_degree_fold(h, s.data(), d.data(), e.data(), ev.size(), GS_DEGREE_ALL));
  }
  std::vector<int64_t> deg(8), cnt(8);
  size_t n = 0;
  gs_check(gs_degree_distribution(h, deg.data(), cnt.data(), deg.size(), &n));
  bool ok = n == want.size();
  for (size_t i = 0; ok && i < n; ++i) ok = deg[i] == want[i].first && cnt[i] == want[i].second;
  gs_check(gs_destroy(h));
  return ok;
}

int main() {
  try {
    EdgeStream<int64_t, int64_t> s;
    s.edges = {{1, 2, 12}, {1, 3, 13}, {2, 3, 23}, {3, 4, 34}, {3, 5, 35}, {4, 5, 45}, {5, 1, 51}};
    SimpleEdgeStream<int64_t, int64_t> graph(s);

    const std::vector<std::string> all = {"1,1", "1,2", "1,3", "2,1", "2,2", "3,1", "3,2",
                                          "3,3", "3,4", "4,1", "4,2", "5,1", "5,2", "5,3"};
    const std::vector<std::string> in = {"1,1", "2,1", "3,1", "3,2", "4,1", "5,1", "5,2"};
    const std::vector<std::string> out = {"1,1", "1,2", "2,1", "3,1", "3,2", "4,1", "5,1"};
    const auto da = graph.getDegrees(), di = graph.getInDegrees(), dout = graph.getOutDegrees();
    expect(expand(da) == all && ascending(da), "TestGetDegrees.testGetDegrees");
    expect(expand(di) == in && ascending(di), "TestGetDegrees.testGetInDegrees");
    expect(expand(dout) == out && ascending(dout), "TestGetDegrees.testGetOutDegrees");
    expect(graph.numberOfVertices() == 5, "SimpleEdgeStream.numberOfVertices");
    expect(graph.numberOfEdges() == 7, "SimpleEdgeStream.numberOfEdges");

    SimpleEdgeStream<int64_t, int64_t> empty(EdgeStream<int64_t, int64_t>{});
    expect(empty.getDegrees().empty() && empty.numberOfVertices() == 0 && empty.numberOfEdges() == 0,
           "SimpleEdgeStream.empty");

    const std::vector<Event> data = {{1, 2, 0}, {2, 3, 0}, {1, 4, 0}, {2, 3, 1}, {3, 4, 0}, {1, 2, 1}};
    std::vector<Event> zero = data;
    zero.push_back({2, 3, 1});
    for (int per_edge = 0; per_edge < 2; ++per_edge) {
      const std::string how = per_edge ? " (one edge per call)" : "";
      expect(distribution_is(data, per_edge != 0, {{1, 2}, {2, 1}}), "DegreeDistribution.DEGREES_RESULT" + how);
      expect(distribution_is(zero, per_edge != 0, {{1, 1}, {2, 1}}), "DegreeDistribution.DEGREES_RESULT_ZERO" + how);
    }
  } catch (const std::exception& e) {
    std::printf("FAIL exception: %s\n", e.what());
    ++failures;
  }
  std::printf("%d failure(s)\n", failures);
  return failures ? 1 : 0;
}
