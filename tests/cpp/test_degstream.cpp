// SimpleEdgeStream.getDegreeStream / degreeDistributionStream / numberOfVerticesStream /
// numberOfEdgesStream on the C++ host mirror (gelly_streaming.hpp -> libgs_summary.so). The
// expected values are the reference's own, the same numbers as tests/golden/degree_pins.json:
//   sample edges       test/GraphStreamTestUtils.java:58-64
//   degree outputs     test/operations/TestGetDegrees.java:38-51, 68-74, 92-98 -- every value the
//                      continuous stream emits
//   DEGREES_DATA, DEGREES_RESULT, DEGREES_DATA_ZERO, DEGREES_RESULT_ZERO
//                      util/ExamplesTestData.java:36-60 -- every (degree,count), in order
//   counts             test/operations/TestNumberOfEntities.java:40-71 -- 1..5 and 1..7
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

static std::vector<std::string> lines_of(const std::vector<Vertex<int64_t, long>>& rows) {
  std::vector<std::string> lines;
  for (const auto& v : rows) lines.push_back(std::to_string(v.getId()) + "," + std::to_string(v.getValue()));
  std::sort(lines.begin(), lines.end());
  return lines;
}

static std::vector<long> upto(long n) {
  std::vector<long> v;
  for (long i = 1; i <= n; ++i) v.push_back(i);
  return v;
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
    expect(lines_of(graph.getDegreeStream()) == all, "TestGetDegrees.testGetDegrees stream");
    expect(lines_of(graph.getDegreeStream(EdgeDirection::IN)) == in, "TestGetDegrees.testGetInDegrees stream");
    expect(lines_of(graph.getDegreeStream(EdgeDirection::OUT)) == out, "TestGetDegrees.testGetOutDegrees stream");
    // arrival order: the first rows are edge (1, 2)'s endpoints, then edge (1, 3)'s
    const auto rows = graph.getDegreeStream();
    expect(rows.size() == 14 && rows[0].getId() == 1 && rows[1].getId() == 2 && rows[2].getId() == 1 &&
               rows[2].getValue() == 2 && rows[3].getId() == 3,
           "getDegreeStream arrival order");
    expect(graph.numberOfVerticesStream() == upto(5), "TestNumberOfEntities.testNumberOfVertices stream");
    expect(graph.numberOfEdgesStream() == upto(7), "TestNumberOfEntities.testNumberOfEdges stream");
    // the existing members keep their meaning
    expect(graph.numberOfVertices() == 5 && graph.numberOfEdges() == 7 && graph.getDegrees().size() == 5,
           "SimpleEdgeStream last values");

    SimpleEdgeStream<int64_t, int64_t> empty(EdgeStream<int64_t, int64_t>{});
    expect(empty.getDegreeStream().empty() && empty.degreeDistributionStream().empty() &&
               empty.numberOfVerticesStream().empty() && empty.numberOfEdgesStream().empty(),
           "SimpleEdgeStream.empty streams");

    EdgeStream<int64_t, int64_t> d;
    d.edges = {{1, 2, 0}, {2, 3, 0}, {1, 4, 0}, {2, 3, 0}, {3, 4, 0}, {1, 2, 0}};
    std::vector<uint8_t> del = {0, 0, 0, 1, 0, 1};
    std::vector<std::pair<long, long>> want = {{1, 1}, {1, 2}, {2, 1}, {1, 1}, {1, 2}, {2, 2}, {1, 1}, {1, 2}, {1, 3},
                                               {2, 1}, {1, 2}, {1, 3}, {2, 2}, {1, 2}, {1, 3}, {2, 1}, {1, 2}};
    expect(SimpleEdgeStream<int64_t, int64_t>(d).degreeDistributionStream(del) == want,
           "DegreeDistribution.DEGREES_RESULT stream");
    d.edges.push_back({2, 3, 0});
    del.push_back(1);
    want.push_back({1, 1});
    expect(SimpleEdgeStream<int64_t, int64_t>(d).degreeDistributionStream(del) == want,
           "DegreeDistribution.DEGREES_RESULT_ZERO stream");
    bool threw = false;
    try {
      SimpleEdgeStream<int64_t, int64_t>(d).degreeDistributionStream({1});
    } catch (const GsException& e) {
      threw = e.code() == GS_ERR_INVALID;
    }
    expect(threw, "degreeDistributionStream deletion count");
  } catch (const std::exception& e) {
    std::printf("FAIL exception: %s\n", e.what());
    ++failures;
  }
  std::printf("%d failure(s)\n", failures);
  return failures ? 1 : 0;
}
