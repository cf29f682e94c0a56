// SlidingWindowTriangles on the C++ host mirror (gelly_streaming.hpp -> libgs_summary.so), on
// the reference's 19 pinned edges (TRIANGLES_DATA, util/ExamplesTestData.java:21-34, the rows
// of tests/golden/triangle_pins.json "triangles_data"):
//   size = slide = 400   the pinned rows of WindowTrianglesITCase (TRIANGLES_RESULT)
//   size = 800, slide = 400   per window the brute-force triangle count of the union of its
//                             two panes, computed here on the host
//   size % slide != 0    refused
// Exit status 0 when every check passes.
#include <algorithm>
#include <cstdio>
#include <set>
#include <string>
#include <vector>

#include "gelly_streaming.hpp"

using namespace gelly;

static int failures = 0;

static void expect(bool ok, const std::string& name) {
  std::printf("%s %s\n", ok ? "PASS" : "FAIL", name.c_str());
  if (!ok) ++failures;
}

// triangles of the distinct non-loop pairs among the rows whose timestamp lies in [from, to)
static long brute(const int64_t (*rows)[3], int n, int64_t from, int64_t to, bool* any) {
  std::set<std::pair<int64_t, int64_t>> g;
  std::set<int64_t> v;
  for (int i = 0; i < n; ++i) {
    if (rows[i][2] < from || rows[i][2] >= to || rows[i][0] == rows[i][1]) continue;
    g.insert({std::min(rows[i][0], rows[i][1]), std::max(rows[i][0], rows[i][1])});
    v.insert(rows[i][0]);
    v.insert(rows[i][1]);
  }
  *any = !g.empty();
  const std::vector<int64_t> ids(v.begin(), v.end());
  long t = 0;
  for (size_t a = 0; a < ids.size(); ++a)
    for (size_t b = a + 1; b < ids.size(); ++b)
      for (size_t c = b + 1; c < ids.size(); ++c)
        if (g.count({ids[a], ids[b]}) && g.count({ids[b], ids[c]}) && g.count({ids[a], ids[c]})) ++t;
  return t;
}

int main() {
  try {
    EdgeStream<int64_t, NullValue> data;
    const int64_t rows[19][3] = {{1, 2, 100},  {1, 3, 150},  {3, 2, 200},  {2, 4, 250},  {3, 4, 300},
                                 {3, 5, 350},  {4, 5, 400},  {4, 6, 450},  {6, 5, 500},  {5, 7, 550},
                                 {6, 7, 600},  {8, 6, 650},  {7, 8, 700},  {7, 9, 750},  {8, 9, 800},
                                 {10, 8, 850}, {9, 10, 900}, {9, 11, 950}, {10, 11, 1000}};
    for (const auto& r : rows) {
      data.edges.push_back({r[0], r[1], NullValue{}});
      data.timestamps.push_back(r[2]);
    }
    using Rows = std::vector<std::pair<long, int64_t>>;
    const Rows tumbling = SlidingWindowTriangles(400, 400).run(data);
    expect(tumbling == Rows{{2, 399}, {3, 799}, {2, 1199}}, "SlidingWindowTriangles.sizeEqualsSlide");
    expect(tumbling == WindowTriangles(400).run(data), "SlidingWindowTriangles.equalsWindowTriangles");

    // Flink fires the windows [-400, 400), [0, 800), [400, 1200), [800, 1600): the first is a
    // leading partial window, the last one trails the last pane
    Rows want;
    for (int64_t start = -400; start <= 800; start += 400) {
      bool any = false;
      const long t = brute(rows, 19, start, start + 800, &any);
      if (any) want.emplace_back(t, start + 800 - 1);
    }
    expect(want.size() == 4 && want.front().second == 399 && want.back().second == 1599,
           "SlidingWindowTriangles.bruteForceHasTheFourWindows");
    expect(SlidingWindowTriangles(800, 400).run(data) == want, "SlidingWindowTriangles.twoPanes");

    // panes far apart: the windows between them hold nothing and are not emitted
    EdgeStream<int64_t, NullValue> gap;
    const int64_t grow[6][3] = {{1, 2, 0}, {2, 3, 10}, {1, 3, 20}, {1, 2, 100000}, {2, 3, 100010}, {3, 1, 100700}};
    for (const auto& r : grow) {
      gap.edges.push_back({r[0], r[1], NullValue{}});
      gap.timestamps.push_back(r[2]);
    }
    Rows gwant;
    for (int64_t start = -400; start <= 100800; start += 400) {
      bool any = false;
      const long t = brute(grow, 6, start, start + 800, &any);
      if (any) gwant.emplace_back(t, start + 800 - 1);
    }
    expect(gwant.size() == 5 && SlidingWindowTriangles(800, 400).run(gap) == gwant, "SlidingWindowTriangles.gap");

    bool refused = false;
    try {
      SlidingWindowTriangles bad(1000, 400);
    } catch (const std::invalid_argument&) {
      refused = true;
    }
    expect(refused, "SlidingWindowTriangles.sizeNotAMultipleOfSlide");
  } catch (const std::exception& e) {
    std::printf("FAIL exception: %s\n", e.what());
    ++failures;
  }
  std::printf("%d failure(s)\n", failures);
  return failures ? 1 : 0;
}
