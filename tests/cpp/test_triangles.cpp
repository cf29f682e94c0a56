// WindowTriangles and ExactTriangleCount on the C++ host mirror (gelly_streaming.hpp ->
// libgs_summary.so). The expected values are the reference's own, the same numbers as
// tests/golden/triangle_pins.json:
//   TRIANGLES_DATA, TRIANGLES_RESULT   util/ExamplesTestData.java:21-34, run by
//                                      example/test/WindowTrianglesITCase.java with 400 ms windows;
//                                      lines compared sorted (compareResultsByLinesInMemory)
//   default stream                     example/ExactTriangleCount.java:196-205; its final
//                                      counters are {-1:4, 1:2, 2:2, 3:4, 4:1, 5:1, 6:2}
// Exit status 0 when every check passes.
#include <algorithm>
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "gelly_streaming.hpp"

using namespace gelly;

static int failures = 0;

static void expect(bool ok, const std::string& name) {
  std::printf("%s %s\n", ok ? "PASS" : "FAIL", name.c_str());
  if (!ok) ++failures;
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
    std::vector<std::string> lines;
    for (const auto& w : WindowTriangles(400).run(data))
      lines.push_back("(" + std::to_string(w.first) + "," + std::to_string(w.second) + ")");
    std::sort(lines.begin(), lines.end());
    std::vector<std::string> want = {"(2,1199)", "(2,399)", "(3,799)"};
    std::sort(want.begin(), want.end());
    expect(lines == want, "WindowTrianglesITCase.test");

    EdgeStream<int64_t, NullValue> loops;
    loops.edges = {{5, 5, NullValue{}}, {7, 7, NullValue{}}};
    loops.timestamps = {10, 20};
    expect(WindowTriangles(400).run(loops).empty(), "WindowTriangles.onlySelfLoops");

    EdgeStream<int64_t, NullValue> def;
    const int64_t e[9][2] = {{1, 2}, {2, 3}, {2, 6}, {5, 6}, {1, 4}, {5, 3}, {3, 4}, {3, 6}, {1, 3}};
    for (const auto& r : e) def.edges.push_back({r[0], r[1], NullValue{}});
    const std::map<int64_t, long> final_counters = {{-1, 4}, {1, 2}, {2, 2}, {3, 4}, {4, 1}, {5, 1}, {6, 2}};
    expect(ExactTriangleCount().run(def, 9) == final_counters, "ExactTriangleCount.defaultStream");
    bool same = true;
    for (size_t batch : {size_t(1), size_t(2), size_t(9)}) same = same && ExactTriangleCount().run(def, batch) == final_counters;
    expect(same, "ExactTriangleCount.batchings");
  } catch (const std::exception& e) {
    std::printf("FAIL exception: %s\n", e.what());
    ++failures;
  }
  std::printf("%d failure(s)\n", failures);
  return failures ? 1 : 0;
}
