// ExactTriangleCount::stream on the C++ host mirror (gelly_streaming.hpp -> libgs_summary.so).
// The expected sequence is the `derived` section of tests/golden/tristream_pins.json: worked out
// by hand from ExactTriangleCount.java:74-134 over the example's built-in stream (:196-205),
// (-1, total) after each closing arrival's records.
// Exit status 0 when every check passes.
#include <cstdio>
#include <map>
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

typedef std::vector<std::pair<int64_t, long>> Tuples;

int main() {
  try {
    EdgeStream<int64_t, NullValue> s;
    const int64_t e[9][2] = {{1, 2}, {2, 3}, {2, 6}, {5, 6}, {1, 4}, {5, 3}, {3, 4}, {3, 6}, {1, 3}};
    for (const auto& p : e) s.edges.push_back({p[0], p[1], NullValue{}});
    const Tuples want = {{2, 1}, {5, 1}, {3, 2}, {6, 2}, {-1, 2}, {2, 2}, {4, 1}, {1, 2}, {3, 4}, {-1, 4}};
    ExactTriangleCount etc;
    const Tuples whole = etc.stream(s);
    expect(whole == want, "ExactTriangleCount.stream built-in stream");
    expect(etc.stream(s, 1) == want && etc.stream(s, s.edges.size()) == want && etc.stream(s, 4) == want,
           "ExactTriangleCount.stream batch 1, 4 and n");
    std::map<int64_t, long> last;
    for (const auto& t : whole) last[t.first] = t.second;
    expect(last == etc.run(s, 0) && last == etc.run(s, 2), "ExactTriangleCount.stream last values == run");
    // a repeated edge is counted again, as the reference does; a loop emits nothing
    s.edges.push_back({3, 1, NullValue{}});
    s.edges.push_back({4, 4, NullValue{}});
    Tuples more = want;
    const Tuples extra = {{2, 3}, {4, 2}, {1, 4}, {3, 6}, {-1, 6}};
    more.insert(more.end(), extra.begin(), extra.end());
    expect(etc.stream(s, 3) == more, "ExactTriangleCount.stream repeated edge and loop");
    EdgeStream<int64_t, NullValue> none;
    expect(etc.stream(none).empty(), "ExactTriangleCount.stream empty stream");
  } catch (const std::exception& ex) {
    std::printf("FAIL exception: %s\n", ex.what());
    ++failures;
  }
  std::printf("%d failure(s)\n", failures);
  return failures ? 1 : 0;
}
