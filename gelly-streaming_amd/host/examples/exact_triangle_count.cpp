// ExactTriangleCount (example/ExactTriangleCount.java:44-66) on the C++ host mirror: lines
// "src trg", lines that start with "%" skipped (:185-192), or the example's built-in stream
// (:196-205); prints every (vertex,count) tuple the example emits, in order, as its print()
// does; key -1 is the total.
// Usage: exact_triangle_count [<input edges path>]
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>

#include "gelly_streaming.hpp"

using namespace gelly;

int main(int argc, char** argv) {
  EdgeStream<int64_t, NullValue> s;
  if (argc == 2) {
    std::ifstream in(argv[1]);
    if (!in) {
      std::fprintf(stderr, "cannot read %s\n", argv[1]);
      return 1;
    }
    std::string line;
    while (std::getline(in, line)) {
      if (!line.empty() && line[0] == '%') continue;
      std::istringstream ls(line);
      int64_t a, b;
      if (ls >> a >> b) s.edges.push_back({a, b, NullValue{}});
    }
  } else if (argc != 1) {
    std::fprintf(stderr, "Usage: exact_triangle_count [<input edges path>]\n");
    return 1;
  } else {
    const int64_t e[9][2] = {{1, 2}, {2, 3}, {2, 6}, {5, 6}, {1, 4}, {5, 3}, {3, 4}, {3, 6}, {1, 3}};
    for (const auto& p : e) s.edges.push_back({p[0], p[1], NullValue{}});
  }
  try {
    for (const auto& t : ExactTriangleCount().stream(s)) std::printf("(%ld,%ld)\n", (long)t.first, t.second);
  } catch (const std::exception& ex) {
    std::fprintf(stderr, "%s\n", ex.what());
    return 1;
  }
  return 0;
}
