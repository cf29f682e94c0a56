// BroadcastTriangleCount (example/BroadcastTriangleCount.java:41-174) on the C++ host mirror: lines
// "src \t trg" with a vertex count and a sample count, or the reference's built-in stream -- the
// edges (k, (k + 2) % 1000) and (k, (k + 4) % 1000) for k = 0 .. 999 (:257-264) with 1000 vertices
// and 10000 samples; prints every (edge count, estimate) tuple as the reference's print() does,
// "(edges,estimate)".
// Usage: broadcast_triangle_count [<edges path> <vertex count> <sample count> [<batch>]]
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>

#include "gelly_streaming.hpp"

using namespace gelly;

int main(int argc, char** argv) {
  EdgeStream<int64_t, NullValue> s;
  size_t batch = 1 << 16;
  int vertexCount = 1000, samples = 10000;  // :216-217
  if (argc == 4 || argc == 5) {
    std::ifstream in(argv[1]);
    if (!in) {
      std::fprintf(stderr, "cannot read %s\n", argv[1]);
      return 1;
    }
    std::string line;
    while (std::getline(in, line)) {
      std::istringstream ls(line);
      int64_t a, b;
      if (ls >> a >> b) s.edges.push_back({a, b, NullValue()});
    }
    vertexCount = std::stoi(argv[2]);
    samples = std::stoi(argv[3]);
    if (argc == 5) batch = (size_t)std::stoull(argv[4]);
  } else if (argc != 1) {
    std::fprintf(stderr, "Usage: broadcast_triangle_count [<input edges path> <vertex count> <sample count> [<batch>]]\n");
    return 1;
  } else {
    for (int64_t k = 0; k < 1000; ++k) {
      s.edges.push_back({k, (k + 2) % 1000, NullValue()});
      s.edges.push_back({k, (k + 4) % 1000, NullValue()});
    }
  }
  try {
    BroadcastTriangleCount count(samples, vertexCount);
    for (const auto& r : count.run(s, batch)) std::printf("(%d,%d)\n", r.first, r.second);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
