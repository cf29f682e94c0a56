// SpannerExample (example/SpannerExample.java:49-166) on the C++ host mirror: the built-in
// default stream of 12 edges with k = 3, or a whitespace-separated edge file; for every Merger
// emission prints the spanner's edges, one "(src,trg)" line each with src <= trg, ascending
// (the reference flattens the adjacency sets into such pairs, in hash order).
// Usage: spanner_example [<edges path> <merge window ms> <k>]
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>

#include "gelly_streaming.hpp"

using namespace gelly;

int main(int argc, char** argv) {
  int64_t mergeWindowTime = 1000;  // :78
  int k = 3;                       // :80
  EdgeStream<int64_t, NullValue> s;
  if (argc == 4) {
    std::ifstream in(argv[1]);
    std::string line;
    while (std::getline(in, line)) {  // :111-119, split on whitespace
      std::istringstream ls(line);
      int64_t a, b;
      if (ls >> a >> b) s.edges.push_back({a, b, NullValue{}});
    }
    mergeWindowTime = std::stoll(argv[2]);
    k = std::stoi(argv[3]);
  } else if (argc != 1) {
    std::fprintf(stderr, "Usage: spanner_example <input edges path> <merge window time (ms)> <distance factor>\n");
    return 1;
  } else {  // :123-135
    const int64_t def[12][2] = {{1, 4}, {4, 7}, {7, 8}, {4, 8}, {4, 5}, {5, 6},
                                {2, 3}, {3, 4}, {3, 6}, {8, 9}, {6, 8}, {5, 9}};
    for (const auto& r : def) s.edges.push_back({r[0], r[1], NullValue{}});
  }
  SimpleEdgeStream<int64_t, NullValue> edges(s);
  Spanner<NullValue> spanner(mergeWindowTime, k);
  edges.aggregate(spanner, [](const AdjacencyListGraphRef& g) {
    for (const auto& e : g->edges()) std::printf("(%lld,%lld)\n", (long long)e.first, (long long)e.second);
  });
  return 0;
}
