// DegreeDistribution (example/DegreeDistribution.java:52-193) on the C++ host mirror: lines
// "src trg +|-" (:170-182), or the example's default data (:185-191); prints every
// (degree,count) record the example emits, in order, as its print() does.
// Usage: degree_distribution [<input edges path>]
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "gelly_streaming.hpp"

using namespace gelly;

int main(int argc, char** argv) {
  EdgeStream<int64_t, NullValue> s;
  std::vector<uint8_t> deletions;
  auto event = [&](int64_t src, int64_t trg, bool addition) {
    s.edges.push_back({src, trg, NullValue{}});
    deletions.push_back(addition ? 0 : 1);
  };
  if (argc == 2) {
    std::ifstream in(argv[1]);
    if (!in) {
      std::fprintf(stderr, "cannot read %s\n", argv[1]);
      return 1;
    }
    std::string line;
    while (std::getline(in, line)) {
      std::istringstream ls(line);
      int64_t a, b;
      std::string op;
      if (ls >> a >> b >> op) event(a, b, op == "+");  // (:179: anything but "+" is a deletion)
    }
  } else if (argc != 1) {
    std::fprintf(stderr, "Usage: degree_distribution [<input edges path>]\n");
    return 1;
  } else {
    event(1, 2, true), event(2, 3, true), event(1, 4, true), event(2, 3, false), event(3, 4, true), event(1, 2, false);
  }
  try {
    SimpleEdgeStream<int64_t, NullValue> graph(s);
    for (const auto& r : graph.degreeDistributionStream(deletions)) std::printf("(%ld,%ld)\n", r.first, r.second);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
