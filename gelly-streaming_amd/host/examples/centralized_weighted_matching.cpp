// CentralizedWeightedMatching (example/CentralizedWeightedMatching.java:36-110) on the C++ host
// mirror: lines "src \t trg \t value" (the reference reads movielens_10k_sorted.txt), 1000000
// added to the target and the value multiplied by 10 (:48-50), or a built-in small stream; prints
// every MatchingEvent as the reference's print() does, "(ADD,(src,trg,value))".
// Usage: centralized_weighted_matching [<edges path> [<batch>]]
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>

#include "gelly_streaming.hpp"

using namespace gelly;

int main(int argc, char** argv) {
  EdgeStream<int64_t, int64_t> s;
  size_t batch = 1 << 16;
  auto map = [&](int64_t src, int64_t trg, int64_t val) {  // :45-52
    s.edges.push_back({src, trg + 1000000, (int64_t)((uint64_t)val * 10ull)});
  };
  if (argc == 2 || argc == 3) {
    std::ifstream in(argv[1]);
    if (!in) {
      std::fprintf(stderr, "cannot read %s\n", argv[1]);
      return 1;
    }
    std::string line;
    while (std::getline(in, line)) {
      std::istringstream ls(line);
      int64_t a, b, v;
      if (ls >> a >> b >> v) map(a, b, v);
    }
    if (argc == 3) batch = (size_t)std::stoull(argv[2]);
  } else if (argc != 1) {
    std::fprintf(stderr, "Usage: centralized_weighted_matching [<input edges path> [<batch>]]\n");
    return 1;
  } else {  // users 1..4 rating movies 1..4
    const int64_t def[10][3] = {{1, 1, 1}, {2, 1, 3}, {2, 2, 1}, {3, 2, 3}, {3, 3, 2},
                                {1, 3, 5}, {4, 1, 4}, {4, 4, 1}, {2, 4, 9}, {2, 1, 2}};
    for (const auto& r : def) map(r[0], r[1], r[2]);
  }
  CentralizedWeightedMatching matching;
  for (const MatchingEvent& e : matching.run(s, batch))
    std::printf("(%s,(%lld,%lld,%lld))\n", e.type == MatchingEvent::Type::ADD ? "ADD" : "REMOVE",
                (long long)e.edge.f0, (long long)e.edge.f1, (long long)e.edge.f2);
  return 0;
}
