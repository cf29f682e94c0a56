// MatchingEvent and CentralizedWeightedMatching on the C++ host mirror (gelly_streaming.hpp ->
// libgs_summary.so). The three pinned streams are those of tests/golden/matching_pins.json, worked
// by hand from CentralizedWeightedMatching.java:79-106. A generated stream of 1000 edges is run at
// batch sizes 1, 7 and 1000: the events must agree with each other and with the sequential
// definition of csrc/gs_matching_seq.hpp. Exit status 0 when every check passes.
#include <cstdio>
#include <string>
#include <vector>

#include "gelly_streaming.hpp"
#include "gs_matching_seq.hpp"

using namespace gelly;

static int failures = 0;

static void expect(bool ok, const std::string& name) {
  std::printf("%s %s\n", ok ? "PASS" : "FAIL", name.c_str());
  if (!ok) ++failures;
}

using Row = std::vector<int64_t>;  // type, src, dst, val

static std::vector<Row> rows(const std::vector<MatchingEvent>& ev) {
  std::vector<Row> out;
  for (const MatchingEvent& e : ev) out.push_back({(int64_t)e.type, e.edge.f0, e.edge.f1, e.edge.f2});
  return out;
}

static EdgeStream<int64_t, int64_t> stream_of(const std::vector<Row>& edges) {
  EdgeStream<int64_t, int64_t> s;
  for (const Row& e : edges) s.edges.push_back({e[0], e[1], e[2]});
  return s;
}

static std::vector<Row> model(const EdgeStream<int64_t, int64_t>& s) {
  gs::MatchingSeq m;
  std::vector<gs::MtEvent> ev;
  for (size_t i = 0; i < s.edges.size(); ++i) m.step(s.edges[i].f0, s.edges[i].f1, s.edges[i].f2, (uint32_t)i, &ev);
  std::vector<Row> out;
  for (const gs::MtEvent& e : ev) out.push_back({(int64_t)e.type, e.src, e.dst, e.val});
  return out;
}

int main() {
  const int64_t A = GS_MATCH_ADD, R = GS_MATCH_REMOVE;
  try {
    {
      CentralizedWeightedMatching m;
      const auto ev = rows(m.run(stream_of({{0, 1, 1}, {0, 2, 3}, {0, 3, 7}, {0, 4, 14}, {0, 5, 29}})));
      const std::vector<Row> want = {{A, 0, 1, 1}, {R, 0, 1, 1}, {A, 0, 2, 3},  {R, 0, 2, 3},
                                     {A, 0, 3, 7}, {R, 0, 3, 7}, {A, 0, 5, 29}};
      expect(ev == want, "CentralizedWeightedMatching.doublingStar");
      const auto M = m.matching();
      expect(M.size() == 1 && M[0].f0 == 0 && M[0].f1 == 5 && M[0].f2 == 29 && m.weight() == 29,
             "CentralizedWeightedMatching.doublingStar.matching");
    }
    {
      CentralizedWeightedMatching m;
      const auto ev = rows(m.run(stream_of({{1, 2, 1}, {2, 3, 1}, {3, 4, 1}, {4, 5, 1}}), 2));
      const std::vector<Row> want = {{A, 1, 2, 1}, {A, 3, 4, 1}};
      expect(ev == want, "CentralizedWeightedMatching.unitPath");
    }
    {
      CentralizedWeightedMatching m;
      const auto ev = rows(m.run(stream_of({{1, 2, 5}, {3, 4, 5}, {2, 3, 21}})));
      const std::vector<Row> want = {{A, 1, 2, 5}, {A, 3, 4, 5}, {R, 1, 2, 5}, {R, 3, 4, 5}, {A, 2, 3, 21}};
      expect(ev == want, "CentralizedWeightedMatching.bridge");
      MatchingEvent e{MatchingEvent::Type::REMOVE, {1, 2, 5}};
      expect(e.geType() == MatchingEvent::Type::REMOVE && e.getEdge().getValue() == 5 &&
                 (int)MatchingEvent::Type::ADD == 0 && (int)MatchingEvent::Type::REMOVE == 1,
             "MatchingEvent.accessors");
    }
    {  // 1000 generated edges over 120 vertices, values 1..64 (an LCG, so every run is the same)
      std::vector<Row> edges;
      uint64_t x = 0x9E3779B97F4A7C15ull;
      auto next = [&]() {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        return x >> 33;
      };
      for (int i = 0; i < 1000; ++i) {
        const int64_t u = (int64_t)(next() % 120), v = (int64_t)(next() % 120) + 1000000;
        edges.push_back({u, v, (int64_t)(next() % 64) + 1});
      }
      const auto s = stream_of(edges);
      const auto want = model(s);
      std::vector<std::vector<Row>> got;
      for (size_t batch : {(size_t)1, (size_t)7, (size_t)1000}) {
        CentralizedWeightedMatching m;
        got.push_back(rows(m.run(s, batch)));
      }
      expect(got[0] == got[1] && got[1] == got[2], "CentralizedWeightedMatching.batchSizesAgree");
      expect(got[2] == want && want.size() > 100, "CentralizedWeightedMatching.generatedStream");
    }
  } catch (const std::exception& e) {
    std::printf("FAIL exception: %s\n", e.what());
    ++failures;
  }
  std::printf("%d failure(s)\n", failures);
  return failures ? 1 : 0;
}
