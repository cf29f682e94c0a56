// The text reader and WindowTriangles::runText on the C++ host mirror (gelly_streaming.hpp ->
// libgs_summary.so): the reference's TRIANGLES_DATA (util/ExamplesTestData.java:21-31, the numbers
// of tests/golden/triangle_pins.json) written as the "src trg timestamp" lines its driver reads
// (example/WindowTriangles.java:178-186), against TRIANGLES_RESULT (:33-34, 400 ms windows; lines
// compared sorted as compareResultsByLinesInMemory does) and against run() on the same stream.
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

static std::vector<std::string> sorted_lines(const std::vector<std::pair<long, int64_t>>& rows) {
  std::vector<std::string> lines;
  for (const auto& w : rows) lines.push_back("(" + std::to_string(w.first) + "," + std::to_string(w.second) + ")");
  std::sort(lines.begin(), lines.end());
  return lines;
}

int main() {
  try {
    const int64_t rows[19][3] = {{1, 2, 100},  {1, 3, 150},  {3, 2, 200},  {2, 4, 250},  {3, 4, 300},
                                 {3, 5, 350},  {4, 5, 400},  {4, 6, 450},  {6, 5, 500},  {5, 7, 550},
                                 {6, 7, 600},  {8, 6, 650},  {7, 8, 700},  {7, 9, 750},  {8, 9, 800},
                                 {10, 8, 850}, {9, 10, 900}, {9, 11, 950}, {10, 11, 1000}};
    EdgeStream<int64_t, NullValue> data;
    std::string text, tsv;
    for (const auto& r : rows) {
      data.edges.push_back({r[0], r[1], NullValue{}});
      data.timestamps.push_back(r[2]);
      text += std::to_string(r[0]) + " " + std::to_string(r[1]) + " " + std::to_string(r[2]) + "\n";
      tsv += std::to_string(r[0]) + "\t" + std::to_string(r[1]) + "\t" + std::to_string(r[2]) + "\r\n";
    }
    const std::vector<std::string> want = {"(2,1199)", "(2,399)", "(3,799)"};
    expect(sorted_lines(WindowTriangles(400).runText(text.data(), text.size())) == want, "WindowTriangles.runText");
    expect(WindowTriangles(400).runText(text.data(), text.size()) == WindowTriangles(400).run(data),
           "WindowTriangles.runText equals run");
    expect(sorted_lines(WindowTriangles(400).runText(tsv.data(), tsv.size(), GS_SEP_TAB)) == want,
           "WindowTriangles.runText tab and CRLF");
    // chunks of 64 bytes: every window spans chunks, held back and prepended on the device
    expect(sorted_lines(WindowTriangles(400).runText(text.data(), text.size(), GS_SEP_WHITESPACE, 64)) == want,
           "WindowTriangles.runText small chunks");
    expect(WindowTriangles(400).runText("", 0).empty(), "WindowTriangles.runText empty");
    bool threw = false;
    try {
      const std::string bad = text + "1 2\n";
      WindowTriangles(400).runText(bad.data(), bad.size());
    } catch (const std::exception&) {
      threw = true;
    }
    expect(threw, "WindowTriangles.runText malformed line throws");

    // the reader alone: "src trg +|-" events (DegreeDistribution.java:170-182)
    const std::string ev = "1 2 +\n2 3 +\n% note\n2 3 -\n";
    TextReader reader(0, GS_SEP_WHITESPACE, GS_TEXT_THIRD_EVENT, GS_TEXT_INT32 | GS_TEXT_COMMENT_PERCENT);
    reader.open(ev.data(), ev.size());
    TextReader::Chunk c;
    size_t records = 0, chunks = 0;
    while (reader.next(&c)) {
      records += c.n;
      ++chunks;
    }
    uint64_t lines = 0, recs = 0;
    int64_t bad_line = 0;
    gs_check(gs_text_position(reader.handle(), &lines, &recs, &bad_line));
    expect(chunks == 1 && records == 3 && lines == 4 && recs == 3 && bad_line == -1 && !reader.next(&c),
           "TextReader.events and comments");
  } catch (const std::exception& e) {
    std::printf("FAIL exception: %s\n", e.what());
    ++failures;
  }
  std::printf("%d failure(s)\n", failures);
  return failures ? 1 : 0;
}
