// text_seq_sanitize.cpp -- the rules of the field-spec text ingest (csrc/gs_text_seq.hpp, the header
// the parse kernels include) walked on the host, built with -fsanitize=address,undefined by
// tests/test_text_seq.py.
//
//   text_seq_san parse FILE SEP THIRD FLAGS   the sequential parse of FILE's bytes (every buffer
//       sized exactly: a read past the text or a write past the rows is a sanitizer report);
//       prints "lines L records R bad B", then one line "src dst val del" per record slot
//       (zeros for the unwritten slot of a malformed line)
//   text_seq_san windows FILE SIZE            FILE holds int64 timestamps, one per line; prints
//       "windows W", then one line "first id" per window
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gs_text_seq.hpp"

static std::vector<uint8_t> read_file(const char* path) {
  std::vector<uint8_t> out;
  FILE* f = fopen(path, "rb");
  if (!f) {
    fprintf(stderr, "cannot open %s\n", path);
    exit(2);
  }
  uint8_t buf[4096];
  size_t k;
  while ((k = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + k);
  fclose(f);
  return out;
}

int main(int argc, char** argv) {
  if (argc == 6 && !strcmp(argv[1], "parse")) {
    const std::vector<uint8_t> text = read_file(argv[2]);
    const int sep = atoi(argv[3]), third = atoi(argv[4]), flags = atoi(argv[5]);
    if (!gs::txt_args_ok(sep, third, flags)) return 2;
    // a copy of exactly len bytes on the heap: the accessor must never read text[len]
    uint8_t* exact = text.empty() ? nullptr : new uint8_t[text.size()];
    if (exact) memcpy(exact, text.data(), text.size());
    // first pass without rows: the totals size the columns exactly
    const gs::TxtTotals t0 = gs::txt_parse_seq(exact, text.size(), sep, third, flags, nullptr, nullptr, nullptr, nullptr, 0);
    std::vector<int64_t> src(t0.records, 0), dst(t0.records, 0), val(t0.records, 0);
    std::vector<uint8_t> del(t0.records, 0);
    const gs::TxtTotals t = gs::txt_parse_seq(exact, text.size(), sep, third, flags, src.data(), dst.data(),
                                              third == gs::kTxtLong ? val.data() : nullptr,
                                              third == gs::kTxtEvent ? del.data() : nullptr, t0.records);
    if (t.lines != t0.lines || t.records != t0.records || t.bad_line != t0.bad_line) return 3;
    printf("lines %" PRIu64 " records %" PRIu64 " bad %" PRId64 "\n", t.lines, t.records, t.bad_line);
    for (uint64_t i = 0; i < t.records; ++i)
      printf("%" PRId64 " %" PRId64 " %" PRId64 " %u\n", src[i], dst[i], val[i], (unsigned)del[i]);
    delete[] exact;
    return 0;
  }
  if (argc == 4 && !strcmp(argv[1], "windows")) {
    const std::vector<uint8_t> text = read_file(argv[2]);
    const int64_t size = strtoll(argv[3], nullptr, 10);
    if (size <= 0) return 2;
    std::vector<int64_t> ts;
    const gs::TxtBytes at{text.data(), text.size()};
    for (uint64_t pos = 0; pos < text.size();) {  // one Long.parseLong per line
      uint64_t q = pos;
      int64_t v = 0;
      if (gs::txt_parse_long(at, q, gs::kTxtWhitespace, v) == gs::kTxtFieldBad) return 2;
      ts.push_back(v);
      while (pos < text.size() && text[pos] != '\n') ++pos;
      ++pos;
    }
    const uint64_t w0 = gs::txt_windows_seq(ts.data(), ts.size(), size, nullptr, nullptr, 0);
    std::vector<uint64_t> first(w0);
    std::vector<int64_t> window(w0);
    const uint64_t w = gs::txt_windows_seq(ts.data(), ts.size(), size, first.data(), window.data(), w0);
    if (w != w0) return 3;
    printf("windows %" PRIu64 "\n", w);
    for (uint64_t i = 0; i < w; ++i) printf("%" PRIu64 " %" PRId64 "\n", first[i], window[i]);
    return 0;
  }
  fprintf(stderr, "usage: %s parse FILE SEP THIRD FLAGS | windows FILE SIZE\n", argv[0]);
  return 2;
}
