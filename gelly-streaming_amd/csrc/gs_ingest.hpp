// gs_ingest.hpp -- internal interface of the GPU text parser (gs_ingest.hip),
// used by gs_parse_edges_device / gs_parse_records_device, by gs_fold_text (gs_capi.cpp) and by
// the text reader (gs_text.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gs_devbuf.hpp"
#include "gs_testing.h"

namespace gsi {
int64_t testing_value(int knob, int64_t product);  // include/gs_testing.h (gs_capi.cpp)
}

namespace gs {

struct ParseScratch {
  uint64_t* tile_cnt = nullptr;  // '\n' per 4 KiB tile
  uint64_t* tile_pre = nullptr;  // exclusive scan of tile_cnt
  unsigned long long* bad = nullptr;  // min malformed line index
  uint64_t* res = nullptr;            // [2] {line count, first malformed line or ~0}
  void* cub_tmp = nullptr;
  size_t cub_bytes = 0;
  uint64_t tiles_cap = 0;
  bool bad_ready = false;  // `bad` holds ~0 (k_parse_result resets it after every parse)
  bool st_zero = false;    // the one-pass status words are zero (the last one-pass parse's k_parse_finish cleared them)
  hipStream_t zero_stream = nullptr;  // the stream that k_parse_finish ran on (st_zero holds only there)
};

// The columns of the field-spec parse (gs_text_seq.hpp, mode != 0) beside src and dst: the LONG
// values or the EVENT bytes of the third field, and, for a mode with comment lines, a skip byte
// per line (the compaction's flags). The comment lines are counted into ParseScratch::res[2].
struct TxtCols {
  int64_t* val = nullptr;
  uint8_t* del = nullptr;
  uint8_t* skip = nullptr;
  unsigned long long* nskip = nullptr;  // (set by parse_text_enqueue)
};

// Device bytes needed to parse up to max_len bytes of text.
size_t parse_scratch_bytes(size_t max_len, size_t* cub_bytes);
int parse_scratch_init(ParseScratch& s, void* mem, size_t max_len);
// Enqueue the parse of device text on st; the result {lines, bad or ~0} lands in s.res
// (device) and, with host_res (mapped), in host_res[1..2] behind host_res[0] = seq.
// fused: one pass (k_parse_fused, decoupled look-back) instead of count + scan + parse.
// Returns 0 or -1 (HIP failure).
int parse_text_enqueue(hipStream_t st, const char* text, size_t len, int sep, int64_t* src, int64_t* dst, size_t cap,
                       ParseScratch& s,
                       unsigned long long* host_res = nullptr, unsigned long long seq = 0, bool fused = true,
                       hipEvent_t kev0 = nullptr, hipEvent_t kev1 = nullptr,  // optional: bracket the parse kernel
                       int mode = 0, const TxtCols* cols = nullptr);  // mode != 0 (one pass only): the field-spec parse
// The rows of the lines whose skip byte is 0, in order, into the o columns (at most cap rows;
// val / del may be null); *total (device) = their number. tb: txt_tiles(n) + 1 words.
void launch_txt_compact(const uint8_t* skip, uint64_t n, uint32_t* tb, unsigned long long* total, const int64_t* src,
                        const int64_t* dst, const int64_t* val, const uint8_t* del, int64_t* osrc, int64_t* odst,
                        int64_t* oval, uint8_t* odel, uint64_t cap, hipStream_t st);
// first[w] / window[w] = the first record and the id of window w of ts[0 .. n) (at most cap
// written); *total (device) = the number of windows. tb: txt_tiles(n) + 1 words.
void launch_txt_windows(const int64_t* ts, uint64_t n, int64_t size, uint32_t* tb, unsigned long long* total,
                        uint64_t* first, int64_t* window, uint64_t cap, hipStream_t st);
// Scratch of a field-spec parse and of the window bounds, grown on demand (grow_group): the skip
// bytes of `lines` lines; the tile counts and the columns the comment compaction writes before
// they are copied back, for `rows` rows; the device count word of either compaction.
struct TxtScratch {
  uint64_t lines = 0, tile_rows = 0, rows = 0;  // what skip, tb and the columns hold
  gsi::DevBuf<uint8_t> skip;
  gsi::DevBuf<uint32_t> tb;
  gsi::DevBuf<int64_t> src, dst, val;
  gsi::DevBuf<uint8_t> del;
  gsi::DevBuf<unsigned long long> total;
  uint64_t compactions = 0;  // comment compactions run (tests: none without a comment line)
};
struct TxtResult {
  uint64_t lines = 0, records = 0;
  int64_t bad_line = -1;
};
// Device text -> device columns under (sep, third, flags), comment rows compacted away; line i
// is written while i < cap. Synchronises st. Returns 0 or -1 (HIP failure, or more than
// kTxtMaxRows lines to compact).
int parse_records(hipStream_t st, const char* text, size_t len, int sep, int third, int flags, int64_t* src,
                  int64_t* dst, int64_t* val, uint8_t* del, size_t cap, ParseScratch& s, TxtScratch& x, TxtResult* out,
                  hipEvent_t kev0 = nullptr, hipEvent_t kev1 = nullptr);
// The window bounds of ts[0 .. n), n <= kTxtMaxRows; synchronises st. Returns 0 or -1.
int window_bounds(hipStream_t st, const int64_t* ts, size_t n, int64_t size, uint64_t* first, int64_t* window,
                  size_t cap, TxtScratch& x, uint64_t* n_windows);

// Parse device text; synchronises st. Returns 0 or -1 (HIP failure).
int parse_text(hipStream_t st, const char* text, size_t len, int sep, int64_t* src, int64_t* dst, size_t cap,
               ParseScratch& s, uint64_t* n_lines, int64_t* bad_line);

}  // namespace gs
