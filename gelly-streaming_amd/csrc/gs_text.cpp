// gs_text.cpp -- the text reader behind include/gs_ingest.h's gs_text_* section: host text in,
// chunks of device columns out, for any handle's *_fold_device. The rules of a line are in
// gs_text_seq.hpp, the parse and the two compactions in gs_ingest.hip (parse_records,
// window_bounds); this file cuts the text, stages it and keeps the held-back window.
//
// One call of gs_text_next: the chunk (already staged in pinned memory by the previous call, or
// staged now) goes to the device asynchronously; while it travels the host stages the next chunk
// into the other pinned half; the held-back records of the previous call are copied from the
// other column set to the front of this one; the chunk is parsed behind them (parse_records
// waits for the stream: the counts are host values); in window mode the bounds are taken over
// held-back and new records together and the last window is held back again.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "gs_grow.hpp"
#include "gs_ingest.h"
#include "gs_ingest.hpp"
#include "gs_internal.hpp"
#include "gs_text_seq.hpp"

using namespace gsi;

struct gs_text_s : StreamOwner {
  int sep = 0, third = 0, flags = 0;
  size_t chunk = kTextChunk;
  int64_t window = 0;  // > 0: whole windows only
  // staging and parse scratch
  HostBuf<char> h_text;  // two halves of `chunk` bytes
  DevBuf<char> d_text;   // one chunk (a call ends with the stream idle)
  DevBuf<void> d_scratch;
  gs::ParseScratch scratch;
  gs::TxtScratch x;
  // the two alternating sets of output columns, each behind its own capacity word
  struct Columns {
    uint64_t cap = 0;
    DevBuf<int64_t> src, dst, val;
    DevBuf<uint8_t> del;
    DevBuf<uint64_t> first;  // window mode
    DevBuf<int64_t> window;
  } set[2];
  // the open text
  const char* text = nullptr;
  size_t len = 0, off = 0;
  bool open = false;
  bool staged = false;  // bytes [off, staged_end) lie in half `half` of h_text
  size_t staged_end = 0;
  int half = 0;
  uint64_t calls = 0, lines = 0, records = 0;
  int64_t bad_line = -1;
  // the held-back window: rows [carry_off, carry_off + carry_n) of set[carry_set]
  int carry_set = 0;
  uint64_t carry_off = 0, carry_n = 0;
  // the windows the last gs_text_next delivered: windows [0, last_windows) of set[last_set]
  int last_set = 0;
  uint64_t last_windows = 0;
};

namespace {

constexpr const char* kWhat = "text reader";
constexpr size_t kTextMaxChunk = 1u << 30;

int grow_columns(gs_text_s* t, gs_text_s::Columns& c, uint64_t need) {
  const auto alloc_columns = [&](uint64_t n) {
    hipError_t e = alloc_each(n, c.src, c.dst);
    if (e == hipSuccess && t->third == GS_TEXT_THIRD_LONG) e = c.val.alloc(n);
    if (e == hipSuccess && t->third == GS_TEXT_THIRD_EVENT) e = c.del.alloc(n);
    if (e == hipSuccess && t->window > 0) e = alloc_each(n, c.first, c.window);
    return e;
  };
  GS_HIP(grow_group(t->stream, c.cap, need, need + need / 4, alloc_columns));
  return GS_OK;
}

// stage the chunk that starts at `off` into half h; *end = its end (0: a line longer than a chunk)
void stage(gs_text_s* t, size_t off, int h, size_t* end) {
  *end = chunk_end(t->text, t->len, off, t->chunk);
  if (*end) staged_copy(t->h_text + (size_t)h * t->chunk, t->text + off, *end - off);
}

int close_with(gs_text_s* t, int code, const std::string& msg) {
  t->open = false;
  return fail(code, msg);
}

}  // namespace

extern "C" {

int gs_text_destroy(gs_text t) { return owner_destroy(t); }

int gs_text_create(gs_text* out, int device, int sep, int third, int flags, size_t chunk_bytes) {
  if (!out) return fail(GS_ERR_INVALID, "out is null");
  *out = nullptr;
  if (!gs::txt_args_ok(sep, third, flags)) return fail(GS_ERR_INVALID, "text reader: unknown separator, third field or flag");
  if (chunk_bytes > kTextMaxChunk) return fail(GS_ERR_INVALID, "text reader: a chunk has at most 2^30 bytes");
  if (int rc = check_device_index(device)) return rc;
  return owner_create(out, device, [&](gs_text_s* t) -> int {
    t->sep = sep;
    t->third = third;
    t->flags = flags;
    t->chunk = chunk_bytes ? chunk_bytes : kTextChunk;
    size_t cub = 0;
    GS_HIP(t->h_text.alloc(2 * t->chunk, hipHostMallocDefault));
    GS_HIP(t->d_text.alloc(t->chunk));
    GS_HIP(t->d_scratch.alloc(gs::parse_scratch_bytes(t->chunk, &cub)));
    if (gs::parse_scratch_init(t->scratch, t->d_scratch, t->chunk)) return fail(GS_ERR_HIP, "text reader: parse scratch");
    return GS_OK;
  });
}

int gs_text_set_window(gs_text t, int64_t size) {
  if (int rc = check_handle(t, kWhat)) return rc;
  if (size < 0) return fail(GS_ERR_INVALID, "text reader: a window size is >= 0");
  if (size > 0 && t->third != GS_TEXT_THIRD_LONG)
    return fail(GS_ERR_INVALID, "text reader: windows need a LONG third field (the timestamp)");
  t->open = false;  // a text that was not read to its end is dropped
  t->carry_n = 0;
  t->last_windows = 0;
  DeviceGuard g(t->device);
  if ((size > 0) != (t->window > 0)) {  // the window columns come and go with the sets
    GS_HIP(hipStreamSynchronize(t->stream));
    for (auto& c : t->set) c = gs_text_s::Columns();
  }
  t->window = size;
  return GS_OK;
}

int gs_text_open(gs_text t, const char* text, size_t len) {
  if (int rc = check_handle(t, kWhat)) return rc;
  if (len && !text) return fail(GS_ERR_INVALID, "text is null");
  t->text = text;
  t->len = len;
  t->off = 0;
  t->open = true;
  t->staged = false;
  t->lines = t->records = 0;
  t->bad_line = -1;
  t->carry_n = 0;
  t->last_windows = 0;
  return GS_OK;
}

int gs_text_next(gs_text t, const int64_t** src, const int64_t** dst, const int64_t** val, const uint8_t** del,
                 size_t* n, const uint64_t** first, const int64_t** window, size_t* n_windows, int* last) {
  if (int rc = check_handle(t, kWhat)) return rc;
  if (!src || !dst || !n || !last) return fail(GS_ERR_INVALID, "null argument");
  if (!t->open) return fail(GS_ERR_INVALID, "text reader: no open text (gs_text_open)");
  DeviceGuard g(t->device);
  hipStream_t st = t->stream;
  const int b = (int)(t->calls & 1);
  gs_text_s::Columns& c = t->set[b];
  // this call's chunk, in pinned memory
  size_t clen = 0;
  if (t->off < t->len) {
    if (!t->staged) {
      t->half = 0;
      stage(t, t->off, t->half, &t->staged_end);
    }
    if (!t->staged_end) return close_with(t, GS_ERR_INVALID, "text reader: a line is longer than a chunk");
    clen = t->staged_end - t->off;
  }
  const size_t end = t->off + clen;
  const bool final = end >= t->len;
  // rows: the held-back ones, and a line has >= 2 bytes unless it is malformed
  if (int rc = grow_columns(t, c, t->carry_n + clen / 2 + 2)) return rc;
  if (clen)
    GS_HIP(hipMemcpyAsync(t->d_text, t->h_text + (size_t)t->half * t->chunk, clen, hipMemcpyHostToDevice, st));
  // host: the next chunk into the other half while this one travels
  t->staged = false;
  if (!final) {
    stage(t, end, t->half ^ 1, &t->staged_end);
    t->staged = true;
    t->half ^= 1;
  }
  const uint64_t held = t->carry_n;
  if (held) {
    const gs_text_s::Columns& p = t->set[t->carry_set];
    const auto move = [&](void* to, const void* from, size_t elem) {
      return hipMemcpyAsync(to, static_cast<const char*>(from) + t->carry_off * elem, held * elem,
                            hipMemcpyDeviceToDevice, st);
    };
    GS_HIP(move(c.src, p.src, 8));
    GS_HIP(move(c.dst, p.dst, 8));
    if (c.val) GS_HIP(move(c.val, p.val, 8));
    if (c.del) GS_HIP(move(c.del, p.del, 1));
    t->carry_n = 0;
  }
  gs::TxtResult r;
  if (gs::parse_records(st, t->d_text, clen, t->sep, t->third, t->flags, c.src + held, c.dst + held,
                        c.val ? c.val + held : nullptr, c.del ? c.del + held : nullptr, c.cap - held, t->scratch, t->x,
                        &r))
    return close_with(t, GS_ERR_HIP, "text reader: the parse failed");
  const uint64_t line0 = t->lines;
  t->lines += r.lines;
  if (r.bad_line >= 0) {
    t->bad_line = (int64_t)line0 + r.bad_line;
    return close_with(t, GS_ERR_PARSE, "malformed line " + std::to_string(t->bad_line));
  }
  if (r.lines > c.cap - held) return close_with(t, GS_ERR_HIP, "text reader: more lines than rows");
  t->records += r.records;
  uint64_t rows = held + r.records, windows = 0;
  if (t->window > 0 && rows) {
    if (gs::window_bounds(st, c.val, rows, t->window, c.first, c.window, c.cap, t->x, &windows))
      return close_with(t, GS_ERR_HIP, "text reader: the window bounds failed");
    if (!final) {  // the last window may go on in the next chunk: held back
      uint64_t at = 0;
      GS_HIP(hipMemcpyAsync(&at, c.first + (windows - 1), 8, hipMemcpyDeviceToHost, st));
      GS_HIP(hipStreamSynchronize(st));
      if (at >= rows) return close_with(t, GS_ERR_HIP, "text reader: window bounds out of range");
      t->carry_set = b;
      t->carry_off = at;
      t->carry_n = rows - at;
      rows = at;
      --windows;
    }
  }
  *src = c.src;
  *dst = c.dst;
  if (val) *val = c.val;
  if (del) *del = c.del;
  *n = rows;
  if (first) *first = t->window > 0 ? c.first.get() : nullptr;
  if (window) *window = t->window > 0 ? c.window.get() : nullptr;
  if (n_windows) *n_windows = windows;
  t->last_set = b;
  t->last_windows = windows;
  *last = final ? 1 : 0;
  t->off = end;
  ++t->calls;
  if (final) t->open = false;
  return GS_OK;
}

int gs_text_windows(gs_text t, uint64_t* first, int64_t* window, size_t cap, size_t* n) {
  if (int rc = check_handle(t, kWhat)) return rc;
  if (!n) return fail(GS_ERR_INVALID, "n is null");
  const uint64_t rows = t->last_windows;
  *n = rows;
  if (cap < rows) return truncated(cap, rows);
  if (rows == 0) return GS_OK;
  if (!first || !window) return fail(GS_ERR_INVALID, "null arrays");
  DeviceGuard g(t->device);
  const gs_text_s::Columns& c = t->set[t->last_set];
  GS_HIP(hipMemcpyAsync(first, c.first, rows * 8, hipMemcpyDeviceToHost, t->stream));
  GS_HIP(hipMemcpyAsync(window, c.window, rows * 8, hipMemcpyDeviceToHost, t->stream));
  GS_HIP(hipStreamSynchronize(t->stream));
  return GS_OK;
}

int gs_text_position(gs_text t, uint64_t* lines, uint64_t* records, int64_t* bad_line) {
  if (int rc = check_handle(t, kWhat)) return rc;
  if (lines) *lines = t->lines;
  if (records) *records = t->records;
  if (bad_line) *bad_line = t->bad_line;
  return GS_OK;
}

int gs_text_sync(gs_text t) { return owner_sync(t, kWhat); }
int gs_text_get_stream(gs_text t, void** s) { return owner_get_stream(t, kWhat, s); }
int gs_text_wait_stream(gs_text t, void* s) { return owner_wait_stream(t, kWhat, s); }

}  // extern "C"
