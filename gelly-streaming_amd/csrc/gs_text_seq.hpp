// gs_text_seq.hpp -- the rules of the text ingest with a value, event or time field
// (include/gs_ingest.h, gs_parse_records_device / gs_text_*), one line at a time. Plain functions
// of their arguments with standard headers only: the parse kernels (gs_ingest.hip) take their
// per-character paths, the comment test, the int32 range, the event byte and the window id from
// here, and a host compiler builds the whole sequential parse (txt_parse_seq, txt_windows_seq)
// as a stand-alone program under the address and UB sanitizers (tests/cpp/text_seq_sanitize.cpp).
//
// A line is the bytes between '\n's with one trailing '\r' dropped; no record after a final '\n'.
// Fields 0 and 1 follow include/gs_ingest.h word for word (Java's split + Long.parseLong): this
// header only adds what comes after them.
//   kTxtInt32    fields 0 and 1 are Integer.parseInt arguments: the same grammar, the range
//                [-2^31, 2^31 - 1]. A third LONG field stays Long.parseLong.
//   field 2      p2 = the separator that ends field 1. Field 2 EXISTS iff some byte in (p2, end)
//                is not a separator (Java's split drops trailing empty strings only). If it
//                exists it is the bytes from p2 + 1 to the next separator or the line end, and
//                may be empty: "1 2  x" has an empty field 2, "1 2 " and "1 2" have none.
//   kTxtLong     malformed if field 2 does not exist or is not a Long.parseLong argument (the
//                empty field included); later fields are ignored. Tab mode: "1\t2\t 5" is
//                malformed, the field is " 5".
//   kTxtEvent    malformed only if field 2 does not exist. The deletion byte is 0 iff field 2 is
//                the single byte '+', else 1 (fields[2].equals("+") ? addition : deletion); an
//                empty field gives a deletion.
//   kTxtComment  a line whose field 0 is exactly "%" ('%' at the line start, then a separator or
//                the line end) gives no record and is never malformed. "%foo" and " % x" are
//                malformed. Comment lines count as lines (line indices, n_lines), not as records.
//   windows      record i with timestamp ts and size S > 0 has window id ts / S, C++ truncating
//                division: the rule of SummaryBulkAggregation::window_of in the host mirror.
//                Flink's TimeWindow start is ts - ((ts % S + S) % S), the FLOOR: for negative
//                timestamps that are no multiple of S Flink's window lies one below this one. A
//                window is a maximal run of consecutive records with equal id; nothing is sorted
//                or checked for ascent.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GS_TXT_HD __host__ __device__ inline
#else
#define GS_TXT_HD inline
#endif

namespace gs {

// the values of include/gs_ingest.h
enum TxtSep : int { kTxtWhitespace = 0, kTxtTab = 1 };
enum TxtThird : int { kTxtNone = 0, kTxtLong = 1, kTxtEvent = 2 };
enum TxtFlags : int { kTxtInt32 = 1, kTxtComment = 2 };
// what a line gives
enum TxtVerdict : int { kTxtBad = 0, kTxtRecord = 1, kTxtSkip = 2 };
// how a field ended
enum TxtFieldEnd : int { kTxtFieldBad = 0, kTxtFieldSep = 1, kTxtFieldEol = 2 };

// one kernel instantiation per (third, flags): the template parameter of the parse
GS_TXT_HD constexpr int txt_mode(int third, int flags) { return third | (flags << 2); }
GS_TXT_HD constexpr int txt_mode_third(int mode) { return mode & 3; }
GS_TXT_HD constexpr bool txt_mode_int32(int mode) { return ((mode >> 2) & kTxtInt32) != 0; }
GS_TXT_HD constexpr bool txt_mode_comment(int mode) { return ((mode >> 2) & kTxtComment) != 0; }
GS_TXT_HD bool txt_args_ok(int sep, int third, int flags) {
  return (sep == kTxtWhitespace || sep == kTxtTab) && third >= kTxtNone && third <= kTxtEvent &&
         (flags & ~(kTxtInt32 | kTxtComment)) == 0;
}

// Java regex \s = [ \t\n\x0B\f\r]; \t = tab only
GS_TXT_HD bool txt_is_sep(uint8_t c, int sep) {
  return sep == kTxtTab ? c == '\t' : (c == ' ' || (c >= '\t' && c <= '\r'));
}
GS_TXT_HD bool txt_int32_ok(int64_t v) { return v >= -2147483648ll && v <= 2147483647ll; }
GS_TXT_HD int64_t txt_window_of(int64_t ts, int64_t size) { return ts / size; }

// `at(q)` is byte q of the text, and '\n' at or past its end (the last line needs no terminator).
// The line that holds q ends at q: at '\n', or at a '\r' right before one.
template <class At>
GS_TXT_HD bool txt_line_ends(const At& at, uint64_t q) {
  const uint8_t c = at(q);
  return c == '\n' || (c == '\r' && at(q + 1) == '\n');
}

// the line that starts at q is a comment: "%" alone, or '%' and a separator
template <class At>
GS_TXT_HD bool txt_is_comment(const At& at, uint64_t q, int sep) {
  return at(q) == '%' && (txt_line_ends(at, q + 1) || txt_is_sep(at(q + 1), sep));
}

// Long.parseLong on the field starting at q (the grammar of include/gs_ingest.h): optional sign,
// >= 1 ASCII digit, the int64 range, ended by a separator or the line end. q moves to the byte
// that ended it.
template <class At>
GS_TXT_HD int txt_parse_long(const At& at, uint64_t& q, int sep, int64_t& out) {
  uint8_t c = at(q);
  const bool neg = c == '-';
  if (neg || c == '+') c = at(++q);
  const uint64_t cut = 922337203685477580ull;  // (2^63 - 1) / 10
  const uint32_t last_ok = neg ? 8u : 7u;
  uint64_t m = 0;
  int digits = 0;
  uint32_t d = (uint32_t)c - '0';
  while (d <= 9u) {
    if (m >= cut && (m > cut || d > last_ok)) return kTxtFieldBad;
    m = m * 10 + d;
    ++digits;
    c = at(++q);
    d = (uint32_t)c - '0';
  }
  if (digits == 0) return kTxtFieldBad;
  out = neg ? (int64_t)(0ull - m) : (int64_t)m;
  if (txt_line_ends(at, q)) return kTxtFieldEol;
  return txt_is_sep(c, sep) ? kTxtFieldSep : kTxtFieldBad;
}

// The event field of a line whose field 1 ended at the separator q - 1: false if field 2 does not
// exist; else *del = 0 for the single byte '+', 1 for anything else (the empty field included).
template <class At>
GS_TXT_HD bool txt_event_field(const At& at, uint64_t q, int sep, uint8_t* del) {
  if (txt_line_ends(at, q)) return false;
  const uint8_t c = at(q);
  if (!txt_is_sep(c, sep)) {
    *del = (c == '+' && (txt_line_ends(at, q + 1) || txt_is_sep(at(q + 1), sep))) ? 0 : 1;
    return true;
  }
  *del = 1;  // an empty field 2, if anything but separators follows
  for (++q; !txt_line_ends(at, q); ++q)
    if (!txt_is_sep(at(q), sep)) return true;
  return false;
}

struct TxtRecord {
  int64_t src = 0, dst = 0, val = 0;  // val: the LONG field
  uint8_t del = 0;                    // the EVENT byte
};

// The line that starts at q, whole.
template <class At>
GS_TXT_HD int txt_parse_line(const At& at, uint64_t q, int sep, int third, int flags, TxtRecord* r) {
  if ((flags & kTxtComment) && txt_is_comment(at, q, sep)) return kTxtSkip;
  // two fields: the first must end at a separator (else fields[1] does not exist)
  if (txt_parse_long(at, q, sep, r->src) != kTxtFieldSep) return kTxtBad;
  ++q;
  const int e1 = txt_parse_long(at, q, sep, r->dst);
  if (e1 == kTxtFieldBad) return kTxtBad;
  if ((flags & kTxtInt32) && !(txt_int32_ok(r->src) && txt_int32_ok(r->dst))) return kTxtBad;
  if (third == kTxtNone) return kTxtRecord;
  if (e1 != kTxtFieldSep) return kTxtBad;  // no separator after field 1: no field 2
  ++q;
  if (third == kTxtLong) return txt_parse_long(at, q, sep, r->val) != kTxtFieldBad ? kTxtRecord : kTxtBad;
  return txt_event_field(at, q, sep, &r->del) ? kTxtRecord : kTxtBad;
}

// ---- the sequential parse of a whole text (host walk; the kernels number lines the same way)
struct TxtBytes {
  const uint8_t* text;
  uint64_t len;
  GS_TXT_HD uint8_t operator()(uint64_t q) const { return q < len ? text[q] : (uint8_t)'\n'; }
};

struct TxtTotals {
  uint64_t lines = 0, records = 0;
  int64_t bad_line = -1;  // the first malformed line (lines are numbered with the comment lines)
};

// Records in order into src/dst/val/del (val, del may be null), at most cap of them. A malformed
// line keeps its record slot (unwritten), as a malformed line of gs_parse_edges_device keeps its
// row; a comment line has none.
inline TxtTotals txt_parse_seq(const uint8_t* text, uint64_t len, int sep, int third, int flags, int64_t* src,
                               int64_t* dst, int64_t* val, uint8_t* del, uint64_t cap) {
  TxtTotals t;
  const TxtBytes at{text, len};
  uint64_t pos = 0;
  while (pos < len) {
    TxtRecord r;
    const int v = txt_parse_line(at, pos, sep, third, flags, &r);
    if (v == kTxtBad && t.bad_line < 0) t.bad_line = (int64_t)t.lines;
    if (v == kTxtRecord && t.records < cap) {
      src[t.records] = r.src;
      dst[t.records] = r.dst;
      if (val) val[t.records] = r.val;
      if (del) del[t.records] = r.del;
    }
    if (v != kTxtSkip) ++t.records;
    ++t.lines;
    while (pos < len && text[pos] != '\n') ++pos;
    ++pos;  // past the '\n' (a final '\n' yields no further line)
  }
  return t;
}

// ---- windows: record i opens one when it is the first or its id differs from record i - 1's
GS_TXT_HD bool txt_window_opens(const int64_t* ts, uint64_t i, int64_t size) {
  return i == 0 || txt_window_of(ts[i], size) != txt_window_of(ts[i - 1], size);
}
// first[w] = the first record of window w, window[w] = its id (at most cap written); returns the count
inline uint64_t txt_windows_seq(const int64_t* ts, uint64_t n, int64_t size, uint64_t* first, int64_t* window,
                                uint64_t cap) {
  uint64_t w = 0;
  for (uint64_t i = 0; i < n; ++i) {
    if (!txt_window_opens(ts, i, size)) continue;
    if (w < cap) {
      first[w] = i;
      window[w] = txt_window_of(ts[i], size);
    }
    ++w;
  }
  return w;
}

// ---- tiles of the two compactions (comment rows, window bounds): kTxtTile consecutive rows per
// workgroup, kTxtPer consecutive rows per thread
constexpr uint32_t kTxtBS = 256, kTxtPer = 4, kTxtTile = kTxtBS * kTxtPer;
constexpr uint64_t kTxtMaxRows = 0xFFFFFFFEull;  // the tile scan carries 32-bit counts
GS_TXT_HD uint64_t txt_tiles(uint64_t n) { return (n + kTxtTile - 1) / kTxtTile; }
GS_TXT_HD uint64_t txt_row_first(uint64_t tile, uint32_t thread) { return tile * kTxtTile + (uint64_t)thread * kTxtPer; }

}  // namespace gs
