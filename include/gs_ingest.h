/*
 * gs_ingest.h -- text edge-file ingest on the GPU.
 *
 * Replaces the reference's per-record source map
 *     String[] fields = s.split("\\s");          (or "\\t")
 *     long src = Long.parseLong(fields[0]);
 *     long trg = Long.parseLong(fields[1]);
 * of ConnectedComponentsExample.java:109-118 (whitespace; also SpannerExample,
 * DegreeDistribution, WindowTriangles) and BipartitenessCheckExample.java:97-106
 * (tab), applied to the lines of env.readTextFile: '\n'-delimited, a trailing
 * '\r' dropped, no record after a final '\n'.
 *
 * A line is MALFORMED exactly when that map would throw: fewer than two fields,
 * an empty field 0 or 1 (leading or doubled separator), a field that is not an
 * optionally signed run of decimal digits, or a value outside the int64 range.
 * Fields after the second are ignored (as the reference ignores fields[2..]).
 * Deviation: Java's Long.parseLong also accepts non-ASCII Unicode decimal digits;
 * the byte parser accepts ASCII '0'-'9' only.
 */
#ifndef GS_INGEST_H
#define GS_INGEST_H

#include <stddef.h>
#include <stdint.h>

#include "gs_summary.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
  GS_SEP_WHITESPACE = 0, /* split("\\s"): any of ' ' '\t' '\n' '\x0B' '\f' '\r' */
  GS_SEP_TAB = 1         /* split("\\t") */
};

#define GS_ERR_PARSE (-5)

/* Parse `len` bytes of DEVICE text (on the current HIP device) into DEVICE arrays:
 * line i -> src[i], dst[i] for i < cap. *n_lines (HOST) = number of lines; *bad_line
 * (HOST) = 0-based index of the first malformed line, or -1. Returns GS_OK,
 * GS_ERR_PARSE (a malformed line; the other lines are still written) or
 * GS_ERR_TRUNCATED (more lines than cap). Work is queued on `stream`
 * (hipStream_t, NULL = default) and the call synchronises it. */
int gs_parse_edges_device(void* stream, const char* text, size_t len, int sep, int64_t* src, int64_t* dst,
                          size_t cap, uint64_t* n_lines, int64_t* bad_line);

/* HOST text (e.g. a memory-mapped edge file) -> fold: copied through pinned staging
 * in chunks that end at line boundaries, parsed on the device and folded into h
 * (gs_fold semantics, one fold per chunk). *n_edges = edges folded. On a malformed
 * line returns GS_ERR_PARSE with *bad_line = its 0-based line index; the chunks
 * before it have been folded (the reference's job would have processed those
 * records before its map threw). */
int gs_fold_text(gs_handle h, const char* text, size_t len, int sep, uint64_t* n_edges, int64_t* bad_line);

/*
 * ---- Records with a third field, int32 endpoints and comment lines --------------------------
 *
 * The reference's other drivers read more than two fields: "src trg +|-" (DegreeDistribution.java:
 * 170-182, fields[2].equals("+") ? addition : deletion), "src trg timestamp" (WindowTriangles.java:
 * 178-186, Long.parseLong x 3), "src\ttrg\tweight" (CentralizedWeightedMatching.java:44-52) and
 * "src trg" with '%' comment lines and Integer.parseInt (ExactTriangleCount.java:182-190). The
 * rules, one line at a time (csrc/gs_text_seq.hpp states them as code, and the kernels and a
 * sanitizer-built host program both include it):
 *
 *  - Fields 0 and 1 are as above. With GS_TEXT_INT32 they are Integer.parseInt arguments: the
 *    same grammar, the range [-2^31, 2^31 - 1]. A third LONG field stays Long.parseLong.
 *  - Let p2 be the separator that ends field 1. Field 2 EXISTS iff some byte in (p2, end) is not
 *    a separator (Java's split drops trailing empty strings only). If it exists it is the bytes
 *    from p2 + 1 to the next separator or the line end, and may be empty: "1 2  x" has an empty
 *    field 2; "1 2 " and "1 2" have none.
 *  - GS_TEXT_THIRD_LONG: malformed if field 2 does not exist or is not a Long.parseLong argument
 *    (empty included). Later fields are ignored. Tab mode: "1\t2\t 5" is malformed (" 5").
 *  - GS_TEXT_THIRD_EVENT: malformed only if field 2 does not exist. The deletion byte is 0 iff
 *    field 2 is the single byte '+', else 1; an empty field gives a deletion.
 *  - GS_TEXT_COMMENT_PERCENT: a line whose field 0 is exactly "%" ('%' at the line start, then a
 *    separator or the line end) gives no record and is never malformed; "%foo" and " % x" are
 *    malformed. Comment lines count as lines: *bad_line and *n_lines index lines, *n_records
 *    counts records (lines that are no comment; a malformed line keeps its unwritten row, as in
 *    gs_parse_edges_device).
 *  - Windows: record i with timestamp ts and size S > 0 has window id ts / S, C++ truncating
 *    division (SummaryBulkAggregation::window_of of the host mirror; Flink's TimeWindow start
 *    floors, so for negative timestamps that are no multiple of S its window lies one lower). A
 *    window is a maximal run of consecutive records with equal id: nothing is sorted or checked
 *    for ascent.
 */
enum { GS_TEXT_THIRD_NONE = 0, GS_TEXT_THIRD_LONG = 1, GS_TEXT_THIRD_EVENT = 2 };
enum { GS_TEXT_INT32 = 1, GS_TEXT_COMMENT_PERCENT = 2 };

/* DEVICE text -> DEVICE columns: record r -> src[r], dst[r] and val[r] (LONG) or del[r] (EVENT);
 * val / del may be NULL when unused. cap counts LINES: the parse writes line-indexed rows and,
 * only if the text holds a comment line, compacts them afterwards, so a text of more than cap
 * lines is GS_ERR_TRUNCATED. *n_lines, *n_records, *bad_line are HOST words. With third = NONE
 * and flags = 0 this is gs_parse_edges_device. Returns GS_OK, GS_ERR_PARSE (the other lines are
 * still written), GS_ERR_TRUNCATED or GS_ERR_INVALID. Queued on `stream`; synchronises it. */
int gs_parse_records_device(void* stream, const char* text, size_t len, int sep, int third, int flags, int64_t* src,
                            int64_t* dst, int64_t* val, uint8_t* del, size_t cap, uint64_t* n_lines,
                            uint64_t* n_records, int64_t* bad_line);

/* The event-time windows of DEVICE timestamps ts[0 .. n), n < 2^32 - 1: first[w] = the first
 * record of window w and window[w] = its id, for w < cap (DEVICE arrays), *n_windows (HOST) =
 * their number. Returns GS_OK, GS_ERR_TRUNCATED (more windows than cap), GS_ERR_INVALID
 * (size <= 0, a null array) or GS_ERR_CAPACITY (n > 2^32 - 2: the tile scan carries 32-bit
 * counts). Queued on `stream`; synchronises it. */
int gs_window_bounds_device(void* stream, const int64_t* ts, size_t n, int64_t size, uint64_t* first,
                            int64_t* window, size_t cap, uint64_t* n_windows);

/* ---- The text reader: HOST text -> chunks of DEVICE columns, for any handle's *_fold_device.
 *
 * The text is cut at line boundaries into chunks of at most chunk_bytes, copied through
 * double-buffered pinned staging and parsed on the reader's stream. The reader owns two sets of
 * output columns that alternate: the arrays gs_text_next call k returns stay untouched until
 * call k + 2. gs_text_next returns with the chunk complete on the reader's stream (it has
 * synchronised: it returns host counts). A consumer that folds asynchronously on its own stream
 * calls gs_text_wait_stream(t, consumer_stream) before the next gs_text_next.
 *
 * A malformed line: gs_text_next returns GS_ERR_PARSE, gs_text_position gives its global line
 * index; the chunks before it have been delivered (in window mode: their whole windows; the
 * window held back from them is not delivered, the reader is closed with it). A line longer than
 * a chunk: GS_ERR_INVALID. After either, gs_text_open starts again.
 *
 * Window mode (gs_text_set_window, size > 0, third must be LONG): every call delivers whole
 * event-time windows only, first[w] / window[w] for w < *n_windows indexing the delivered
 * records. A chunk's trailing, possibly incomplete, window is held back and prepended (device to
 * device) to the next chunk's records; the call that parses the text's last chunk delivers it.
 * A window may outgrow any number of chunks: the columns grow. */
typedef struct gs_text_s* gs_text;
int gs_text_create(gs_text* out, int device, int sep, int third, int flags, size_t chunk_bytes /* 0 = 16 MiB */);
int gs_text_destroy(gs_text t); /* NULL is GS_OK */
int gs_text_set_window(gs_text t, int64_t size); /* > 0: whole windows only; 0: off. Drops a text not yet read to its end. */
/* HOST bytes, valid until the call of gs_text_next that sets *last; restarts the position. */
int gs_text_open(gs_text t, const char* text, size_t len);
/* The next chunk: DEVICE columns of *n records (*val NULL unless LONG, *del NULL unless EVENT;
 * *first / *window NULL and *n_windows 0 unless window mode), *last = 1 when the text is done
 * (a call after that is GS_ERR_INVALID until the next gs_text_open). src, dst, n, last are
 * required; the other pointers may be NULL. */
int gs_text_next(gs_text t, const int64_t** src, const int64_t** dst, const int64_t** val, const uint8_t** del,
                 size_t* n, const uint64_t** first, const int64_t** window, size_t* n_windows, int* last);
/* The window bounds the last gs_text_next delivered, copied into HOST arrays (a caller without a
 * device runtime of its own cuts the delivered records with them): first[w], window[w] for
 * w < *n = the call's *n_windows. GS_ERR_TRUNCATED when cap < *n. Synchronises the reader's stream. */
int gs_text_windows(gs_text t, uint64_t* first, int64_t* window, size_t cap, size_t* n);
/* Lines and records parsed since gs_text_open (held-back records included), and the global index
 * of the malformed line that ended it, or -1. Any pointer may be NULL. */
int gs_text_position(gs_text t, uint64_t* lines, uint64_t* records, int64_t* bad_line);
int gs_text_sync(gs_text t);
int gs_text_get_stream(gs_text t, void** s);
int gs_text_wait_stream(gs_text t, void* s);

/* Kernel timing of gs_parse_edges_device (measurement; per calling thread): with it on,
 * each parse brackets its parse kernel with HIP events, and gs_parse_profile returns
 * the summed kernel time (microseconds) and the number of parses since it was turned
 * on. Off by default (the events cost a synchronisation per parse). */
int gs_parse_set_profiling(int on);
int gs_parse_profile(double* kernel_us, uint64_t* parses);

/* gs_parse_edges_device keeps a per-thread cache (device scratch of ~1.25 x the longest
 * text parsed, a mapped result record, timing events) across calls. gs_parse_release frees
 * the calling thread's cache; a thread that parses calls it before it ends (a pool thread of
 * a JNI host: when its task finishes). A thread that moves to another device frees the old
 * device's cache at its next parse. */
int gs_parse_release(void);

#ifdef __cplusplus
}
#endif
#endif /* GS_INGEST_H */
