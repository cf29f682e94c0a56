/*
 * gs_testing.h -- PRIVATE test controls of libgs_summary.so. Not part of the drop-in
 * boundary (include/gs_summary.h, gs_group.h, gs_ingest.h): the product path never
 * calls these, and the library reads no environment variable. Tests (tests/test_*.py, the
 * C++ harnesses) use them to reach paths that are otherwise timing-dependent: the
 * window server's idle exit, the change emission's scan fallback, the parse
 * look-back's self-count, and a group folding its own rows back.
 *
 * Every knob is process-wide and starts at its product value; a value < 0 restores
 * the product value. Set them before the operation they affect (a server start, an
 * emission, a parse, a group create).
 */
#ifndef GS_TESTING_H
#define GS_TESTING_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum gs_testing_knob {
  /* resident window server: leave after this many microseconds without a window
   * (product: 2000) */
  GS_TESTING_SERVER_IDLE_US = 0,
  /* change emission: member-list walk limit per hooked root before the scan path
   * (product: 65536) */
  GS_TESTING_CHANGES_WALK_MAX = 1,
  /* text parse: microseconds a look-back waits for its predecessors before it counts
   * the lines before its tile itself (product: ~50000; 0 = at once) */
  GS_TESTING_PARSE_LB_TIMEOUT_US = 2,
  /* exchange group (created afterwards): also fold this rank's own rows back (1) */
  GS_TESTING_GROUP_SELF_APPLY = 3,
  /* exchange group (created afterwards): exchanges between an own fold and its data
   * half, 1..3 (product: 2) */
  GS_TESTING_GROUP_DATA_LAG = 4,
  /* degree fold: kernel variant of the measured alternatives (tools/degree_bench.py):
   * 0 product, 1 no on-chip combining, 2 4096 LDS slots, 3 tile 1024, 4 2048 LDS slots,
   * 5 diagnostic without the counter adds (counts stay 0) */
  GS_TESTING_DEGREE_VARIANT = 5,
  /* triangle fold: work assignment of the count step (tools/triangle_bench.py): 0 product
   * (edges binned by shorter-row length: a lane group of 8, a wave, a workgroup with the
   * longer row sampled in LDS), 1 one wave per new edge */
  GS_TESTING_TRIANGLE_VARIANT = 6,
  /* triangle fold: 1 = bracket the fold's phases with events and wait for them
   * (gs_testing_triangle_stats); product: 0 */
  GS_TESTING_TRIANGLE_PROFILE = 7,
  /* window slices: 1 = bracket the phases of a window, a reduce and an export with events and
   * wait for them (gs_testing_slice_stats); product: 0 */
  GS_TESTING_SLICE_PROFILE = 8,
  /* distinct streams: 1 = bracket the five phases of a fold with events, wait for them, and count
   * the occurrences that issue an atomic minimum (gs_testing_distinct_phases; needed by
   * tools/distinct_bench.py); product: 0 */
  GS_TESTING_DISTINCT_PROFILE = 9,
  /* spanner fold: rounds before the undecided pending edges go to the serial tail (product: 16,
   * and a round that decides less than one in eight ends the rounds too; a set value fixes the
   * number of rounds alone: 0 sends every pending edge to the tail, a huge one leaves no tail) */
  GS_TESTING_SPANNER_ROUND_CAP = 10,
  /* spanner searches: vertices per side of a wave's on-chip sets, 1..256 (product: 256); a search
   * that needs more takes the heavy path */
  GS_TESTING_SPANNER_LDS_SET = 11,
  /* spanner heavy path: arenas of the pool, 1..64 (product: 32); 1 serialises the heavy searches */
  GS_TESTING_SPANNER_ARENAS = 12,
  GS_TESTING_KNOBS = 13
};

/* Set knob `knob` to `value` (< 0: the product value). Returns GS_OK or GS_ERR_INVALID. */
int gs_testing_set(int knob, int64_t value);

/* The current value of a knob (the product value when unset). */
int64_t gs_testing_get(int knob);

/* Diagnostics: the label forest of a partitioned group (gs_group_create_partitioned), as a
 * summary handle the caller may read (gs_counters, gs_debug_counters, gs_num_vertices) but
 * not destroy; *forest = NULL for a replica group. `g` is a gs_group_t. */
int gs_testing_group_forest(void* g, void** forest);

/* Diagnostics of a triangle handle (`t` is a gs_triangles; synchronises): out[0] = intersection
 * steps since reset (the sum over new edges of the shorter row's length), out[1] = the longest
 * row a new edge met, out[2..5] = microseconds of the last profiled fold's canonise, sort and
 * dedup, merge (with the fold's host synchronisation and growth) and count phases. Six words. */
int gs_testing_triangle_stats(void* t, uint64_t* out);

/* The work assignment of a triangle handle's last fold that had new edges (`t` is a
 * gs_triangles; synchronises): out[0] = edges the count step gave to a wave, out[1] = edges it
 * gave to a workgroup with the longer row sampled in LDS; every other new edge took a lane
 * group. Both are 0 under GS_TESTING_TRIANGLE_VARIANT 1 and after a reset. Two words. */
int gs_testing_triangle_bins(void* t, uint64_t* out);

/* The last removal of a triangle handle (`t` is a gs_triangles; gs_triangle_remove,
 * _remove_device or _expire; synchronises): out[0] = edges removed, out[1] = triangles
 * destroyed, out[2] = vertices vanished, out[3] = dying edges the count step gave to a wave,
 * out[4] = to a workgroup with the longer row sampled in LDS (both 0 under
 * GS_TESTING_TRIANGLE_VARIANT 1), out[5] = intersection steps (the sum over the dying edges of
 * the shorter row's length, rows as they were before the removal); out[0..5] are zero when
 * the last removal removed nothing and after a reset. out[6] = slots of the vertex table,
 * out[7] = entries of the adjacency, both as they are now. Eight words. */
int gs_testing_triangle_remove_stats(void* t, uint64_t* out);

/* Microseconds of the last removal's phases under GS_TESTING_TRIANGLE_PROFILE 1 (`t` is a
 * gs_triangles; no device call; zero otherwise): out[0] = mark (the dying edges, the survivors'
 * positions and the host synchronisation), out[1] = rows and count, out[2] = compaction and the
 * table rebuild. Three words. */
int gs_testing_triangle_remove_phases(void* t, uint64_t* out);

/* The fold number of an EMPTY triangle handle (`t` is a gs_triangles; no device call;
 * GS_ERR_INVALID when it holds an edge or value >= 2^32) becomes `value`, so that the next fold
 * takes value + 1: a test places it a few folds before the 32-bit wrap. */
int gs_testing_triangle_set_fold(void* t, uint64_t value);

/* Diagnostics of a slice handle (`s` is a gs_slices; synchronises): out[0] = tiles of the last
 * reduce (0: none yet, the count op reads no tile), out[1] = tiles of the current window that
 * hold no head -- carry records that hand a run on to the next tile --, out[2] = the longest
 * segment of the current window, out[3..7] = microseconds of the last profiled expand, sort,
 * heads, reduce and gather phases (GS_TESTING_SLICE_PROFILE). Eight words. */
int gs_testing_slice_stats(void* s, uint64_t* out);

/* Diagnostics of a distinct handle (`d` is a gs_distinct; no device call): out[0] = slots of the
 * vertex table, out[1] = slots of the edge table, out[2] / out[3] = rebuilds of the vertex / edge
 * table since create, out[4] = the longest probe of the last fold in slots past the home slot
 * (either table; kept with an atomic maximum issued only when a probe left its home slot),
 * out[5] = tiles of the last fold's edge compaction (its entry compaction runs over twice as
 * many positions). Six words. */
int gs_testing_distinct_stats(void* d, uint64_t* out);

/* The last fold of a distinct handle under GS_TESTING_DISTINCT_PROFILE 1 (`d` is a gs_distinct; no
 * device call; all zero otherwise): out[0..4] = microseconds of its vertex probe, vertex
 * compaction, edge probe, edge compaction, and control read with the host synchronisation,
 * out[5] = occurrences that issued an atomic minimum, out[6] = its occurrences (2 n entries + n
 * edges). Seven words. */
int gs_testing_distinct_phases(void* d, uint64_t* out);

/* The last fold of a spanner handle (`s` is a gs_spanner; no device call; zero after a reset):
 * out[0] = arrivals the filter pass dropped (within k in the graph before the fold), out[1] = the
 * pending edges it left, out[2] = rounds run, out[3] = pending edges the serial tail decided,
 * out[4] = searches that overflowed their on-chip sets and took the heavy path (filter pass and
 * rounds), out[5] = the longest row (adjacency plus pending entries) a search expanded. Six words. */
int gs_testing_spanner_stats(void* s, uint64_t* out);

/* Per-handle control of a spanner handle's heavy searches (`s` is a gs_spanner; no device call;
 * not a knob of gs_testing_set): the generations its stamp arenas have used since they were last
 * cleared. With set >= 0 the counter becomes min(set, 0x7FFFFFF0), so that a test can put the
 * next heavy search or tail right before the clear that a handle otherwise reaches after 2^31
 * searches; set < 0 only reads. *out = the counter afterwards. Returns GS_OK or GS_ERR_INVALID. */
int gs_testing_spanner_generation(void* s, int64_t set, uint64_t* out);

/* The last fold of a matching handle (`m` is a gs_matching; no device call; zero after a reset
 * but the last word): out[0] = rounds run (the tail's included), out[1] = fixpoint passes in
 * total, out[2] = arrivals still pending when the tail took over (the arrivals the tail
 * decided), out[3] = arrivals accepted, out[4] = rounds that hit the pass cap before the
 * fixpoint and fell back to plain reservations, out[5] = 1 while the handle is weight-safe
 * (every value folded since the last reset lies in [0, 2^61): sharpening applies). Six words. */
int gs_testing_matching_stats(void* m, uint64_t* out);

/* Per-handle controls of a matching handle's folds (`m` is a gs_matching; not a knob of
 * gs_testing_set): what = 0 the round cap (product: 32 rounds, and fewer than 4096 pending
 * arrivals go to the tail at once; a set value fixes the rounds alone: 0 sends everything to the
 * tail, a huge one leaves no tail), what = 1 the cap of fixpoint passes per round (product: 6;
 * clamped to 1..64), what = 2 sharpening off (value != 0). A value < 0 restores the product
 * value. Returns GS_OK or GS_ERR_INVALID. */
int gs_testing_matching_tune(void* m, int what, int64_t value);

/* The last fold of a trisample handle (`t` is a gs_trisample; no device call; zero after a
 * reset): out[0] = coin successes (resamples), out[1] = segments searched (one carried-in
 * candidate per instance plus one per resample), out[2] = the longest third-vertex draw, in
 * attempts, out[3] = rows; out[4..7] = microseconds of the fold's coin pass with its count read,
 * of the sort and the segments, of the search pass, and of the outcomes and rows with the control
 * read -- zero unless the handle's profile control is on. Eight words. */
int gs_testing_trisample_stats(void* t, uint64_t* out);

/* Per-handle controls of a trisample handle's folds (`t` is a gs_trisample; not a knob of
 * gs_testing_set), so that a test can put a boundary anywhere: what = 0 the arrivals per
 * workgroup of the coin pass (product: 256), what = 1 the arrivals per workgroup of the search
 * pass (product: 1024, which is also the most its LDS stage holds: larger values are clamped),
 * what = 2 profile: bracket the four phases of a fold with events and wait for them (product: off;
 * needed by tools/trisample_bench.py), what = 3 the most keys the resample list is first sized for
 * (product: the expected count S (H(t0 + n) - H(t0)) plus eight deviations): a small value makes
 * the coin pass overflow the list, which is then grown to the count and the pass run again,
 * what = 4 piece: the arrivals of one device piece of a fold (product: 2^20; clamped to 1..2^20):
 * a longer fold is cut into pieces by the host, its stats are the sums (max_attempts: the maximum)
 * over the pieces and its rows are not kept; the fold scratch and the staging of a host fold grow
 * up to it. For what = 0..4 a value <= 0 restores the product value.
 * what = 5 edge_count is an action, not a stored setting: the handle's arrival count becomes
 * `value`, which must lie in 0..2^31 - 1 (GS_ERR_INVALID otherwise); the generators' states, the
 * candidates, betaSum and the last estimate stay as they are. The handle afterwards corresponds to
 * NO real stream: its only use is to put a fold right before the limit of 2^31 - 1 arrivals, as
 * gs_testing_spanner_generation does for the spanner's stamp generations. A reset undoes it.
 * Returns GS_OK or GS_ERR_INVALID (what outside 0..5 included). */
int gs_testing_trisample_tune(void* t, int what, int64_t value);

/* The last fold of a degstream handle (`d` is a gs_degstream; synchronises; zero after a reset
 * but the last two words): out[0] = tiles of the occurrence scan, out[1] = tiles of the fold's
 * two scans (occurrences by vertex, records by degree) that began inside a segment, so that the
 * segment's carry crossed a tile boundary, out[2] = the count array's capacity in degrees (first
 * capacity: 1024), out[3] = growths of the count array since create; out[4..8] = microseconds of
 * the fold's five phases -- ranks and keys, the sort by rank, the clamped scan with the record
 * counts and the control read, the record rows with the sort by degree, the seeded sum -- zero
 * unless the handle's profile control is on. Nine words. */
int gs_testing_degstream_stats(void* d, uint64_t* out);

/* Per-handle control of a degstream handle's folds (`d` is a gs_degstream; not a knob of
 * gs_testing_set): what = 0 profile: bracket the five phases of a fold with events and wait for
 * them, so that the fold ends with a second wait (product: off; needed by
 * tools/degstream_bench.py). A value <= 0 restores the product value. Returns GS_OK or
 * GS_ERR_INVALID. */
int gs_testing_degstream_tune(void* d, int what, int64_t value);

/* The last fold of a tristream handle (`d` is a gs_tristream; synchronises; zero after a reset):
 * out[0] = tiles of the record scan, out[1] = tiles of it that began inside a segment, so that
 * the segment's carry crossed a tile boundary, out[2] = the longest row an arrival met, out[3] =
 * intersection steps (the sum over the arrivals of the walked row's length); out[4..9] =
 * microseconds of the fold's six phases -- ranks, sort and dedupe; merge; rows and count with
 * the control read; offsets and write; record ranks and sort; scan and counters -- zero unless
 * the handle's profile control is on. Ten words. */
int gs_testing_tristream_stats(void* d, uint64_t* out);

/* Per-handle controls of a tristream handle's folds (`d` is a gs_tristream; not knobs of
 * gs_testing_set). what = 0 profile: bracket the six phases of a fold with events and wait for
 * them (product: off; needed by tools/tristream_bench.py). what = 1 record limit: the records a
 * fold may emit before it fails with GS_ERR_CAPACITY (product and maximum: 2^27), so that a
 * test reaches the limit with a few hundred arrivals. A value <= 0 restores the product value.
 * Returns GS_OK or GS_ERR_INVALID. */
int gs_testing_tristream_tune(void* d, int what, int64_t value);

/* The field-spec text parse (include/gs_ingest.h; process-wide, no device call): out[0] = parses
 * that gs_parse_records_device ran with a third field or a flag, out[1] = comment compactions
 * among them (a text without a comment line runs none). Two words. */
int gs_testing_text_stats(uint64_t* out);

/* Per-handle controls of the hot index's build (`h` is a gs_handle of a connected-components
 * summary; not knobs of gs_testing_set): what = 0 the sketch's rows (1 or 2), what = 1 the
 * sketch's counters per row and per id the index can hold, as a log2 (0..6), what = 2 the folds
 * counted for one build (1, 2 or 4: the build comes behind the last of them and takes its
 * candidates from it; a forced index counts 1 unless this says otherwise). A value < 0 restores
 * the library's value. The call waits for the handle's work and drops a live index and a partly
 * counted sketch. Returns GS_OK or GS_ERR_INVALID. */
int gs_testing_hot_tune(void* h, int what, int64_t value);

/* The keys the live hot index of `h` holds, in bucket order: up to `cap` of them into `out`.
 * Waits for the handle's work (a queued build is done and adopted). Returns their number
 * (which may exceed cap; 0 without a live index) or a negative GS_ERR_* code. */
int64_t gs_testing_hot_keys(void* h, int64_t* out, uint64_t cap);

#ifdef __cplusplus
}
#endif
#endif /* GS_TESTING_H */
