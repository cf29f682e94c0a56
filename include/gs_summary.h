/*
 * gs_summary.h -- C ABI of the MI355X-native summary-aggregation hot path.
 *
 * Drop-in boundary for gelly-streaming's SimpleEdgeStream.aggregate() ->
 * SummaryBulkAggregation path as used by ConnectedComponents (DisjointSet summary)
 * and BipartitenessCheck (Candidates summary). A GPU-resident union-find forest
 * (CC) or signed union-find forest (bipartiteness) lives behind an opaque handle;
 * the JVM-side summary objects buffer their per-edge callbacks and flush them here
 * (binding stubs: INTEGRATION.md). Reference paths are relative to
 * src/main/java/org/apache/flink/graph/streaming/ in jiexray/gelly-streaming.
 *
 * Conventions
 *   - Every function returns GS_OK (0) or a negative GS_ERR_* code; the message of
 *     the last failure on the calling thread is gs_last_error() (the reference's
 *     `throws Exception` on foldEdges/reduce, EdgesFold.java:47).
 *   - Plain pointers and sizes only. "host" buffers are caller-owned and copied
 *     before the call returns; "device" buffers must live on the handle's device.
 *   - A handle is thread-compatible (one thread at a time), the library is
 *     re-entrant across handles. Work is enqueued on the handle's own HIP stream;
 *     functions that return data to the host synchronise that stream.
 *   - Vertex ids are signed 64-bit (Edge<Long,...>; Integer ids widen losslessly).
 *     Canonical component label = minimum signed id in the component.
 */
#ifndef GS_SUMMARY_H
#define GS_SUMMARY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gs_summary* gs_handle;

enum gs_status {
  GS_OK = 0,
  GS_ERR_INVALID = -1,  /* bad argument / handle */
  GS_ERR_HIP = -2,      /* HIP runtime error (device missing, OOM, launch failure) */
  GS_ERR_CAPACITY = -3, /* vertex table cannot grow further */
  GS_ERR_TRUNCATED = -4 /* output buffer too small; *n holds the required count */
};

/* Count words (delta takes, exchange stages) carry a failed signed verdict in bit 62. */
#define GS_FAIL_BIT (1ull << 62)

enum gs_kind {
  GS_KIND_CC = 0,     /* DisjointSet (DisjointSet.java:25-151) via ConnectedComponents */
  GS_KIND_SIGNED = 1, /* Candidates (Candidates.java:27-196) via BipartitenessCheck  */
  GS_KIND_DEGREE = 2  /* vertex degrees and their distribution (the gs_degree_* section below) */
};

/* Last error message of the calling thread ("" if none). */
const char* gs_last_error(void);

/* Library/ABI version (major*10000 + minor*100 + patch). */
int gs_version(void);

/* Create an empty summary on HIP device `device`. `capacity_hint` = expected
 * number of distinct vertices: the table starts with >= 4 slots per hinted vertex
 * (load <= 1/4, short probe clusters) and grows past it automatically.
 * Replaces the summary's initial value: `new DisjointSet<>()`
 * (ConnectedComponents.java:52-54) / `new Candidates(true)` (BipartitenessCheck.java:50-52). */
int gs_create(gs_handle* out, int device, int kind, uint64_t capacity_hint);

/* Release the handle and its device memory. */
int gs_destroy(gs_handle h);

/* Reset to the initial value (empty forest, verdict true). Replaces
 * `summary = initialVal` of a transient Merger (SummaryAggregation.java:113-115)
 * and Flink's per-window copy of the initial value (a pooled handle is reset
 * instead of created). Asynchronous; O(vertices) on a sparse table
 * (only the touched slots are re-initialised). */
int gs_reset(gs_handle h);

/* gs_reset plus the handle's default configuration: delta and change tracking off,
 * pipelining depth 1, profiling off -- a pooled handle handed to the next summary
 * behaves as a fresh gs_create (the per-window initial-value copy, INTEGRATION.md
 * HandlePool). Not for a group's summary (destroy the group first). */
int gs_reset_config(gs_handle h);

/* Fold n edges from HOST memory: for each i, union(src[i], dst[i]).
 * Replaces UpdateCC.foldEdges -> DisjointSet.union (ConnectedComponents.java:83-86,
 * DisjointSet.java:92-118) and updateFunction.foldEdges ->
 * candidates.merge(edgeToCandidate(u, v)) (BipartitenessCheck.java:54-61,93-95),
 * called once per buffered micro-batch instead of once per edge.
 * New endpoints are added (DisjointSet.makeSet :53-56); a self-loop adds its vertex
 * and never fails the bipartiteness verdict (BipartitenessCheck.java:58-59).
 * src/dst may be pageable or pinned; the fold itself is asynchronous, but the edges
 * have been copied to the device when the call returns, so the caller may reuse them. */
int gs_fold(gs_handle h, const int64_t* src, const int64_t* dst, size_t n);

/* Same with a required colour parity per edge from HOST memory (GS_KIND_SIGNED; w[i]
 * bit 0: 1 = different sides, as every edge of the stream; 0 = same side). This is a
 * general Candidates merged in component by component (Candidates.merge :77-139 with
 * an input that is not a one-edge candidate: each vertex against its component's
 * anchor, parity = the two signs differ). A CC summary ignores w. */
int gs_fold_parity(gs_handle h, const int64_t* src, const int64_t* dst, const uint8_t* w, size_t n);

/* Same, from DEVICE memory already resident on the handle's device. Element i is
 * src[i*stride], dst[i*stride] (stride 1: two arrays; stride 2 with dst = src + 1:
 * interleaved pairs). `w` (device, optional, may be NULL) gives the required colour
 * parity per edge for GS_KIND_SIGNED (1 = different sides, the edge default;
 * 0 = same side, used when a serialized/exported summary is merged back). The
 * inputs must be complete before work on the handle's stream: written on that
 * stream (gs_get_stream), synchronised, or ordered with gs_wait_event /
 * gs_wait_stream / gs_fold_device_after below. */
int gs_fold_device(gs_handle h, const int64_t* src, const int64_t* dst, const uint8_t* w, size_t n, size_t stride);

/* Micro-batch dedup by hashing (north_star's staging stage). With it on, every fold of
 * edges without a parity array (gs_fold, gs_fold_device with stride 1, the window take)
 * first inserts each edge's unordered pair into a batch hash table and marks exact
 * repeats of a pair within the launch's chunk; the fold skips them (union is
 * idempotent: the result is identical). It pays one batch-table insert per edge, so it
 * is off by default: it wins on streams with many repeated edges (the reference's
 * bipartite example repeats every edge 10 times, BipartitenessCheckExample.java:109-118)
 * and loses on RMAT, whose repeats are rare. */
int gs_set_batch_dedup(gs_handle h, int on);

/* Cross-stream ordering for callers whose edges are produced on another stream (a
 * decoder, a copy engine, torch): gs_wait_event makes every later operation of the
 * handle wait for `event` (a hipEvent_t the producer recorded); gs_wait_stream for
 * all work queued on `stream` (a hipStream_t) so far. No host synchronisation.
 * gs_fold_device_after = gs_wait_event(ready) (skipped when ready is NULL) +
 * gs_fold_device. Pipelined folds and a group's own folds are ordered too. */
int gs_wait_event(gs_handle h, void* event);
int gs_wait_stream(gs_handle h, void* stream);
int gs_fold_device_after(gs_handle h, const int64_t* src, const int64_t* dst, const uint8_t* w, size_t n,
                         size_t stride, void* ready);

/* Pipelined windows: with depth d (1..4), up to d consecutive gs_fold_device calls
 * may run concurrently on the device (fold b+1 starts while fold b drains), the way Flink
 * runs the window fold of window w+1 while the Merger still handles window w
 * (SummaryBulkAggregation.java:77-90 is a pipelined dataflow). Union is associative
 * and commutative, so the forest after the folds is the same; every other call on
 * the handle (reads, exports, combine, serialize, sync, gs_get_stream) first orders
 * the handle's stream behind all pending folds. Device buffers passed to a
 * pipelined fold must stay valid until that next call. Applies to plain folds
 * (no delta or change tracking, profiling off); depth 1 (default) = in order.
 * Each lane is a HIP stream, and streams beyond GPU_MAX_HW_QUEUES share hardware
 * queues (run in submission order): depth 2 fits HIP's default of 4 queues beside the
 * handle's and the process's null stream in any creation order; depth 3 gains ~1 %
 * when its lanes land on distinct queues and loses ~15 % when two share one
 * (DESIGN.md section 7). */
int gs_set_pipelining(gs_handle h, int depth);

/* Hot index of the plain connected-components fold: a small table of the stream's most
 * frequent ids, resident in every L2, probed before the relabel table. A bucket is 16 bytes:
 * two ids, read with one load. An id is held only if the relabel table holds it and one slot
 * chosen per build -- the root most of the sampled hot ids reached -- is an ancestor of its
 * slot: one index serves one component, the one that dominates the stream. A small header
 * beside the buckets names that ancestor and a root found from it later. An edge with both
 * endpoints in the index, or with one in it and the other hanging directly under one of the
 * header's two slots, is done without a find, hook, insert or store; the index is used for
 * nothing else, so results are unchanged. It is rebuilt from a micro-batch, off the folds'
 * critical path, and dropped whenever the table is reset, rebuilt, combined into or
 * deserialized.
 * By default it is on for GS_KIND_CC summaries whose table has at least 256 MiB, in plain
 * host and device folds (no delta or change tracking, no window takes, no window server, no
 * exchange group): 2^17 ids (2^16 buckets, 1 MiB), first due after 2^26 edges since the
 * reset, then every 2048 folds, with a refresh every 16 folds (one wave: the root above the
 * index's ancestor found again, one word stored into the live header). By the default rule a
 * build ranks ids by their occurrences in two folds, the one at which it is due and the next,
 * which it follows and takes its candidates from; a forced index counts one fold. (The library reads
 * no environment variable: the Python binding turns the default off for summaries created
 * while GS_HOT_INDEX=0 is set, for A/B runs.)
 *   log2_entries < 0  : off;
 *   log2_entries == 0 : the defaults above (the other two arguments are ignored);
 *   log2_entries 1..20: at most 2^log2_entries ids (2^(log2_entries - 1) buckets; 1: one
 *                       bucket) whatever the table's size, first built after
 *                       first_after_edges edges, then every rebuild_every_folds folds, with a
 *                       refresh every rebuild_every_folds / 16 folds (none below 16).
 * GS_ERR_INVALID for signed and degree summaries. The call waits for the handle's work.
 * gs_hot_index_stats: out4 = {builds queued since create, ids the live index holds,
 * log2 of the ids it can hold (0: no live index), refreshes queued since create}; it waits
 * for the handle's work as well. The debug-counter build counts the edges the index settled
 * and those that fell back to the table (gs_debug_counters). */
int gs_set_hot_index(gs_handle h, int log2_entries, uint64_t first_after_edges, uint32_t rebuild_every_folds);
int gs_hot_index_stats(gs_handle h, uint64_t* out4);

/* Merge summary `src` into `dst` (either may be on any device; `src` is unchanged).
 * Replaces CombineCC.reduce -> DisjointSet.merge (ConnectedComponents.java:116-126,
 * DisjointSet.java:127-131) and combineFunction.reduce -> Candidates.merge
 * (BipartitenessCheck.java:128-130, Candidates.java:77-139); the verdict is the AND.
 * Asynchronous: src is exported on its stream (over its vertex list when sparse:
 * O(vertices of src), not O(table)), dst folds the rows behind an event; the row
 * count and verdict are read on the device. No host synchronisation and, once the
 * reusable scratch is sized, no allocation. */
int gs_combine(gs_handle dst, gs_handle src);

/* Receiving half of a combine from EXPORTED arrays (gs_export_labels_device of
 * another summary, e.g. received from another rank): folds union(v[i], label[i])
 * with required parity parity[i] (NULL for GS_KIND_CC) -- DisjointSet.merge
 * (DisjointSet.java:127-131: union(k, parent(k)) for every entry) -- and ANDs the
 * verdict with !failed (BipartitenessCheck.java:128-130 -> Candidates.java:79-81).
 * DEVICE arrays on h's device; queued on h's stream. */
int gs_combine_exported_device(gs_handle h, const int64_t* v, const int64_t* label, const uint8_t* parity, size_t n,
                               int failed);

/* Block until all work queued on the handle has finished. */
int gs_sync(gs_handle h);

/* Number of distinct vertices seen (DisjointSet.getMatches().size(), :44-46). On a degree
 * summary: the table entries, those whose net count is <= 0 included. */
int gs_num_vertices(gs_handle h, uint64_t* n);

/* Canonical label of one vertex: *label = min id of its component; *found = 0 if
 * the vertex was never seen (DisjointSet.find returns null, :66-69). */
int gs_find(gs_handle h, int64_t v, int64_t* label, int* found);

/* Batched find over DEVICE arrays: label[i] = canonical label of v[i]; found[i]
 * (optional, may be NULL) = 0 for an id never seen (label[i] is then v[i]).
 * Asynchronous on the handle's stream (DisjointSet.find, :66-80, for many ids). */
int gs_find_labels_device(gs_handle h, const int64_t* v, size_t n, int64_t* label, uint8_t* found);

/* Order-independent 64-bit digest of the summary (synchronises): the sum, mod 2^64, over
 * every vertex v of mix64(v ^ C1) * mix64(label(v) + parity(v) * C2) (splitmix64
 * finaliser; parity = 0 for GS_KIND_CC). Two summaries with the same partition (and
 * colouring) have the same digest whatever their fold order, windows, devices or ranks,
 * so replicas are compared without an export -- what the reference's tests compare as
 * sorted strings (ConnectedComponentsTest.java:54-63, DisjointSet.toString :134-150).
 * A GS_KIND_SIGNED summary whose verdict failed digests to GS_DIGEST_FAILED, as its
 * output is (false,{}) (Candidates.java:194-196). Not part of the reference API. */
#define GS_DIGEST_FAILED (~0ull)
int gs_digest(gs_handle h, uint64_t* digest);

/* Export every (vertex, canonical label) pair to HOST arrays of capacity `cap`,
 * unordered. *n = number of vertices (GS_ERR_TRUNCATED if cap < *n; nothing
 * written). Replaces getMatches()/find()/toString() sinks (DisjointSet.java:44-46,
 * 134-150; ConnectedComponentsExample.FlattenSet :143-156). */
int gs_export_labels(gs_handle h, int64_t* v, int64_t* label, size_t cap, size_t* n);

/* Same into DEVICE arrays; *n is written on the host (synchronises). Used for
 * the final canonical label pass without a device->host copy. `parity` (device,
 * may be NULL) receives parity(v) xor parity(label) for GS_KIND_SIGNED. */
int gs_export_labels_device(gs_handle h, int64_t* v, int64_t* label, uint8_t* parity, size_t cap, size_t* n);

/* Part `part` of `nparts` of the same export: the vertices whose dense id (table
 * slot) lies in the part-th of nparts equal slot ranges. The parts are disjoint and
 * together are exactly gs_export_labels_device. Replicas kept equal by a group
 * (gs_group.h) emit the final label pass partitioned: rank r exports part r, like
 * a Flink sink at parallelism p consuming a keyed stream. DEVICE arrays; *n on the
 * host (synchronises). */
int gs_export_labels_part_device(gs_handle h, int part, int nparts, int64_t* v, int64_t* label, uint8_t* parity,
                                 size_t cap, size_t* n);

/* Bipartiteness verdict so far (Candidates.getSuccess, :44-46): 1 = bipartite. */
int gs_bip_status(gs_handle h, int* ok);

/* Canonical colouring to HOST arrays (Candidates.getMap, :48-50): comp = min id of
 * the component, sign = 1 when v has the colour of comp (SignedVertex sign,
 * SignedVertex.java:23-40). Unordered. When the verdict is false, *n = 0
 * (the reference's fail() state is (false,{}), Candidates.java:194-196). */
int gs_export_colouring(gs_handle h, int64_t* comp, int64_t* v, uint8_t* sign, size_t cap, size_t* n);

/* ---- grouped component export (sinks that read the summary grouped and ordered) ----
 * Number of components (roots), what DisjointSet.toString's grouping map
 * (DisjointSet.java:134-150) or Candidates.getMap().size() (Candidates.java:48-50) would
 * count, without an ordered export: one unordered label pass and a count of the rows
 * with v == label. 0 for a GS_KIND_SIGNED summary whose verdict failed -- its output is
 * (false,{}) (Candidates.java:194-196). Synchronises. */
int gs_num_components(gs_handle h, uint64_t* n);

/* The summary grouped and ordered, as CSR, into DEVICE arrays -- the canonical form of
 * DisjointSet.toString() (DisjointSet.java:134-150: vertices grouped by root) and of
 * Candidates.getMap() (Candidates.java:48-50: a TreeMap of components, each an ordered map
 * of SignedVertex, SignedVertex.java:23-40), sorted on the device instead of by the sink:
 *   comp[0..nc)      component labels (= minimum id), ascending in SIGNED int64 order
 *   offset[0..nc]    uint64 start of each component in member[]; offset[nc] = nv
 *   member[0..nv)    vertices, ordered by (label ascending, vertex ascending), signed order
 *   sign[0..nv)      optional (may be NULL): 1 when the vertex has the colour of its
 *                    component's minimum (gs_export_colouring's sign); 0 for GS_KIND_CC
 * cap_v / cap_c are the capacities of member/sign and of comp (offset holds cap_c + 1).
 * *nv, *nc on the host (synchronises). GS_ERR_TRUNCATED with *nv, *nc set and nothing
 * written if either capacity is too small. A failed signed verdict gives nv = nc = 0
 * (Candidates.java:194-196). An empty summary gives nv = nc = 0 and offset[0] = 0.
 * Read-only on the summary (gs_digest, delta and change tracking are unaffected). The
 * sort's scratch (24 bytes per vertex and a histogram table) is allocated by the first
 * call, kept in the handle and counted by gs_hbm_bytes. */
int gs_export_components_device(gs_handle h, int64_t* comp, uint64_t* offset, int64_t* member, uint8_t* sign,
                                size_t cap_v, size_t cap_c, size_t* nv, size_t* nc);

/* Same into HOST arrays: what a JVM sink or the C++ mirror formats toString() /
 * getMap() from without sorting (DisjointSet.java:134-150, Candidates.java:48-50,
 * ConnectedComponentsExample.FlattenSet :143-156). */
int gs_export_components(gs_handle h, int64_t* comp, uint64_t* offset, int64_t* member, uint8_t* sign, size_t cap_v,
                         size_t cap_c, size_t* nv, size_t* nc);

/* Checkpoint: compact (vertex, label, parity) image of the summary plus the
 * verdict, for Merger.snapshotState/restoreState (SummaryAggregation.java:127-135).
 * Call with buf = NULL to get *len. gs_deserialize replaces the summary: a gs_reset,
 * then a fold of the image's rows. On a handle with change tracking on that is what a
 * sink sees too: the reset empties the summary (changes not yet taken are dropped, and
 * the sink's state is to be dropped with them), and the next take emits every vertex of
 * the image once, so a sink cleared at the deserialize holds exactly the image's rows. */
int gs_serialize(gs_handle h, void* buf, size_t cap, size_t* len);
int gs_deserialize(gs_handle h, const void* buf, size_t len);

/* ---- streaming delta (multi-GPU combine; see DESIGN.md "Multi-GPU") ----------
 * While tracking is on, every fold records the structural changes it made:
 * each successful hook as (root, new parent, parity) and each new vertex seen
 * only through a self-loop as (v, v, 0) (every other new vertex is named by a
 * hook record): at most one record per folded edge. Folding another replica's
 * delta into this summary reproduces that replica's changes (union is associative
 * and commutative), which replaces shipping whole summaries to one reducer
 * (SummaryBulkAggregation.java:77-83).
 *
 * The delta list holds the records of gs_delta_capacity() rows (the folds of at
 * least 2^22 edges, more after gs_group_create with a larger batch) between two
 * takes/stages; a tracked fold past that fails with GS_ERR_CAPACITY before it folds
 * anything (a host fold of several staging chunks is refused as a whole).
 *
 * gs_take_delta_records packs the delta accumulated since the previous take into
 * DEVICE records {a, b, w} (24 bytes; w bit 0 = parity, w bit 7 = skip), first
 * `cap` of them, and writes the COUNT WORD to the DEVICE word *count: the total
 * record count, | GS_FAIL_BIT (2^62) once a GS_KIND_SIGNED summary's verdict has
 * failed -- a failed verdict travels with the records even when no record names
 * the odd cycle (Candidates.merge :79-81). Both complete on the handle's stream (no
 * host synchronisation). gs_fold_records_device folds such records (track = 0:
 * apply another replica's delta without re-recording it); `n` may be a count word
 * (rows | GS_FAIL_BIT): the failure is ANDed into the verdict before the rows fold.
 * gs_fold_records_counted_device is the same replay with the count word read on the
 * DEVICE (*count_dev as a take wrote it; at most `cap` rows), so a consumer replays a
 * window with no host round trip.
 *
 * gs_fold_take_device is one small window of the latency path (BASELINE config 5:
 * per window fold + delta export + completion; PartialAgg.fold then CombineCC /
 * Merger, S/SummaryBulkAggregation.java:109-130, S/SummaryAggregation.java:107-119):
 * fold n device edges with tracking on, take the records since the previous take
 * as gs_take_delta_records does (rec, cap, DEVICE *count_dev), and return when the
 * window is complete with the same count word (rows | GS_FAIL_BIT) in the HOST word
 * *count. A window of at
 * most 2^22 edges with nothing else pending runs as ONE launch whose last workgroup
 * publishes the rows and signals the host through mapped memory. Tracking must be
 * on; change tracking (which consumes the records itself) takes the general path.
 *
 * gs_delta_stage is the exchange form: every pending record into `send` as rows of
 * `width` int64 ({a, b} for CC, {a, b, w} for the signed kind; cap must be at least
 * gs_delta_capacity), and the DEVICE count word *count = rows | 2^62 when the
 * signed verdict has failed (the exchange carries the verdict: Candidates.merge
 * :79-81). gs_fold_exchange_device folds a gathered buffer: `world` blocks of
 * `rows` rows of `width` int64, block r live for its first counts[r] rows (DEVICE
 * count words as staged, failure bits ORed into the verdict), skipping block
 * `skip_rank` (the caller's own). */
int gs_set_delta_tracking(gs_handle h, int on);
int gs_delta_capacity(gs_handle h, uint64_t* rows);
int gs_take_delta_records(gs_handle h, int64_t* rec, size_t cap, uint64_t* count);
int gs_fold_take_device(gs_handle h, const int64_t* src, const int64_t* dst, size_t n, int64_t* rec, size_t cap,
                        uint64_t* count_dev, uint64_t* count);
int gs_delta_stage(gs_handle h, int64_t* send, size_t cap, int width, uint64_t* count);

/* Resident window server for gs_fold_take_device (the latency path without a kernel
 * launch per window). With it on, a window of at most 2^16 edges with nothing else
 * pending is posted to ONE persistent launch through host-mapped memory: its block 0
 * polls the mailbox and hands the window to the other blocks, every block folds 256
 * edges, and the window's last block publishes rows, count word and completion word
 * exactly as the fused launch does. Results are identical; any other call on the
 * handle stops the server first (it restarts at the next window), and a server idle
 * for ~2 ms leaves on its own. While it runs, the server occupies the handle stream's
 * hardware queue: work of ANOTHER stream that HIP mapped onto the same queue
 * (GPU_MAX_HW_QUEUES, 4 by default, are shared round-robin by the process's streams)
 * starts only after the server leaves, i.e. within ~2 ms of the last window (a stop or a
 * call on this handle ends it at once). The edge buffers of a window must be complete before
 * the window is posted and must not be rewritten while the server runs (each window
 * reads its edges once; a stream pre-staged in HBM, as BASELINE config 5 has it).
 * gs_window_server_stats: server launches and windows served. */
int gs_set_window_server(gs_handle h, int on);
int gs_window_server_stats(gs_handle h, uint64_t* launches, uint64_t* windows);
int gs_fold_records_device(gs_handle h, const int64_t* rec, size_t n, int track);
int gs_fold_records_counted_device(gs_handle h, const int64_t* rec, size_t cap, const uint64_t* count_dev, int track);
int gs_fold_exchange_device(gs_handle h, const int64_t* recv, const uint64_t* counts, size_t world, size_t rows,
                            int width, int skip_rank);

/* ---- per-window change emission (sinks) ------------------------------------------
 * The reference's Merger emits the whole cumulative summary every window
 * (SummaryAggregation.java:107-119) and its sinks flatten it: FlattenSet emits
 * (v, find(v)) for every vertex (ConnectedComponentsExample.java:143-156), keyed
 * downstream; DisjointSet.toString groups every vertex (DisjointSet.java:134-150).
 * With change tracking on, gs_take_changes_device emits only the rows a keyed sink
 * needs to reach the same state: (v, canonical label[, parity]) for every vertex
 * inserted or relabelled since the previous take, into DEVICE arrays; *n on the host
 * (synchronises). Work is O(changes): members of each component whose old root was
 * hooked this window are enumerated by walking a member list, not by a table scan;
 * a relabelled component of more than 2^16 vertices is emitted by one parallel scan,
 * which also re-emits the absorbing component's unchanged members (idempotent
 * rows). The first take after a table rebuild emits every vertex. cap must be at
 * least gs_num_vertices (each vertex is emitted at most once). Turns delta
 * tracking on and consumes the delta records (not for a group's summary). */
int gs_set_change_tracking(gs_handle h, int on);
int gs_take_changes_device(gs_handle h, int64_t* v, int64_t* label, uint8_t* parity, size_t cap, uint64_t* n);
/* The same rows into HOST arrays (a JVM sink; parity may be
 * NULL); device scratch is kept in the handle. */
int gs_take_changes(gs_handle h, int64_t* v, int64_t* label, uint8_t* parity, size_t cap, uint64_t* n);

/* ---- degree summary (GS_KIND_DEGREE) -------------------------------------------------
 * Streaming vertex degrees -- SimpleEdgeStream.getDegrees / getInDegrees / getOutDegrees
 * (SimpleEdgeStream.java:366-478) -- and the degree distribution under edge additions and
 * deletions (example/DegreeDistribution.java:52-132), folded on the device. The summary keeps
 * one signed 32-bit NET count per vertex: occurrences added minus occurrences deleted.
 *
 * dir follows DegreeTypeSeparator (SimpleEdgeStream.java:440-459): GS_DEGREE_ALL adds 1 to the
 * source and to the target of every edge (a self-loop counts 2, a repeated edge every time),
 * GS_DEGREE_OUT to the source only, GS_DEGREE_IN to the target only. An endpoint that is not
 * collected is neither looked up nor inserted (getInDegrees never emits a vertex without an
 * in-edge). del (optional, may be NULL = every edge is an addition) holds one byte per edge,
 * of which bit 0 is read: 0 = addition, 1 = deletion (EventType, DegreeDistribution.java:
 * 73-78); a deletion subtracts 1.
 *
 * A vertex whose count is <= 0 is absent from the exports, from the distribution and for
 * gs_degree_find_device (VertexDegreeCounts removes it, DegreeDistribution.java:98-101), but
 * it stays a table entry: gs_num_vertices counts the entries, those at <= 0 included.
 * One difference from the reference: it clamps at removal, so the deletion of an edge that
 * was never added is forgotten there; here it stays in the net count. Streams whose every
 * deletion removes an edge that is present give identical results.
 *
 * Overflow: the handle keeps the endpoint occurrences folded since the last reset (additions
 * and deletions alike; gs_combine adds the source's total, gs_deserialize restores it). A
 * call that would take that total past 2^31 - 1 fails with GS_ERR_CAPACITY and leaves the
 * summary unchanged, so no counter can wrap.
 *
 * A degree summary also serves gs_destroy, gs_reset, gs_reset_config, gs_sync,
 * gs_num_vertices, gs_get_stream, gs_wait_event, gs_wait_stream, gs_table_capacity,
 * gs_combine (dst += src, same kind only) and gs_serialize / gs_deserialize (the image
 * carries its kind); every other call above and below returns GS_ERR_INVALID on it, as the
 * gs_degree_* calls do on a summary of another kind.
 *
 * gs_degree_fold: n edges from HOST arrays (copied before the call returns).
 * gs_degree_fold_device: DEVICE arrays, element i = src[i*stride], dst[i*stride], del[i];
 *   ordered like gs_fold_device (gs_wait_event / gs_wait_stream). Asynchronous.
 * gs_degree_find_device: degree[i] = count of the DEVICE id v[i] when it is > 0, else 0;
 *   found[i] (optional, may be NULL) = 1 when it is > 0. Asynchronous.
 * gs_degree_export_device / gs_degree_export: the (vertex, degree) rows with degree > 0 into
 *   DEVICE / HOST arrays of capacity cap; unordered, or with sorted != 0 ascending by vertex
 *   in signed order (sorted on the device; the sort's scratch is kept in the handle and
 *   counted by gs_hbm_bytes). *n on the host (synchronises); GS_ERR_TRUNCATED with *n set and
 *   nothing written when cap < *n.
 * gs_degree_distribution_device / gs_degree_distribution: degree[0..*n) the distinct degrees,
 *   strictly ascending, count[i] the number of vertices of degree[i] -- the final state of
 *   DegreeDistributionMap (DegreeDistribution.java:116-131). Same capacity rule. */
enum gs_degree_dir { GS_DEGREE_ALL = 0, GS_DEGREE_IN = 1, GS_DEGREE_OUT = 2 };
int gs_degree_fold(gs_handle h, const int64_t* src, const int64_t* dst, const uint8_t* del, size_t n, int dir);
int gs_degree_fold_device(gs_handle h, const int64_t* src, const int64_t* dst, const uint8_t* del, size_t n,
                          size_t stride, int dir);
int gs_degree_find_device(gs_handle h, const int64_t* v, size_t n, int64_t* degree, uint8_t* found);
int gs_degree_export_device(gs_handle h, int64_t* v, int64_t* degree, size_t cap, size_t* n, int sorted);
int gs_degree_export(gs_handle h, int64_t* v, int64_t* degree, size_t cap, size_t* n, int sorted);
int gs_degree_distribution_device(gs_handle h, int64_t* degree, int64_t* count, size_t cap, size_t* n);
int gs_degree_distribution(gs_handle h, int64_t* degree, int64_t* count, size_t cap, size_t* n);

/* ---- triangle summary -----------------------------------------------------------
 * Exact triangle counts of a streamed graph: example/WindowTriangles (the count of each
 * window's graph: reset, fold, read) and example/ExactTriangleCount with
 * SimpleEdgeStream.buildNeighborhood (single pass, insertion only: fold after fold).
 *
 * A triangle handle is its own opaque type with its own create call, not a gs_kind. It
 * holds a graph G and its counts. G is the set of distinct unordered pairs {u, v}, u != v,
 * of signed 64-bit ids folded since create or reset: edge direction, repeated edges (inside
 * one fold or across folds) and self-loops do not change G, a self-loop does not register its
 * vertex, and every id is legal, INT64_MIN and INT64_MAX included. The handle answers T (the
 * triangles of G), t(v) for every vertex of G (the triangles through v; their sum is 3 T),
 * the number of edges and the number of vertices -- all 64-bit counters, on the device and
 * here. The answers depend on G only, never on how the stream was cut into folds or ordered.
 *
 * Relation to the reference. On a window without self-loops the count equals
 * WindowTriangles (it deduplicates neighbours in a HashSet too). On a stream without
 * repeated edges and without self-loops T and t(v) equal the final counters of
 * ExactTriangleCount (key -1 the total, the other keys the vertices). The reference
 * intersects a repeated edge again and counts its triangles twice; here it is ignored. The
 * reference's handling of self-loops (the j = i candidates of WindowTriangles.java:103-104,
 * undirected() of a loop) is not reproduced. No gs_combine, serialization or multi-GPU groups.
 *
 * Removal. Edges leave G by name (gs_triangle_remove) or by age (gs_triangle_expire). After any
 * sequence of fold, remove, expire and reset every answer still depends on G only and equals
 * that of a fresh handle that folded exactly G. A vertex whose last edge is removed is no
 * vertex any more: it is not counted, not exported, found = 0, and a new vertex again when a
 * later fold brings it back (INT64_MIN included). G stays a set: a remove deletes the pair
 * however often it was folded. Every edge carries a stamp, the number of the fold that added
 * it -- or, with refresh on (gs_triangle_set_refresh), of the last fold that contained it. Fold
 * numbers count calls: a fold of zero elements takes one too. They have 32 bits; at the wrap
 * the stamps are rebased, so ages within the last 2^31 folds stay exact and older ones read as
 * 2^31. A removal is not a fold: the fold number does not move. It synchronises with the host
 * ONCE (the number of dying edges); a removal after which a vertex vanished rebuilds the vertex
 * table at its capacity (the first such rebuild at a capacity waits once more, to allocate the
 * second table). The table and the adjacency buffers never shrink.
 *
 * Synchronisation: a fold synchronises with the host ONCE, to learn the number of new edges
 * and grow its arrays; apart from that gs_triangle_fold_device is ordered like
 * gs_fold_device (its reads of src / dst are queued on the handle's stream:
 * gs_triangle_wait_stream orders them behind a producer). Adjacency entries (two per edge)
 * are indexed by the sort's 32-bit payload: a fold that could take them past 2^32 - 1 fails
 * with GS_ERR_CAPACITY before any work. Every device allocation of a handle, growth
 * included, is counted by gs_hbm_bytes and released by gs_triangle_destroy.
 *
 * gs_triangle_create: edge_hint sizes the first allocation only (growth keeps the counts).
 * gs_triangle_reset: G empty, counters zero, capacity kept.
 * gs_triangle_fold / _fold_device: n edges from HOST arrays (copied before the call
 *   returns) / DEVICE arrays, element i = src[i*stride], dst[i*stride].
 * gs_triangle_remove / _remove_device: n pairs from HOST / DEVICE arrays, with the argument
 *   checks and the stream behaviour of fold / fold_device. Every element names an unordered
 *   pair; a pair of G is removed; a pair not in G, a self-loop, a repeat inside the batch or
 *   the same pair in both directions changes nothing further.
 * gs_triangle_expire: removes every edge whose stamp is older than the last `folds` folds
 *   (stamp + folds <= the current fold number, computed without wrap-around); folds >= 1,
 *   GS_ERR_INVALID otherwise. More folds than were made so far removes nothing. Asynchronous
 *   but for the one synchronisation above.
 * gs_triangle_set_refresh: on != 0: from the next fold on, an edge that a fold contains again
 *   takes that fold's number (both directed entries; a pass behind the count step). Off by
 *   default, and then a fold queues no launch for it.
 * gs_triangle_count: T, |G| and the vertex count on the host (synchronises).
 * gs_triangle_count_device: the same three words into DEVICE memory, asynchronous.
 * gs_triangle_find_device: count[i] = t(v[i]) of the DEVICE id v[i] (0 when absent);
 *   found[i] (optional, may be NULL) = 1 when v[i] is a vertex of G. Asynchronous.
 * gs_triangle_export_device / gs_triangle_export: the rows (vertex, t(vertex)) into DEVICE /
 *   HOST arrays of capacity cap, ascending by vertex in signed order (ordered on the device);
 *   nonzero_only drops the vertices with t = 0. *n on the host (synchronises);
 *   GS_ERR_TRUNCATED with *n set and nothing written when cap < *n.
 * gs_triangle_sync / _get_stream / _wait_stream: as gs_sync / gs_get_stream / gs_wait_stream.
 * Null handles and pointers return GS_ERR_INVALID before any device call. */
typedef struct gs_triangles_s* gs_triangles;
int gs_triangle_create(gs_triangles* out, int device, uint64_t edge_hint);
int gs_triangle_destroy(gs_triangles t); /* NULL is GS_OK */
int gs_triangle_reset(gs_triangles t);
int gs_triangle_fold(gs_triangles t, const int64_t* src, const int64_t* dst, size_t n);
int gs_triangle_fold_device(gs_triangles t, const int64_t* src, const int64_t* dst, size_t n, size_t stride);
int gs_triangle_remove(gs_triangles t, const int64_t* src, const int64_t* dst, size_t n);
int gs_triangle_remove_device(gs_triangles t, const int64_t* src, const int64_t* dst, size_t n, size_t stride);
int gs_triangle_expire(gs_triangles t, uint64_t folds);
int gs_triangle_set_refresh(gs_triangles t, int on);
int gs_triangle_count(gs_triangles t, uint64_t* triangles, uint64_t* edges, uint64_t* vertices);
int gs_triangle_count_device(gs_triangles t, uint64_t* out);
int gs_triangle_find_device(gs_triangles t, const int64_t* v, size_t n, int64_t* count, uint8_t* found);
int gs_triangle_export_device(gs_triangles t, int64_t* v, int64_t* count, size_t cap, size_t* n, int nonzero_only);
int gs_triangle_export(gs_triangles t, int64_t* v, int64_t* count, size_t cap, size_t* n, int nonzero_only);
int gs_triangle_sync(gs_triangles t);
int gs_triangle_get_stream(gs_triangles t, void** stream);
int gs_triangle_wait_stream(gs_triangles t, void* stream);

/* ---- window slices ---------------------------------------------------------------
 * The per-vertex neighbourhoods of one window of an edge stream: SimpleEdgeStream.slice
 * (SimpleEdgeStream.java:135-167) and the SnapshotStream it returns, whose reduceOnEdges,
 * foldNeighbors and applyOnNeighbors (SnapshotStream.java:61-131) read them.
 *
 * A slice handle is its own opaque type. It holds ONE window: a call of gs_slice_window
 * replaces the window before it (capacity is kept). Edge i of the n edges of a window is
 * (src[i], dst[i], val[i]), all int64; val may be NULL (a NullValue stream). The direction
 * turns edges into entries (key, neighbour, value) numbered in arrival order:
 *   GS_SLICE_OUT  entry i = (src, dst, val)              (the reference's default)
 *   GS_SLICE_IN   entry i = (dst, src, val)              (reverse(), keyed by field 0)
 *   GS_SLICE_ALL  entry 2i = (src, dst, val), entry 2i+1 = (dst, src, val)
 *                 (undirected(), SimpleEdgeStream.java:355-360: a self-loop gives two entries)
 * Nothing is deduplicated: repeated edges and loops are entries like any other. The window's
 * vertices are the distinct keys; a vertex's neighbourhood is its entries in ascending entry
 * number, Flink's per-key arrival order. Every id and value is legal, INT64_MIN and
 * INT64_MAX included. A window has at most 2^32 - 1 entries (the sort's payload);
 * more returns GS_ERR_CAPACITY before any device work. n = 0 is a valid, empty window.
 *
 * Two things are read from a window, both with rows in ascending signed vertex order (the
 * reference's order is unspecified):
 *   reduce          one int64 per vertex: GS_SLICE_SUM (two's-complement wrap-around, as Java
 *                   long), GS_SLICE_MIN, GS_SLICE_MAX (signed), GS_SLICE_COUNT (the number of
 *                   entries; values are not read). Equal to reduceOnEdges with the same
 *                   function.
 *   neighbourhoods  a CSR: v[nv], offset[nv + 1], neighbor[ne], val[ne]; the entries of
 *                   vertex k are offset[k] .. offset[k + 1] - 1, in arrival order. What
 *                   foldNeighbors and applyOnNeighbors iterate.
 * On a window without values (val == NULL) only GS_SLICE_COUNT and an export with a NULL val
 * array are valid; anything else returns GS_ERR_INVALID. Not built: floating-point values,
 * user functions on the device, time-window assignment on the device, multi-GPU groups,
 * serialization.
 *
 * Synchronisation: gs_slice_window* synchronises with the host ONCE, to learn the vertex
 * count; its reads of DEVICE src / dst / val are queued on the handle's stream before that
 * (gs_slice_wait_stream orders them behind a producer). gs_slice_reduce_device and
 * gs_slice_neighborhoods_device queue their work on the handle's stream and do not wait;
 * the host-array forms return with their arrays filled. Every device allocation of a handle
 * is counted by gs_hbm_bytes and released by gs_slice_destroy.
 *
 * gs_slice_create: edge_hint sizes the first allocation only (0: none until the first window).
 * gs_slice_window / _window_device: n edges from HOST arrays (copied before the call returns)
 *   / DEVICE arrays, element i = src[i*stride], dst[i*stride], val[i*stride].
 * gs_slice_size: the vertices and entries of the current window (no device call).
 * gs_slice_reduce_device / gs_slice_reduce: v[k], out[k] for the *n vertices into DEVICE / HOST
 *   arrays of capacity cap; GS_ERR_TRUNCATED with *n set and nothing written when cap < *n.
 * gs_slice_neighborhoods_device / gs_slice_neighborhoods: the CSR into DEVICE / HOST arrays;
 *   offset holds cap_v + 1 words, val may be NULL; GS_ERR_TRUNCATED with *nv, *ne set and
 *   nothing written when cap_v < *nv or cap_e < *ne.
 * gs_slice_sync / _get_stream / _wait_stream: as gs_sync / gs_get_stream / gs_wait_stream.
 * Null handles and pointers return GS_ERR_INVALID before any device call; so do an unknown
 * dir and an unknown op. */
typedef struct gs_slices_s* gs_slices;
enum gs_slice_dir { GS_SLICE_OUT = 0, GS_SLICE_IN = 1, GS_SLICE_ALL = 2 };
enum gs_slice_op { GS_SLICE_SUM = 0, GS_SLICE_MIN = 1, GS_SLICE_MAX = 2, GS_SLICE_COUNT = 3 };
int gs_slice_create(gs_slices* out, int device, uint64_t edge_hint);
int gs_slice_destroy(gs_slices s); /* NULL is GS_OK */
int gs_slice_window(gs_slices s, const int64_t* src, const int64_t* dst, const int64_t* val, size_t n, int dir);
int gs_slice_window_device(gs_slices s, const int64_t* src, const int64_t* dst, const int64_t* val, size_t n,
                           size_t stride, int dir);
int gs_slice_size(gs_slices s, uint64_t* vertices, uint64_t* entries);
int gs_slice_reduce_device(gs_slices s, int op, int64_t* v, int64_t* out, size_t cap, size_t* n);
int gs_slice_reduce(gs_slices s, int op, int64_t* v, int64_t* out, size_t cap, size_t* n);
int gs_slice_neighborhoods_device(gs_slices s, int64_t* v, uint64_t* offset, int64_t* neighbor, int64_t* val,
                                  size_t cap_v, size_t cap_e, size_t* nv, size_t* ne);
int gs_slice_neighborhoods(gs_slices s, int64_t* v, uint64_t* offset, int64_t* neighbor, int64_t* val, size_t cap_v,
                           size_t cap_e, size_t* nv, size_t* ne);
int gs_slice_sync(gs_slices s);
int gs_slice_get_stream(gs_slices s, void** stream);
int gs_slice_wait_stream(gs_slices s, void* stream);

/* ---- distinct streams -------------------------------------------------------------
 * The first-seen edges and vertices of an edge stream: SimpleEdgeStream.distinct
 * (SimpleEdgeStream.java:301-323) and getVertices (SimpleEdgeStream.java:116-121, 181-202),
 * with the running numberOfVertices stream read off the same state.
 *
 * A distinct handle is its own opaque type. It holds the set of distinct vertices and the set
 * of distinct edges folded since create or reset. A fold of n edges answers which of them are
 * seen for the first time. Edge i of the fold is arrival number folded + i of the stream; its
 * endpoints are entries 2i (src) and 2i + 1 (dst) of the fold.
 *   new edges     edge i is new when no earlier arrival -- in an earlier fold or at a smaller i of
 *                 this fold -- has the same key: the ordered pair (src, dst) in
 *                 GS_DISTINCT_DIRECTED mode, the unordered pair in GS_DISTINCT_UNDIRECTED mode.
 *                 The occurrence kept is always the FIRST in arrival order; its index i is
 *                 reported (take val[i]: the reference emits the first edge with its value).
 *                 New edges are reported ascending by i, with the orientation they arrived with.
 *                 A self-loop is an edge like any other.
 *   new vertices  entry e is new when its id occurs at no earlier entry of the stream; reported
 *                 ascending by e (src before dst, a loop's vertex once). The rank of a vertex is
 *                 its 0-based position in that order over the whole stream and never changes;
 *                 the running numberOfVertices() stream emits k + 1 at the entry of the vertex
 *                 of rank k.
 * Every int64 id is legal, INT64_MIN and INT64_MAX included. Results depend on the stream
 * only, never on how it was cut into folds. Limits, refused with GS_ERR_CAPACITY before any
 * device work: n <= 2^31 - 2 edges per fold, at most 2^32 - 2 distinct vertices, and tables of
 * at most 2^31 slots (vertices + 2 n and edges + n of a fold at most 2^30).
 *
 * Relation to the reference. DistinctEdgeMapper (SimpleEdgeStream.java:310-323) keeps ONE
 * HashSet of targets per parallel subtask, not one per source vertex; at parallelism 1 it
 * therefore drops every edge whose target was seen before -- on TestDistinct's input (2,3) and
 * (4,5). Its own test (TestDistinct.java:38-44) pins all seven edges and its Javadoc says "a
 * neighborhood set for each vertex". This section implements the documented, pinned behaviour:
 * distinct (src, dst) pairs, first occurrence kept (the same choice as for Candidates). The
 * undirected mode has no reference counterpart. getVertices() at parallelism 1 is reproduced
 * exactly, emission order included.
 *
 * Synchronisation: a fold synchronises with the host ONCE, at its end, to read the two new
 * counts; whether a table grows is decided before the fold from host-known totals (worst case
 * + 2 n vertices, + n edges), so no table grows inside a fold. (A fold that does grow a table
 * or its scratch waits once more before the old arrays are freed.) Reads of DEVICE src / dst
 * are queued on the handle's stream (gs_distinct_wait_stream orders them behind a producer);
 * HOST arrays are copied before the call returns. The _device readers and the probes queue
 * their work on the handle's stream and do not wait; the host-array forms return with their
 * arrays filled. The emissions of a fold stay readable until the next fold or reset. Every
 * device allocation of a handle is counted by gs_hbm_bytes and released by gs_distinct_destroy.
 *
 * gs_distinct_create: the hints size the first tables only (0: the smallest).
 * gs_distinct_reset: both sets empty, folded = 0; capacity is kept.
 * gs_distinct_fold / _fold_device: n edges from HOST / DEVICE arrays, element i at index
 *   i * stride of the device arrays.
 * gs_distinct_size: totals and the last fold's counts (no device call).
 * gs_distinct_new_edges* / _new_vertices*: the last fold's emissions into HOST / DEVICE arrays
 *   of capacity cap; index / src / dst (resp. v / entry) may each be NULL.
 * gs_distinct_vertices*: every vertex in rank order. gs_distinct_edges*: every edge ascending
 *   by first arrival, first[k] = that arrival number; src / dst / first may each be NULL.
 *   A capacity below the row count returns GS_ERR_TRUNCATED with *n set and nothing written.
 * gs_distinct_rank_device: rank[i] of the DEVICE id v[i], -1 when absent; found may be NULL.
 * gs_distinct_contains_device: found[i] = the pair (src[i], dst[i]) is in the edge set (either
 *   orientation in undirected mode). Both are read-only and asynchronous on the handle's stream.
 * gs_distinct_sync / _get_stream / _wait_stream: as gs_sync / gs_get_stream / gs_wait_stream.
 * Null handles and pointers, and an unknown mode, return GS_ERR_INVALID before any device
 * call. Not built: edge values on the device (take them through index), multi-GPU groups,
 * serialization, removal. */
typedef struct gs_distinct_s* gs_distinct;
enum gs_distinct_mode { GS_DISTINCT_DIRECTED = 0, GS_DISTINCT_UNDIRECTED = 1 };
int gs_distinct_create(gs_distinct* out, int device, int mode, uint64_t vertex_hint, uint64_t edge_hint);
int gs_distinct_destroy(gs_distinct d); /* NULL is GS_OK */
int gs_distinct_reset(gs_distinct d);
int gs_distinct_fold(gs_distinct d, const int64_t* src, const int64_t* dst, size_t n);
int gs_distinct_fold_device(gs_distinct d, const int64_t* src, const int64_t* dst, size_t n, size_t stride);
int gs_distinct_size(gs_distinct d, uint64_t* vertices, uint64_t* edges, uint64_t* folded, uint64_t* new_vertices,
                     uint64_t* new_edges);
int gs_distinct_new_edges_device(gs_distinct d, uint32_t* index, int64_t* src, int64_t* dst, size_t cap, size_t* n);
int gs_distinct_new_edges(gs_distinct d, uint32_t* index, int64_t* src, int64_t* dst, size_t cap, size_t* n);
int gs_distinct_new_vertices_device(gs_distinct d, int64_t* v, uint32_t* entry, size_t cap, size_t* n);
int gs_distinct_new_vertices(gs_distinct d, int64_t* v, uint32_t* entry, size_t cap, size_t* n);
int gs_distinct_vertices_device(gs_distinct d, int64_t* v, size_t cap, size_t* n);
int gs_distinct_vertices(gs_distinct d, int64_t* v, size_t cap, size_t* n);
int gs_distinct_edges_device(gs_distinct d, int64_t* src, int64_t* dst, uint64_t* first, size_t cap, size_t* n);
int gs_distinct_edges(gs_distinct d, int64_t* src, int64_t* dst, uint64_t* first, size_t cap, size_t* n);
int gs_distinct_rank_device(gs_distinct d, const int64_t* v, size_t n, int64_t* rank, uint8_t* found);
int gs_distinct_contains_device(gs_distinct d, const int64_t* src, const int64_t* dst, size_t n, uint8_t* found);
int gs_distinct_sync(gs_distinct d);
int gs_distinct_get_stream(gs_distinct d, void** stream);
int gs_distinct_wait_stream(gs_distinct d, void* stream);

/* ---- k-spanner summary ------------------------------------------------------------
 * The streaming k-spanner of library/Spanner.java over summaries/AdjacencyListGraph.java: the
 * third SummaryBulkAggregation of the reference's library (example/SpannerExample drives it).
 *
 * A spanner handle is its own opaque type with its own create call. It holds an undirected
 * simple graph G over signed 64-bit ids, which may also hold self-loops {u, u}; every id is
 * legal, INT64_MIN and INT64_MAX included.
 *   within(s, t, k)  AdjacencyListGraph.boundedBFS: false when s is no vertex of G; otherwise
 *                    true iff t is reached from s by 1..k edges of G without revisiting s: for
 *                    s != t iff dist_G(s, t) <= k, for s == t iff the loop {s, s} is in G.
 *                    1 <= k <= 16; any other k returns GS_ERR_INVALID, in gs_spanner_create and
 *                    in gs_spanner_within* (the reference treats k <= 0 like k = 1).
 *   fold             Spanner.UpdateLocal over the n edges in arrival order: edge i is accepted
 *                    (added to G) iff within(src[i], dst[i], k) is false on the graph the edges
 *                    0 .. i-1 left, otherwise dropped. So a repeated edge is dropped, a self-loop
 *                    is kept the first time only, direction does not matter, and the accepted set
 *                    is a function of the stream order alone, however the stream is cut into
 *                    folds. The fold runs in parallel on the device and is exact to that
 *                    sequential order. accepted[i] = 1 / 0 per arrival.
 *   combine          Spanner.CombineSpanners: the edges of `from` folded into `into` with into's
 *                    k, in ascending signed (lo, hi) order, each undirected edge once; `from` is
 *                    unchanged. The reference iterates its hash maps, which is this order for
 *                    small non-negative ids; its order elsewhere is an accident of HashMap
 *                    capacity and is not reproduced. Both handles on one device.
 * Not built: deletions, serialization, multi-GPU groups.
 *
 * Synchronisation: a fold synchronises with the host several times (the pending count, one or
 * two words per round, the accepted count); its reads of DEVICE src / dst are queued on the
 * handle's stream (gs_spanner_wait_stream orders them behind a producer). Adjacency entries
 * (two per edge, one per loop) are 32-bit indices: a fold that could take them past 2^32 - 2
 * fails with GS_ERR_CAPACITY before any work. Every device allocation of a handle is counted by
 * gs_hbm_bytes and released by gs_spanner_destroy.
 *
 * gs_spanner_create: k as above; edge_hint sizes the first allocation only.
 * gs_spanner_reset: G empty, capacity and k kept.
 * gs_spanner_fold / _fold_device: n edges from HOST arrays (copied before the call returns) /
 *   DEVICE arrays, element i = src[i*stride], dst[i*stride]; accepted (may be NULL): n bytes,
 *   HOST / DEVICE (the device form queues the copy on the handle's stream).
 * gs_spanner_add: AdjacencyListGraph.addEdge for n HOST edges in order: every edge joins G
 *   unless G holds it already (the fold with k = 1, whatever the handle's k).
 * gs_spanner_within / _within_device: out[i] = within(src[i], dst[i], k) on G as it stands, HOST /
 *   DEVICE arrays; the device form leaves out[] queued on the handle's stream.
 * gs_spanner_combine: as above (synchronises).
 * gs_spanner_count: the edges (a loop counts as one) and the vertices of G (synchronises).
 * gs_spanner_export_device / gs_spanner_export: the edges (lo <= hi) into DEVICE / HOST arrays of
 *   capacity cap, ascending by (lo, hi) in signed order. *n on the host (synchronises);
 *   GS_ERR_TRUNCATED with *n set and nothing written when cap < *n.
 * gs_spanner_neighbors: the adjacency as a CSR in HOST arrays, what getAdjacencyMap() holds and
 *   SpannerExample.FlattenSet reads: v[nv] ascending, offset[nv + 1], neighbor[ne] ascending
 *   inside each row (a loop appears once in its row). GS_ERR_TRUNCATED with *nv, *ne set and
 *   nothing written when cap_v < *nv or cap_e < *ne.
 * gs_spanner_sync / _get_stream / _wait_stream: as gs_sync / gs_get_stream / gs_wait_stream.
 * Null handles and pointers return GS_ERR_INVALID before any device call. */
typedef struct gs_spanner_s* gs_spanner;
int gs_spanner_create(gs_spanner* out, int device, int k, uint64_t edge_hint);
int gs_spanner_destroy(gs_spanner s); /* NULL is GS_OK */
int gs_spanner_reset(gs_spanner s);
int gs_spanner_fold(gs_spanner s, const int64_t* src, const int64_t* dst, size_t n, uint8_t* accepted);
int gs_spanner_fold_device(gs_spanner s, const int64_t* src, const int64_t* dst, size_t n, uint8_t* accepted,
                           size_t stride);
int gs_spanner_add(gs_spanner s, const int64_t* src, const int64_t* dst, size_t n);
int gs_spanner_within(gs_spanner s, const int64_t* src, const int64_t* dst, size_t n, int k, uint8_t* out);
int gs_spanner_within_device(gs_spanner s, const int64_t* src, const int64_t* dst, size_t n, int k, uint8_t* out);
int gs_spanner_combine(gs_spanner into, gs_spanner from);
int gs_spanner_count(gs_spanner s, uint64_t* edges, uint64_t* vertices);
int gs_spanner_export_device(gs_spanner s, int64_t* lo, int64_t* hi, size_t cap, size_t* n);
int gs_spanner_export(gs_spanner s, int64_t* lo, int64_t* hi, size_t cap, size_t* n);
int gs_spanner_neighbors(gs_spanner s, int64_t* v, uint64_t* offset, int64_t* neighbor, size_t cap_v, size_t cap_e,
                         size_t* nv, size_t* ne);
int gs_spanner_sync(gs_spanner s);
int gs_spanner_get_stream(gs_spanner s, void** stream);
int gs_spanner_wait_stream(gs_spanner s, void* stream);

/* ---- weighted matching ---------------------------------------------------------------
 * The streaming greedy weighted matching of example/CentralizedWeightedMatching.java with the
 * event stream of util/MatchingEvent.java (the reference runs it at parallelism 1 and scans the
 * whole matching for every edge).
 *
 * A matching handle is its own opaque type with its own create call. It holds a set M of edges
 * (src, dst, value), signed 64-bit each; every id is legal, INT64_MIN and INT64_MAX included. M
 * starts empty.
 *   fold     Arrivals are taken in order. For arrival e = (u, v, w): collisions(e) is the set of
 *            edges of M that have u or v as an endpoint -- at most two; one edge that touches both
 *            endpoints counts once; for a self-loop e = (u, u) it is u's edge. sum is the sum of
 *            their values in Java long arithmetic, wrapping. e is accepted iff w > 2 * sum,
 *            wrapping again (CentralizedWeightedMatching.java:79-106). An accepted e removes its
 *            collisions from M and joins M, its orientation kept. accepted[i] = 1 / 0.
 *            M is therefore always a matching, and M is a function of the stream order alone,
 *            however the stream is cut into folds: the fold runs in parallel (rounds of
 *            reservations) and is exact to that order.
 *   events   The MatchingEvent stream of the last fold: each accepted arrival gives its REMOVE
 *            events and then one ADD; rows (arrival index in the fold, type, src, dst, value)
 *            ascending by arrival. The reference emits the one or two REMOVEs of an arrival in
 *            HashSet iteration order, an accident of hash codes; here the edge at the arrival's
 *            source endpoint comes first, then the edge at its target endpoint.
 * Consequences: a value <= 0 is never accepted while no sum has wrapped; a repeated edge is
 * rejected (w > 2 w is false for w >= 0); direction does not matter for collisions but is kept in
 * M and in events.
 *
 * Synchronisation: a fold waits for the handle's stream once per round it runs outside the tail
 * (two words read back; RMAT streams take about ten rounds, a fold of fewer than 4096
 * arrivals takes none) and once at its end (the counts); the tail
 * (one workgroup, no host round trip) finishes what the rounds leave. Every allocation is
 * counted by gs_hbm_bytes and released by gs_matching_destroy. Null handles and pointers return
 * GS_ERR_INVALID before any device call.
 *
 * gs_matching_create: vertex_hint sizes the first allocation only (the handle grows).
 * gs_matching_reset: M empty, no vertex seen, capacity kept.
 * gs_matching_fold / _fold_device: n arrivals from HOST arrays (copied before the call returns) /
 *   DEVICE arrays read on the handle's stream, element i at index i * stride; accepted (may be
 *   NULL): n bytes, HOST / DEVICE. A fold of more than 2^30 arrivals is cut into pieces by the
 *   library, with the same result; its events are then not kept (gs_matching_events returns
 *   GS_ERR_INVALID until the next fold).
 * gs_matching_events / _events_device: the last fold's event rows into HOST / DEVICE arrays of
 *   capacity cap (any array may be NULL); *n = the rows. cap < rows: GS_ERR_TRUNCATED, *n set,
 *   nothing written.
 * gs_matching_count: |M|, the distinct vertex ids seen since reset, and the wrapping sum of M's
 *   values. No device call.
 * gs_matching_export / _export_device: M ascending by the global arrival number (since reset) at
 *   which each edge was accepted, that number in first[] (any array may be NULL); cap and n as
 *   for events.
 * gs_matching_mate_device: per queried DEVICE id v[i]: found[i] = v[i] is matched, mate[i] = its
 *   partner in M (itself for a loop), val[i] = the edge's value; 0, 0, 0 otherwise.
 * gs_matching_sync / _get_stream / _wait_stream: as gs_sync / gs_get_stream / gs_wait_stream.
 * Not built: combine, serialization, multi-GPU groups, deletions. */
enum gs_matching_event { GS_MATCH_ADD = 0, GS_MATCH_REMOVE = 1 }; /* MatchingEvent.Type */
typedef struct gs_matching_s* gs_matching;
int gs_matching_create(gs_matching* out, int device, uint64_t vertex_hint);
int gs_matching_destroy(gs_matching m); /* NULL is GS_OK */
int gs_matching_reset(gs_matching m);
int gs_matching_fold(gs_matching m, const int64_t* src, const int64_t* dst, const int64_t* val, size_t n,
                     uint8_t* accepted);
int gs_matching_fold_device(gs_matching m, const int64_t* src, const int64_t* dst, const int64_t* val, size_t n,
                            uint8_t* accepted, size_t stride);
int gs_matching_events(gs_matching m, uint32_t* arrival, uint8_t* type, int64_t* src, int64_t* dst, int64_t* val,
                       size_t cap, size_t* n);
int gs_matching_events_device(gs_matching m, uint32_t* arrival, uint8_t* type, int64_t* src, int64_t* dst,
                              int64_t* val, size_t cap, size_t* n);
int gs_matching_count(gs_matching m, uint64_t* edges, uint64_t* vertices_seen, int64_t* weight);
int gs_matching_export(gs_matching m, int64_t* src, int64_t* dst, int64_t* val, uint64_t* first, size_t cap,
                       size_t* n);
int gs_matching_export_device(gs_matching m, int64_t* src, int64_t* dst, int64_t* val, uint64_t* first, size_t cap,
                              size_t* n);
int gs_matching_mate_device(gs_matching m, const int64_t* v, size_t n, int64_t* mate, int64_t* val, uint8_t* found);
int gs_matching_sync(gs_matching m);
int gs_matching_get_stream(gs_matching m, void** stream);
int gs_matching_wait_stream(gs_matching m, void* stream);

/* ---- sampling triangle estimate ------------------------------------------------
 * example/BroadcastTriangleCount.java (TriangleSampler and TriangleSummer at parallelism 1,
 * util/TriangleEstimate.java) with the seeded coin of example/IncidenceSamplingTriangleCount.java
 * (EdgeSampleMapper, util/SampledEdge.java): `samples` instances, each holding one candidate
 * (src, trg, third). For arrival number t (from 1) and every instance i:
 *   coin     nextDouble() * (double)t <= 1.0 on the instance's own java.util.Random, exact to the
 *            documented 48-bit LCG; the instance seeds are (long) master.nextInt() of
 *            new Random(seed), drawn in instance order. One nextDouble per instance and arrival,
 *            so the coin is a function of (seed, i, t); it is always true at t = 1.
 *   sample   on success the candidate becomes (src, trg, third) and its flags are cleared. The
 *            reference draws third from the unseeded Math.random(); here it is counter-based:
 *            h = mix64(mix64(third_seed + 0x9E3779B97F4A7C15 * (i + 1)) ^ t), attempt a = 0, 1, ..:
 *            third = floor((mix64(h ^ a) >> 11) * 2^-53 * vertices), the first one that differs
 *            from src and trg (mix64: the finaliser of gs_gen.h's generators).
 *   observe  while beta == 0 the arrival is compared in either direction with {src, third} and
 *            {trg, third}; beta = 1 once both were seen. Ids outside [0, vertices) never match a
 *            third vertex.
 *   rows     betaSum(t) = the instances with beta == 1 after arrival t. A row (t, estimate,
 *            betaSum) is emitted at t iff betaSum(t) != betaSum(t - 1) and its estimate differs
 *            from the estimate at the previous arrival whose betaSum changed (0 before any) --
 *            the two previousResult fields of the reference. estimate =
 *            (int)((((1.0 / samples) * betaSum) * t) * (vertices - 2)) in double, left to right,
 *            cast as Java casts (truncate, saturate, NaN -> 0).
 * The result of folding a stream does not depend on where it is cut into folds. The work of a fold
 * is instances x arrivals: a coin pass and a search pass on the device.
 *
 * Synchronisation: a fold waits for the handle's stream twice (the count of coin successes, the
 * fold's counts). Every allocation is counted by gs_hbm_bytes and released by
 * gs_trisample_destroy. Null handles and pointers return GS_ERR_INVALID before any device call.
 *
 * gs_trisample_create: samples in 1 .. 2^20, vertices in 3 .. 2^31 - 1 (else GS_ERR_INVALID); seed
 *   is a Java long (the reference's is the int literal 0xDEADBEEF widened, -559038737).
 * gs_trisample_reset: no arrival folded, every candidate cleared, the generators reseeded.
 * gs_trisample_fold / _fold_device: n arrivals from HOST arrays (copied before the call returns) /
 *   DEVICE arrays read on the handle's stream, element i at index i * stride; *rows (may be NULL)
 *   = the fold's row count. More than 2^31 - 1 arrivals in total: GS_ERR_INVALID, state untouched.
 *   A fold of more than 2^20 arrivals is cut into pieces by the library, with the same result; its
 *   rows are then not kept (gs_trisample_rows returns GS_ERR_INVALID until the next fold).
 * gs_trisample_rows / _rows_device: the last fold's rows (edge count, estimate, betaSum) into
 *   HOST / DEVICE arrays of capacity cap (any array may be NULL); *n = the rows. cap < rows:
 *   GS_ERR_TRUNCATED, *n set, nothing written.
 * gs_trisample_estimate: arrivals folded, betaSum now, the last emitted estimate (0 before any
 *   row). No device call.
 * gs_trisample_states / _states_device: per instance src, trg, third, flags (bit 0 srcEdgeFound,
 *   bit 1 trgEdgeFound, bit 2 beta) and sampled_at (the edge count at which the candidate was
 *   sampled) into HOST / DEVICE arrays of `samples` elements (any may be NULL); third = -1 and
 *   sampled_at = 0 before the first edge.
 * gs_trisample_sync / _get_stream / _wait_stream: as gs_sync / gs_get_stream / gs_wait_stream.
 * Not built: parallelism above 1 (per-subtask sample shares, the per-source result map),
 * IncidenceSampling's intermediate emissions (the sums it emits while only some instances have
 * seen the current edge; its instance states after every edge equal Broadcast's under the same
 * draws, and those are reproduced), combine, serialization, multi-GPU groups. */
typedef struct gs_trisample_s* gs_trisample;
int gs_trisample_create(gs_trisample* out, int device, uint64_t samples, int64_t vertices, int64_t seed,
                        uint64_t third_seed);
int gs_trisample_destroy(gs_trisample t); /* NULL is GS_OK */
int gs_trisample_reset(gs_trisample t);
int gs_trisample_fold(gs_trisample t, const int64_t* src, const int64_t* dst, size_t n, size_t* rows);
int gs_trisample_fold_device(gs_trisample t, const int64_t* src, const int64_t* dst, size_t n, size_t stride,
                             size_t* rows);
int gs_trisample_rows(gs_trisample t, int32_t* edges, int32_t* estimate, int32_t* beta_sum, size_t cap, size_t* n);
int gs_trisample_rows_device(gs_trisample t, int32_t* edges, int32_t* estimate, int32_t* beta_sum, size_t cap,
                             size_t* n);
int gs_trisample_estimate(gs_trisample t, uint64_t* arrivals, int32_t* beta_sum, int32_t* estimate);
int gs_trisample_states(gs_trisample t, int64_t* src, int64_t* trg, int64_t* third, uint8_t* flags,
                        int32_t* sampled_at);
int gs_trisample_states_device(gs_trisample t, int64_t* src, int64_t* trg, int64_t* third, uint8_t* flags,
                               int32_t* sampled_at);
int gs_trisample_sync(gs_trisample t);
int gs_trisample_get_stream(gs_trisample t, void** stream);
int gs_trisample_wait_stream(gs_trisample t, void* stream);

/* ---- degree streams ------------------------------------------------------------------
 * Every value the reference's degree operators emit, not only the last one: the running
 * Vertex<K, Long> of SimpleEdgeStream.getDegrees / getInDegrees / getOutDegrees
 * (DegreeMapFunction, SimpleEdgeStream.java:461-478) and the (degree, count) record that
 * example/DegreeDistribution.java emits at every change (DegreeDistribution.java:84-132).
 *
 * A degstream handle is its own opaque type with its own create call; its direction
 * (gs_degree_dir) is fixed at create. Every id is legal, INT64_MIN and INT64_MAX included.
 *   occurrences  the collected endpoints of a fold in arrival order: for edge i the source
 *                (GS_DEGREE_OUT or _ALL), then the target (GS_DEGREE_IN or _ALL); a self-loop
 *                gives two occurrences of one vertex under _ALL. An endpoint that is not
 *                collected is neither looked up nor inserted. An occurrence carries c = +1, or
 *                c = -1 when bit 0 of the edge's deletion byte is set; d is the vertex's
 *                degree before it, 0 while the vertex is absent.
 *   rows         old = d, new = max(d + c, 0); the row is (vertex, old, new). A vertex is
 *                present iff d > 0 and an absent vertex forgets a deletion -- the reference's
 *                clamp at removal (VertexDegreeCounts), which the degree summary's net counts
 *                do not have. Without deletions `new` is what DegreeMapFunction emits.
 *   records      per occurrence, in this order: old > 0: (new, +1) if new > 0, then (old, -1);
 *                old == 0 and c > 0: (1, +1); old == 0 and c < 0: none. Taken in arrival
 *                order, count[degree] += delta and the record's row is (occurrence index in
 *                the fold, degree, count[degree]). A count may reach 0 and is then emitted as
 *                0; it never falls below.
 * The rows and records are a function of the stream order alone, however the stream is cut
 * into folds: the fold runs in parallel (two stable sorts and two seeded segmented scans,
 * DESIGN.md section 6i) and is exact to that order.
 *
 * Overflow: the handle keeps the occurrences folded since the last reset; a fold that would
 * take them past 2^31 - 1 fails with GS_ERR_CAPACITY before any work, so no degree or count
 * can wrap.
 *
 * Synchronisation: a fold waits for the handle's stream once (new vertices, record count,
 * largest new degree, error word); the record sort and sum behind it are queued. Every
 * allocation is counted by gs_hbm_bytes and released by gs_degstream_destroy. Null handles and
 * pointers return GS_ERR_INVALID before any device call.
 *
 * gs_degstream_create: dir is a gs_degree_dir; vertex_hint sizes the first allocation only.
 * gs_degstream_reset: no vertex, every count 0, no occurrence folded; capacity kept.
 * gs_degstream_fold / _fold_device: n edges from HOST arrays (copied before the call returns) /
 *   DEVICE arrays read on the handle's stream, element i = src[i*stride], dst[i*stride], del[i];
 *   del may be NULL (every edge an addition). The largest fold whose rows are kept has 2^24
 *   edges; a longer one is cut into pieces by the library, with the same state afterwards, and
 *   gs_degstream_rows / _records return GS_ERR_INVALID until the next fold.
 * gs_degstream_rows / _rows_device: the last fold's (vertex, old, new) per occurrence into HOST /
 *   DEVICE arrays of capacity cap (any array may be NULL); *n = the rows. cap < rows:
 *   GS_ERR_TRUNCATED, *n set, nothing written.
 * gs_degstream_records / _records_device: the last fold's (occurrence, degree, count) per
 *   record, in arrival order; cap and n as for rows.
 * gs_degstream_size: out[0..4] = new vertices, occurrences and records of the last fold, the
 *   occurrences since reset, the largest degree since reset. No device call.
 * gs_degstream_degrees / _degrees_device: the current (vertex, degree) rows with degree > 0, in
 *   first-seen order; gs_degstream_distribution / _distribution_device: the current (degree,
 *   count) rows with count > 0, ascending by degree. *n on the host (synchronises); capacity
 *   rule as above.
 * gs_degstream_sync / _get_stream / _wait_stream: as gs_sync / gs_get_stream / gs_wait_stream.
 * Not built: combine, serialization, multi-GPU groups, parallelism above 1 (where the order of
 * records across keys is Flink's). */
typedef struct gs_degstream_s* gs_degstream;
int gs_degstream_create(gs_degstream* out, int device, int dir, uint64_t vertex_hint);
int gs_degstream_destroy(gs_degstream d); /* NULL is GS_OK */
int gs_degstream_reset(gs_degstream d);
int gs_degstream_fold(gs_degstream d, const int64_t* src, const int64_t* dst, const uint8_t* del, size_t n);
int gs_degstream_fold_device(gs_degstream d, const int64_t* src, const int64_t* dst, const uint8_t* del, size_t n,
                             size_t stride);
int gs_degstream_rows(gs_degstream d, int64_t* vertex, uint32_t* old_degree, uint32_t* new_degree, size_t cap,
                      size_t* n);
int gs_degstream_rows_device(gs_degstream d, int64_t* vertex, uint32_t* old_degree, uint32_t* new_degree, size_t cap,
                             size_t* n);
int gs_degstream_records(gs_degstream d, uint32_t* occurrence, uint32_t* degree, uint32_t* count, size_t cap,
                         size_t* n);
int gs_degstream_records_device(gs_degstream d, uint32_t* occurrence, uint32_t* degree, uint32_t* count, size_t cap,
                                size_t* n);
int gs_degstream_size(gs_degstream d, uint64_t* out);
int gs_degstream_degrees(gs_degstream d, int64_t* vertex, int64_t* degree, size_t cap, size_t* n);
int gs_degstream_degrees_device(gs_degstream d, int64_t* vertex, int64_t* degree, size_t cap, size_t* n);
int gs_degstream_distribution(gs_degstream d, int64_t* degree, int64_t* count, size_t cap, size_t* n);
int gs_degstream_distribution_device(gs_degstream d, int64_t* degree, int64_t* count, size_t cap, size_t* n);
int gs_degstream_sync(gs_degstream d);
int gs_degstream_get_stream(gs_degstream d, void** stream);
int gs_degstream_wait_stream(gs_degstream d, void* stream);

/* ---- triangle streams ----------------------------------------------------------------
 * Every record example/ExactTriangleCount.java emits, not only the final counters:
 * buildNeighborhood(false), ProjectCanonicalEdges, IntersectNeighborhoods and
 * SumAndEmitCounters (ExactTriangleCount.java:52-56, 74-134) at parallelism 1.
 *
 * A tristream handle is its own opaque type with its own create call; how it treats a repeated
 * pair (gs_tristream_repeats) is fixed at create. Every id is legal, INT64_MIN, INT64_MAX and -1
 * included. State: G, a set of unordered pairs {u, v}, u != v, each with first{u,v}, the number
 * of the arrival that added it (1-based, every arrival counted, loops included); a 64-bit
 * counter t(v) per vertex; the 64-bit total T. Arrival number t = (s, d):
 *   1. s == d: nothing is emitted, G, t() and T stay; its row is (closed 0, total T). The
 *      reference's self-loop artefacts are NOT reproduced.
 *   2. u = min(s, d), v = max(s, d) in signed order; {u, v} not in G: it joins with first = t.
 *   3. C = { w : {u, w} in G with first < t and {v, w} in G with first < t }, c = |C|.
 *   4. GS_TRISTREAM_COUNT (the reference): a repeated pair is intersected again.
 *      GS_TRISTREAM_IGNORE: an arrival whose pair was in G before it has c = 0; the final T and
 *      t(v) then equal the triangle summary's (gs_triangle_*).
 *   5. c > 0: the records, in this order: (w, t(w) += 1) for every w of C ascending in signed
 *      order; (u, t(u) += c); (v, t(v) += c); then T += c. The total is not a record: -1 may be a
 *      vertex (the C++ mirror puts (-1, total) back).
 *   6. the arrival's row is (closed = c, total = T after).
 * The rows and records are a function of the stream order alone, however the stream is cut
 * into folds: the fold runs in parallel and is exact to that order.
 *
 * Limits: the arrivals since the last reset stay at or below 2^31 - 1, and one fold emits at most
 * 2^27 records. A fold past either fails with GS_ERR_CAPACITY and leaves G, the counters, the
 * rows and the records as they were before the call: fold smaller pieces, the stream is the
 * same. (A fold of more than 2^22 arrivals is cut into pieces by the library; when a later
 * piece fails, the pieces before it are folded and gs_tristream_size tells how far.)
 *
 * Synchronisation: a fold waits for the handle's stream twice (the new pairs; the record count);
 * the ordered write, the record sort and the sum behind them are queued. Every allocation is
 * counted by gs_hbm_bytes and released by gs_tristream_destroy. Null handles and pointers
 * return GS_ERR_INVALID before any device call.
 *
 * gs_tristream_create: repeats_mode is a gs_tristream_repeats; edge_hint sizes the first
 *   allocation only.
 * gs_tristream_reset: G empty, every counter 0, no arrival folded; capacity kept.
 * gs_tristream_fold / _fold_device: n arrivals from HOST arrays (copied before the call
 *   returns) / DEVICE arrays read on the handle's stream, element i = src[i*stride],
 *   dst[i*stride]. The largest fold whose rows are kept has 2^22 arrivals; a longer one is cut
 *   into pieces by the library, with the same state afterwards, and gs_tristream_rows /
 *   _records return GS_ERR_INVALID until the next fold.
 * gs_tristream_rows / _rows_device: the last fold's (closed, total) per arrival into HOST /
 *   DEVICE arrays of capacity cap (either may be NULL); *n = the rows. cap < rows:
 *   GS_ERR_TRUNCATED, *n set, nothing written.
 * gs_tristream_records / _records_device: the last fold's (arrival index in the fold, vertex,
 *   count) per record, in emission order; cap and n as for rows.
 * gs_tristream_size: out[0..3] = arrivals, records and new pairs of the last fold, the arrivals
 *   since reset. No device call.
 * gs_tristream_count: out[0..3] = T, |G|, the vertices of G, the arrivals since reset.
 *   Synchronises.
 * gs_tristream_counts / _counts_device: the current (vertex, t) rows with t > 0, ascending by
 *   vertex in signed order. *n on the host (synchronises); capacity rule as above.
 * gs_tristream_sync / _get_stream / _wait_stream: as gs_sync / gs_get_stream / gs_wait_stream.
 * Not built: deletions, combine, serialization, multi-GPU groups, parallelism above 1, and the
 * neighbourhood sets buildNeighborhood emits (the adjacency with its stamps holds them). */
typedef enum { GS_TRISTREAM_COUNT = 0, GS_TRISTREAM_IGNORE = 1 } gs_tristream_repeats;
typedef struct gs_tristream_s* gs_tristream;
int gs_tristream_create(gs_tristream* out, int device, int repeats_mode, uint64_t edge_hint);
int gs_tristream_destroy(gs_tristream d); /* NULL is GS_OK */
int gs_tristream_reset(gs_tristream d);
int gs_tristream_fold(gs_tristream d, const int64_t* src, const int64_t* dst, size_t n);
int gs_tristream_fold_device(gs_tristream d, const int64_t* src, const int64_t* dst, size_t n, size_t stride);
int gs_tristream_rows(gs_tristream d, uint32_t* closed, int64_t* total, size_t cap, size_t* n);
int gs_tristream_rows_device(gs_tristream d, uint32_t* closed, int64_t* total, size_t cap, size_t* n);
int gs_tristream_records(gs_tristream d, uint32_t* arrival, int64_t* vertex, int64_t* count, size_t cap, size_t* n);
int gs_tristream_records_device(gs_tristream d, uint32_t* arrival, int64_t* vertex, int64_t* count, size_t cap,
                                size_t* n);
int gs_tristream_size(gs_tristream d, uint64_t* out);
int gs_tristream_count(gs_tristream d, uint64_t* out);
int gs_tristream_counts(gs_tristream d, int64_t* vertex, int64_t* count, size_t cap, size_t* n);
int gs_tristream_counts_device(gs_tristream d, int64_t* vertex, int64_t* count, size_t cap, size_t* n);
int gs_tristream_sync(gs_tristream d);
int gs_tristream_get_stream(gs_tristream d, void** stream);
int gs_tristream_wait_stream(gs_tristream d, void* stream);

/* ---- introspection -----------------------------------------------------------
 * The HIP stream (hipStream_t) the handle enqueues on, and per-kernel timing:
 * when profiling is on, every launch is bracketed by HIP events on the stream it
 * runs on; gs_kernel_stats returns (launches, total milliseconds) for kernel `id`
 * (0 = fold, 1 = stage, 2 = export, 3 = init/reset). gs_capacity_stats: capacity
 * checks that had to wait for in-flight reports, those that synchronised, and the
 * host milliseconds spent waiting. */
int gs_get_stream(gs_handle h, void** stream);
int gs_set_profiling(gs_handle h, int on);
int gs_kernel_stats(gs_handle h, int id, uint64_t* launches, double* total_ms);
int gs_table_capacity(gs_handle h, uint64_t* slots);
int gs_capacity_stats(gs_handle h, uint64_t* waits, uint64_t* syncs, double* wait_ms);

/* HBM accounting for a handle pool's budget (the Java HandlePool,
 * S/SummaryAggregation.java:107-119 and S/SummaryBulkAggregation.java:79-83 drop partials
 * and copies without a release). gs_hbm_bytes: bytes of device memory held right now by
 * every live summary and group of this process on `device` -- tables, vertex lists, delta
 * lists, staging and scratch -- counted by the library's allocator, so a table that grew
 * inside a fold or combine while handed out is included at once. gs_create_bytes: the bytes
 * gs_create(kind, capacity_hint) allocates. Neither synchronises. */
int gs_hbm_bytes(int device, uint64_t* bytes);
int gs_create_bytes(int kind, uint64_t capacity_hint, uint64_t* bytes);

/* Device counters (synchronises): out[0] vertices, [1] bipartiteness failed,
 * [2] table-overflow error, [3] list overflow (bit 0 delta list, bit 1 vertex
 * list), [4] records staged,
 * [5] hook calls, [6] hook-loop iterations, [7] failed hook CASes -- [5..7] only
 * count in the debug build (make -C gelly-streaming_amd debug). */
int gs_counters(gs_handle h, uint64_t* out8);

/* Diagnostics of the fold's memory operations (synchronises), debug build only (all
 * zero otherwise): out[0] edges / rows folded, [1] key CASes issued, [2] key CASes that
 * found the slot taken, [3] agent-scope re-reads before a key CAS, [4] edges settled by
 * the shared-parent shortcut, [5] edges whose finds met one root, [6] parent loads of
 * the finds, [7] hooks that joined two trees, [8] extra linear-probe loads. n <= 16
 * entries are written. Not a reference interface: the tools behind DESIGN.md use it. */
int gs_debug_counters(gs_handle h, uint64_t* out, int n);

#ifdef __cplusplus
}
#endif
#endif /* GS_SUMMARY_H */
