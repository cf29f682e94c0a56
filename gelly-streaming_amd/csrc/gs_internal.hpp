// gs_internal.hpp -- the summary handle and the internal entry points shared by
// gs_capi.cpp (include/gs_summary.h), gs_group.cpp (include/gs_group.h),
// gs_changes.cpp (per-window change emission), gs_degree.cpp and gs_sort.cpp; and what every
// handle type is made from -- the summary here, and the stand-alone summaries of gs_slice.cpp,
// gs_triangle.cpp, gs_distinct.cpp, gs_spanner.cpp, gs_matching.cpp, gs_trisample.cpp,
// gs_degstream.cpp and gs_tristream.cpp: the error macros
// (GS_HIP, GS_LAUNCH), the phase timer, the stream owner each handle derives from with the entry
// points all of them have (sync, get_stream, wait_stream, the null check, the truncation error).
// Every device array a handle owns is a DevBuf (gs_devbuf.hpp), every event, stream and pinned
// host block an Event, Stream or HostBuf (gs_own.hpp): deleting the handle releases them. Groups
// of DevBufs that share a capacity grow through grow_group (gs_grow.hpp); the host-array form of an
// export and the staging of a host fold go through gs_hostio.hpp (ColumnCopy, OutStage,
// FoldStage); a one-column sort is sort_by_key, a two-column one sort_by_pair (gs_sort.hpp); the
// vertex table of the streams that rank their vertices, its fold guard and its growth are
// VertexTable (gs_vtable.hpp). All of it is linked into
// one library, so every summary owns one prefix for its names in namespace gs, in its lower,
// camel and upper case spellings (ts_, kTs, Ts, TS_): degree, tri, slice, dist, sp, mt, ts (the
// sampling triangle estimate), ds (the degree streams), trs (the triangle streams); a new summary
// takes a new one (tests/test_one_definition.py).
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "gs_devbuf.hpp"
#include "gs_grow.hpp"
#include "gs_hostio.hpp"
#include "gs_ingest.hpp"
#include "gs_kernels.hpp"
#include "gs_own.hpp"
#include "gs_sort.hpp"
#include "gs_summary.h"
#include "gs_testing.h"

namespace gsi {

int fail(int code, const std::string& msg);
// gs_testing.h: a test knob's value, or `product` while the knob is unset
int64_t testing_value(int knob, int64_t product);

constexpr int kMaxDevices = 64;  // of the device-memory accounting (dmalloc / dfree, gs_devbuf.hpp)
uint64_t create_capacity(uint64_t capacity_hint);
uint64_t create_bytes(uint64_t cap);

#define GS_HIP(call)                                                                                  \
  do {                                                                                                \
    hipError_t e_ = (call);                                                                           \
    if (e_ != hipSuccess)                                                                             \
      return ::gsi::fail(GS_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_));              \
  } while (0)

// A kernel launch (a gs::launch_* call) and the check of its launch error: a launch without the
// check would hand its error to some later, unrelated call.
#define GS_LAUNCH(...)            \
  do {                            \
    __VA_ARGS__;                  \
    GS_HIP(hipGetLastError());    \
  } while (0)

// The two errors every handle type reports in the same words: a null handle ("null matching
// handle") and an output array too small for its rows.
inline int check_handle(const void* h, const char* what) {
  return h ? GS_OK : fail(GS_ERR_INVALID, std::string("null ") + what + " handle");
}
inline int truncated(size_t cap, uint64_t need) {
  return fail(GS_ERR_TRUNCATED, "output capacity " + std::to_string(cap) + " < " + std::to_string(need));
}

constexpr uint32_t kMaxChunk = 1u << 22;     // edges per k_fold launch
constexpr uint32_t kStageChunk = 1u << 20;   // edges per pinned staging buffer
constexpr double kMaxLoad = 0.70;            // grow the table past this load factor
// Slots per hinted vertex at create (load <= 1/4 at the hinted count). Linear-probe
// clusters set the tail of a small window: config 5 (ER, 2^16-edge windows) p50
// 20.5 -> 13.3 us going from load 1/2 to 1/4; a 2^28-slot table for RMAT-26's 32.8 M
// vertices (load 1/8) was 2 % slower than 2^27 (profiles/r03_capacity_ab.txt).
constexpr uint64_t kSlotsPerHintedVertex = 4;
constexpr uint64_t kMaxCap = 1ull << 30;     // link holds slot << 1 in 32 bits
// A table whose load limit is crossed by pipeline slack alone (the capacity bound
// charges 2 new vertices per in-flight edge) grows once instead of waiting for
// capacity reports on every fold -- up to this many slots (1 GiB); tables keep
// their capacity across resets.
constexpr uint64_t kSlackGrowMaxCap = 1ull << 26;

enum { KID_FOLD = 0, KID_STAGE = 1, KID_EXPORT = 2, KID_INIT = 3, KID_N = 4 };

// per-shard edges of one k_fold launch of c edges (blocks are dealt to the 64
// shards round-robin from a rotating first shard)
inline uint64_t per_shard_edges(uint64_t c) {
  const uint64_t blocks = (c + gs::kFoldBS - 1) / gs::kFoldBS;
  return ((blocks + gs::kShards - 1) / gs::kShards) * gs::kFoldBS;
}

inline uint64_t next_pow2(uint64_t x) {  // the smallest power of two >= x
  uint64_t p = 1;
  while (p < x) p <<= 1;
  return p;
}
inline int log2_ceil(uint64_t x) {  // log2 of next_pow2(x)
  int l = 0;
  while ((1ull << l) < x) ++l;
  return l;
}

// The kernels' view of a relabel table of cap slots (a power of two, logcap its log2) plus the
// reserved slot; vertex list, new marks and host flags off until the caller sets them.
inline gs::Table make_table(gs::Slot* tab, uint32_t* ctr, uint64_t cap, int logcap) {
  gs::Table t;
  t.tab = tab;
  t.ctr = ctr;
  t.cap = (uint32_t)cap;
  t.mask = (uint32_t)(cap - 1);
  t.shift = 64 - logcap;
  t.r0 = (uint32_t)cap;
  t.vlist = nullptr;
  t.vshard_cap = 0;
  t.mark_new = 0;
  t.hflags = nullptr;
  return t;
}

struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int d) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != d) (void)hipSetDevice(d);
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// Times up to kMaxPhases consecutive phases of a call with events on its stream when `on`
// (a profiling knob of gs_testing.h); does nothing otherwise. Event i ends phase i - 1 and
// begins phase i. finish() waits for the stream and sets all `phases` words of phase_us:
// microseconds for a phase whose two events were recorded, zero for one that did not run.
struct PhaseTimer {
  static constexpr int kMaxPhases = 6;
  hipStream_t st;
  bool on;
  uint64_t* us;
  int phases;
  Event ev[kMaxPhases + 1];
  uint32_t recorded = 0;  // bit i: event i
  PhaseTimer(hipStream_t stream, bool enable, uint64_t* phase_us, int n)
      : st(stream), on(enable && n <= kMaxPhases), us(phase_us), phases(n) {
    for (int i = 0; on && i <= phases; ++i)
      if (ev[i].create(hipEventDefault) != hipSuccess) on = false;
  }
  // event i for a launcher that records it between two of its own kernels (null when off)
  hipEvent_t event(int i) {
    if (!on) return nullptr;
    recorded |= 1u << i;
    return ev[i];
  }
  void mark(int i) {
    if (on) (void)hipEventRecord(event(i), st);
  }
  void finish() {
    if (!on) return;
    (void)hipStreamSynchronize(st);
    for (int i = 0; i < phases; ++i) {
      float ms = 0;
      const bool ran = ((recorded >> i) & 3u) == 3u && hipEventElapsedTime(&ms, ev[i], ev[i + 1]) == hipSuccess;
      us[i] = ran ? (uint64_t)(ms * 1000.0f) : 0;
    }
  }
};

// What every handle owns beside its arrays: its device, its stream and the event of its
// *_wait_stream. The handles derive from it, and a base subobject is destroyed last: deleting a
// handle releases its members in reverse order of declaration, then ext_ev, then the stream,
// after every DevBuf.
struct StreamOwner {
  int device = 0;
  Stream stream;
  Event ext_ev;  // *_wait_stream: recorded on a producer's stream

  // work queued on the handle's stream from here on runs after what `producer` holds now
  int wait_stream(void* producer) {
    DeviceGuard g(device);
    hipStream_t st = static_cast<hipStream_t>(producer);
    if (st == stream) return GS_OK;
    GS_HIP(hipEventRecord(ext_ev, st));  // (stream 0 = the device's null stream)
    GS_HIP(hipStreamWaitEvent(stream, ext_ev, 0));
    return GS_OK;
  }
  int sync() {
    DeviceGuard g(device);
    GS_HIP(hipStreamSynchronize(stream));
    return GS_OK;
  }
  int get_stream(void** out) {
    if (!out) return fail(GS_ERR_INVALID, "stream is null");
    *out = stream;
    return GS_OK;
  }
};

// The bodies of a handle type's *_sync, *_get_stream and *_wait_stream (h may be null; `what`
// names the type in the message).
inline int owner_sync(StreamOwner* h, const char* what) {
  if (int rc = check_handle(h, what)) return rc;
  return h->sync();
}
inline int owner_get_stream(StreamOwner* h, const char* what, void** out) {
  if (int rc = check_handle(h, what)) return rc;
  return h->get_stream(out);
}
inline int owner_wait_stream(StreamOwner* h, const char* what, void* producer) {
  if (int rc = check_handle(h, what)) return rc;
  return h->wait_stream(producer);
}

inline int check_device_index(int device) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return fail(GS_ERR_HIP, "no HIP device available");
  if (device < 0 || device >= count) return fail(GS_ERR_INVALID, "bad device");
  return GS_OK;
}

// Handles of type H, derived from StreamOwner (h may be null).
template <class H>
int owner_destroy(H* h) {
  if (!h) return GS_OK;
  DeviceGuard g(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  delete h;  // releases every member, the stream last: device current, the stream idle
  return GS_OK;
}

// *out = a new handle on `device` (checked with check_device_index before): its stream and
// event, then init(h) with the device current, then a wait for the stream. A failure destroys
// the handle and keeps the failure's message.
template <class H, class Init>
int owner_create(H** out, int device, Init init) {
  DeviceGuard g(device);
  H* h = new H();
  h->device = device;
  const int rc = [&]() -> int {
    GS_HIP(h->stream.create());
    GS_HIP(h->ext_ev.create());
    if (int r = init(h)) return r;
    GS_HIP(hipStreamSynchronize(h->stream));
    return GS_OK;
  }();
  if (rc) {
    const std::string msg = gs_last_error();
    (void)owner_destroy(h);
    return fail(rc, msg);
  }
  *out = h;
  return GS_OK;
}

// Resource sets a call creates on first use: filled in a local, move-assigned into the handle
// only when complete, so a failed first use leaves the handle as it was.
struct Lane {  // a pipelining lane: usable wherever its stream is
  Stream st;
  Event ev;
  operator hipStream_t() const { return st; }
};
struct HostStage {  // pinned staging of large host folds, the shape of d_stage / d_wstage
  HostBuf<int64_t> e;
  HostBuf<uint8_t> w;
};
struct CombineSync {
  DevBuf<unsigned long long> cnt;  // device: exported rows (u64) + failure flag (u32 at word 1)
  Event ready, used;
};
// Text ingest (gs_fold_text, the gs_text reader; defined in gs_capi.cpp): a copy into pinned
// staging with a few threads, and the end of the chunk of at most `chunk` bytes that starts at
// off -- after its last '\n', the whole rest when it fits, 0 for a line longer than a chunk.
constexpr size_t kTextChunk = 16u << 20;  // bytes of text per parse + fold
void staged_copy(char* dst, const char* src, size_t n);
size_t chunk_end(const char* text, size_t len, size_t off, size_t chunk);
struct TextIngest {  // pinned + device text chunks, parse results, parsed edges, scratch
  HostBuf<char> h_text;
  HostBuf<uint64_t> h_res;
  Event ev[2];
  DevBuf<char> d_text;
  DevBuf<int64_t> d_src, d_dst;
  DevBuf<void> d_scratch;  // (bytes)
  gs::ParseScratch scratch;
};
struct WindowServer {
  HostBuf<gs::ServerBox> box;  // host-mapped mailbox
  DevBuf<gs::ServerBcast> bc;  // device: block 0 -> other blocks
};
}  // namespace gsi

struct gs_summary : gsi::StreamOwner {
  int kind = GS_KIND_CC;
  // table + vertex list
  gsi::DevBuf<gs::Slot> tab;  // [cap + 1]: hashed slots + the reserved slot of INT64_MIN
  uint64_t cap = 0;
  int logcap = 0;
  gsi::DevBuf<uint32_t> ctr;
  gsi::DevBuf<uint32_t> vlist;  // [kShards][vshard_cap]
  uint32_t vshard_cap = 0;
  uint32_t shard0 = 0;        // first shard of the next fold launch (rotates)
  bool vlist_ok = true;       // false once a shard of the vertex list overflowed (until reset)
  gsi::HostBuf<uint32_t> h_flags;  // [16] host-mapped mirror of CTR_ERR / CTR_OVF / CTR_VOVF (raise_flag)
  // host waits (wait_stream): completion word {seq, value} in the same host-mapped
  // allocation (bytes 32..47), written by k_signal; views, host and device
  unsigned long long* h_done = nullptr;
  unsigned long long* done_dev = nullptr;
  unsigned long long done_seq = 0;
  // capacity tracking: a host upper bound of the vertex count, refreshed without
  // host synchronisation from k_report words (ring in host-coherent memory)
  uint64_t nv_ub = 0;
  uint64_t cap_waits = 0, cap_syncs = 0;  // capacity checks that waited for reports / joined every stream
  double cap_wait_s = 0;                  // host seconds spent in those waits
  static constexpr int kRepRing = 16;
  gsi::HostBuf<unsigned long long> rep;  // [kRepRing] host-mapped
  uint64_t rep_seq = 0;
  uint64_t rep_epoch = 0;  // resets since create: tags reports (k_report) so late ones are ignored
  static constexpr int kRepEvery = 4;    // each stream reports every 4th capacity-checked chunk
  static constexpr int kRepStreams = 6;  // handle stream, 4 lanes, side stream
  int rep_skip[kRepStreams] = {};
  uint64_t rep_pending[kRepStreams] = {};  // per stream: edges of chunks queued since its last report
  uint64_t rep_pending_edges = 0;          // their sum
  uint64_t e_launched = 0;  // edges of capacity-checked folds since reset / rebuild
  uint64_t e_lost = 0;      // launched edges no report will ever claim (complete: dropped at a sync)
  uint64_t nv_exact = 0, e_exact = 0;  // an exact count and the edges complete when it was read
  // delta records (multi-GPU exchange, change emission)
  // Two delta sets: a group's own fold b records into set b % 2 while the stage of
  // exchange b - 1 reads the other set on the communication stream.
  bool track = false;
  gsi::DevBuf<int64_t> drec;  // [kDeltaSets][kShards][delta_shard_cap][3]
  uint32_t delta_shard_cap = 0;
  uint64_t delta_edges = 0;  // fold edges one delta set holds between two stages
  int dset = 0;              // the set tracked folds record into
  uint64_t delta_fill_ub[gs::kDeltaSets] = {};  // worst-case per-shard fill of each set since its last stage
  // change tracking (gs_changes.cpp)
  bool changes = false;
  bool changes_own_track = false;  // change tracking turned delta tracking on (and turns it off)
  gsi::DevBuf<uint32_t> nxt;  // [cap + 1] circular member lists
  uint64_t nxt_slots = 0;
  gsi::DevBuf<unsigned long long> chg_scratch;  // emission scratch: count, marks, big roots, staged records
  uint64_t chg_scratch_rows = 0;
  gsi::DevBuf<int64_t> chg_ov;  // gs_take_changes (host arrays): device rows before the copy
  gsi::DevBuf<int64_t> chg_ol;
  gsi::DevBuf<uint8_t> chg_op;
  uint64_t chg_ocap = 0;
  bool chg_scan_all = false;  // the next emission emits every vertex (after a rebuild)
  // staging for host folds
  gsi::DevBuf<int64_t> d_stage;   // [2][2][d_stage_chunk] (allocated by the first host fold)
  gsi::DevBuf<uint8_t> d_wstage;  // [2][d_stage_chunk]
  uint64_t d_stage_chunk = 0;  // edges per staging buffer
  gsi::HostStage hstage;       // (first use: a host fold too large for direct copies)
  gsi::Event stage_ev[2];      // after each buffer's copies
  int stage_next = 0;
  gsi::DevBuf<int64_t> d_scratch;  // small scratch (find_one)
  // combine export scratch (gs_combine source side): reused across calls
  gsi::DevBuf<int64_t> x_v;
  gsi::DevBuf<int64_t> x_l;
  gsi::DevBuf<uint8_t> x_p;
  uint64_t x_cap = 0;
  gsi::CombineSync xs;     // (first use: ensure_x)
  bool x_pending = false;  // xs.used recorded by a consumer not yet waited for
  // grouped component export (gs_export_components*) and the degree exports: the radix sort's
  // scratch, sized by the first call that needs it; co_*: device staging of the host-array form
  gsi::SortScratch sort;
  gsi::DevBuf<int64_t> co_comp;
  gsi::DevBuf<unsigned long long> co_off;
  gsi::DevBuf<int64_t> co_member;
  gsi::DevBuf<uint8_t> co_sign;
  uint64_t co_vcap = 0, co_ccap = 0;
  // degree summary (GS_KIND_DEGREE, gs_degree.cpp): endpoint occurrences folded since reset --
  // the host-side bound that keeps every 32-bit counter below 2^31
  uint64_t deg_total = 0;
  gsi::TextIngest text;  // (first use: gs_fold_text)
  // pipelined folds (gs_set_pipelining): consecutive plain device folds alternate
  // over lane streams so that fold b+1 may start while fold b drains; every other
  // entry point joins the lanes onto `stream` first (join_lanes)
  int pipe_depth = 1;
  uint64_t api_calls = 0;  // gs_* calls made on the handle (gs_group_fold_device orders its lanes after any)
  int group_lanes = 0;  // own-fold lanes of an exchange group using this summary (0: none)
  static constexpr int kLanes = 4;
  gsi::Lane lane[kLanes];  // (first use: ensure_lanes)
  gsi::Event main_ev;
  gsi::Event idle_ev;  // stream_idle: recorded and queried
  // h->stream holds waits on other streams' events queued since its last completion-kernel wait:
  // only a kernel queued behind them observes them (an event recorded there completed at once
  // in the multi-rank replay), so an idle check must not be taken then
  bool xwait = false;
  int lane_next = 0;
  int last_lane = -1;  // lane of the most recently queued fold (the label pass runs there)
  bool lanes_dirty = false;
  bool export_ctr_zero = false;  // CTR_EXPORT is zero behind the queued work (no fill before an export)
  // hot index of the plain CC fold (gs_set_hot_index; gs_hot_k.hip): two
  // buffers, one read by the folds while a build fills the other on the lane that folded the
  // sampled batch. hot_drop ends an index with the life of the table it was built from.
  int hot_cfg = 0;             // log2 ids asked for: < 0 off, 0 the default rule, > 0 forced
  uint64_t hot_first = 0;      // first build after this many edges of the table's life
  uint32_t hot_every = 0;      // then a build every this many folds
  gsi::DevBuf<gs::HotBucket> hot_buf[2];  // (first use: the first build)
  gsi::DevBuf<unsigned long long> hot_scratch;
  int hot_alloc_log2 = 0;      // log2 ids the buffers hold (0: none)
  int hot_live = -1;           // the buffer the folds read (-1: no index)
  int hot_building = -1;       // the buffer a queued build writes, adopted once hot_built has passed
  gsi::Event hot_built;
  gsi::Event hot_read[2][kLanes + 1];  // behind every stream's last fold that read the buffer (lanes, handle)
  bool hot_read_on[2] = {false, false};
  uint64_t hot_edges = 0;      // edges of the index's folds in this life of the table
  uint32_t hot_folds = 0;      // such folds since the last build was queued
  uint32_t hot_folds_r = 0;    //   ... since the last build or refresh was
  uint64_t hot_builds = 0;     // builds queued since create
  uint64_t hot_refreshes = 0;  // refreshes queued since create
  // the build's counts: the sketch (0 / < 0: the library's defaults) and the folds counted for
  // one build (0: the default; gs_testing_hot_tune), and the folds counted so far for the next
  int hot_rows = 0, hot_sketch_log2 = -1;
  uint32_t hot_sample_folds = 0;
  uint32_t hot_counted = 0;
  gsi::Event hot_zeroed;       // the scratch is zeroed: ahead of every count pass
  gsi::Event hot_count_ev[3];  // behind the count passes of the folds before the build's
  // side stream (a multi-GPU group's apply stream): folds of remote rows run there,
  // overlapping this rank's own folds; every reader joins it (join_lanes), the
  // handle's own folds do not (union commutes). Views: the group owns both and takes them
  // back (null) before it releases them
  hipStream_t side = nullptr;
  hipEvent_t side_ev = nullptr;
  bool side_dirty = false;
  // micro-batch dedup by hashing (gs_set_batch_dedup): one scratch set per stream a
  // fold may run on (handle stream, lanes, side stream): pair table + skip marks
  bool dedup = false;
  static constexpr int kDedupSets = kLanes + 2;
  gsi::DevBuf<unsigned long long> dd_tab[kDedupSets];
  gsi::DevBuf<uint8_t> dd_w[kDedupSets];
  uint64_t dd_edges[kDedupSets] = {};  // edges a set holds (its table has 2x that, a power of two)
  uint64_t dd_kept_hint = 0;
  // resident window server (gs_set_window_server): one persistent launch serves the
  // latency path's windows; every other entry point stops it first (join_lanes)
  bool srv_on = false, srv_running = false;
  int srv_fits = -1;                     // all kServerBlocks workgroups co-resident (-1: not yet checked)
  gsi::WindowServer srv;                 // (first use: gs_set_window_server)
  unsigned long long srv_seq = 0;        // last window posted and completed
  uint64_t srv_launches = 0, srv_windows = 0;
  // profiling
  bool profiling = false;
  gsi::SpanTimer spans;  // one span per launch, its id the kernel's KID_*
  uint64_t launches[gsi::KID_N] = {0, 0, 0, 0};
  double total_ms[gsi::KID_N] = {0, 0, 0, 0};

  gs::Table table() const {
    gs::Table t = gsi::make_table(tab, ctr, cap, logcap);
    t.vlist = vlist;
    t.vshard_cap = vshard_cap;
    t.mark_new = changes ? 1 : 0;
    t.hflags = h_flags.dev();
    return t;
  }
  gs::Delta delta(int set = -1) const {
    if (set < 0) set = dset;
    gs::Delta D;
    D.drec = drec ? drec + (size_t)set * gs::kShards * delta_shard_cap * 3 : nullptr;
    D.shard_cap = delta_shard_cap;
    D.dctr = (uint32_t)(gs::CTR_DELTA + set * gs::kShards);
    return D;
  }
};

namespace gsi {

// Where a fold's rows come from (defaults: plain edge arrays on the handle stream).
struct FoldSource {
  uint32_t rows = 0;  // > 0: gathered exchange buffer, world blocks of `rows` rows
  int skip_rank = -1;
  const unsigned long long* counts = nullptr;  // device: live rows per block (| kFailBit)
  uint64_t units = 0;  // exchange layout: rows that may add vertices (capacity charge)
  const unsigned long long* n_dev = nullptr;   // device element count (<= n)
  const uint32_t* fail_in = nullptr;           // device failure flag of a combined summary
  bool on_side = false;  // launch on h->side (a group's apply stream) instead of h->stream
  bool allow_pipe = false;
  // a TRACKED fold may pipeline too: its caller takes the delta set only after joining the
  // lanes (the partitioned group's windows: records go to one set through sharded atomics)
  bool pipe_tracked = false;
  int lane = -1;         // >= 0: launch on this pipelining lane (a group's own tracked fold)
  // fused window take (gs_fold_take_device): one tracked launch that also writes the
  // rows, the count and the completion word {seq, vertices, rows}
  int64_t* take_out = nullptr;
  uint64_t take_cap = 0;
  unsigned long long* take_count = nullptr;
  unsigned long long* take_seq = nullptr;  // out: the completion sequence number, drawn at launch
};

int fold_device_impl(gs_summary* h, const int64_t* src, const int64_t* dst, const uint8_t* w, size_t n,
                     size_t stride, size_t w_stride, bool track, bool check_cap = true,
                     const FoldSource& fs = FoldSource());
int join_lanes(gs_summary* h);
bool side_ok(const gs_summary* h);
int flush_reports(gs_summary* h);  // standalone capacity reports of every stream's unclaimed chunks
int ensure_lanes(gs_summary* h, int n);  // create lane streams 0..n-1 on first use
int read_nv(gs_summary* h, uint64_t* nv);
// wait until every operation queued on h->stream (or `st`) so far has completed; *value
// (optional) = the sum of nvals device u32 counters vals[i * stride], read in the same
// round trip (and zeroed behind the read with `clear`)
int wait_stream(gs_summary* h, const uint32_t* vals = nullptr, uint64_t* value = nullptr, int nvals = 1,
                int stride = 0, bool clear = false, hipStream_t st = nullptr, const uint32_t* flag = nullptr);
int check_device_flags(gs_summary* h);
int check_flags_now(gs_summary* h);
int done_value_read(gs_summary* h, int i, unsigned long long seq, uint64_t* out);  // tagged completion value
int wait_done(gs_summary* h, unsigned long long seq, hipStream_t st = nullptr);  // spin on the completion word (h->stream / st)  // after a wait: the host-mapped flags only
int export_device_impl(gs_summary* h, int64_t* v, int64_t* l, uint8_t* p, size_t cap, size_t* n, int part = 0,
                       int nparts = 1);
// stage every pending delta record into out (first cap rows, `width` int64 each) and
// the count word into *count_out (device); the delta list is emptied
int stage_delta(gs_summary* h, int64_t* out, uint64_t cap, int width, unsigned long long* count_out, bool with_fail,
                hipStream_t st = nullptr, int set = -1);
int ensure_delta_list(gs_summary* h, uint64_t edges);
bool use_vertex_list(gs_summary* h, uint64_t nv_bound);
// gs_changes.cpp, after a reset (mode 0: vertex-list reset, 1: full table init) or a
// rebuild into a new table (mode 2)
int change_tracking_reset(gs_summary* h, int mode);
// gs_capi.cpp internals the degree summary (gs_degree.cpp) shares
int x_scratch(gs_summary* h, uint64_t rows);     // combine scratch x_v / x_l / x_p of >= rows rows, free to write
void exact_count(gs_summary* h, uint64_t nv);    // an exact vertex count read with every queued fold complete
int rebuild_table(gs_summary* h, uint64_t cap);  // free the table, allocate and initialise one of cap slots
int comp_staging(gs_summary* h, uint64_t nv, uint64_t nc);  // co_member / co_sign (nv), co_comp / co_off (nc)
int dev_stage(gs_summary* h, size_t edges);      // device staging of host folds (d_stage, d_wstage)
// gs_degree.cpp, called by the shared entry points of gs_capi.cpp on a degree summary
int degree_grow(gs_summary* h, uint64_t new_cap);
int degree_combine(gs_summary* dst, gs_summary* src);
int degree_serialize(gs_summary* h, void* buf, size_t cap, size_t* len);
int degree_deserialize(gs_summary* h, const void* buf, uint64_t n, uint32_t total);

}  // namespace gsi
