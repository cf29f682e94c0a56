// gelly_streaming.hpp -- C++ host mirror of gelly-streaming's summary-aggregation API,
// backed by the MI355X C ABI (include/gs_summary.h).
//
// The reference is Java 8 / Flink 1.8 (pom.xml:15-17) and no JVM exists in this
// image, so the host side above the C ABI is C++ with the reference's names,
// argument meanings and error behaviour (exceptions where Java throws):
//
//   EdgesFold<K,EV,T>           EdgesFold.java:33-47
//   SummaryAggregation          SummaryAggregation.java:36-136 (fold/combine/transform/
//                               initial value/transient contract + Merger)
//   SummaryBulkAggregation      SummaryBulkAggregation.java:44-131 (run(): partition tag ->
//                               keyed window fold -> all-window reduce -> Merger)
//   SimpleEdgeStream::aggregate SimpleEdgeStream.java:100-102
//   SimpleEdgeStream::slice     SimpleEdgeStream.java:135-167
//   SimpleEdgeStream::distinct  SimpleEdgeStream.java:301-323 (the pinned behaviour: first-seen pairs)
//   SimpleEdgeStream::getVertices SimpleEdgeStream.java:116-121, 181-202
//   SnapshotStream              SnapshotStream.java:61-131 (reduceOnEdges / foldNeighbors /
//                               applyOnNeighbors over a GPU-resident window slice)
//   DisjointSet                 summaries/DisjointSet.java:25-151  (GPU-resident forest)
//   Candidates                  summaries/Candidates.java:27-196   (GPU-resident signed forest)
//   ConnectedComponents         library/ConnectedComponents.java:41-134
//   BipartitenessCheck          library/BipartitenessCheck.java:37-133
//   AdjacencyListGraph          summaries/AdjacencyListGraph.java:27-140 (GPU-resident adjacency)
//   Spanner                     library/Spanner.java:40-118
//   BroadcastTriangleCount      example/BroadcastTriangleCount.java:41-174 (S sampler instances on the GPU)
//
// Summaries are held by std::shared_ptr (Java object references). A GPU-backed
// summary buffers its per-edge callbacks (union / merge of a one-edge candidate)
// and flushes them to the device as one micro-batch on any read, combine or
// serialization -- the drop-in design of INTEGRATION.md.
#pragma once

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstring>
#include <functional>
#include <limits>
#include <map>
#include <set>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "gs_ingest.h"
#include "gs_summary.h"

namespace gelly {

struct NullValue {};

class GsException : public std::runtime_error {
 public:
  GsException(int code, const std::string& what) : std::runtime_error(what), code_(code) {}
  int code() const { return code_; }

 private:
  int code_;
};

inline void gs_check(int rc) {
  if (rc != GS_OK) throw GsException(rc, std::string("gs: ") + gs_last_error());
}

// Edge<K, EV> is a Tuple3 (f0 = source, f1 = target, f2 = value).
template <typename K, typename EV>
struct Edge {
  K f0;
  K f1;
  EV f2;
  K getSource() const { return f0; }
  K getTarget() const { return f1; }
  EV getValue() const { return f2; }
};

// Vertex<K, VV> is a Tuple2 (f0 = id, f1 = value).
template <typename K, typename VV>
struct Vertex {
  K f0;
  VV f1;
  K getId() const { return f0; }
  VV getValue() const { return f1; }
};

// EdgesFold.java:47 -- T foldEdges(T accum, K vertexID, K neighborID, EV edgeValue)
template <typename K, typename EV, typename T>
struct EdgesFold {
  virtual ~EdgesFold() = default;
  virtual T foldEdges(T accum, K vertexID, K neighborID, EV edgeValue) = 0;
};

// Flink ReduceFunction<S> / MapFunction<S, T>
template <typename S>
struct ReduceFunction {
  virtual ~ReduceFunction() = default;
  virtual S reduce(S value1, S value2) = 0;
};
template <typename S, typename T>
struct MapFunction {
  virtual ~MapFunction() = default;
  virtual T map(S value) = 0;
};

// --------------------------------------------------------------------------
// Handle pool. Flink copies the summary's initial value for every (partition,
// window) fold (SummaryBulkAggregation.java:80, FoldingState) and drops the partial
// after the all-window reduce; creating a GPU summary each time would cost a table
// allocation and initialisation per window. Released handles are reset (O(touched
// vertices) on the device, asynchronous) and handed to the next summary of the same
// kind and device: one whose table size class fits (up to kClassSlack classes larger),
// else any larger pooled one -- reusing HBM that is already held costs nothing against
// the budget, a create does (the per-window copy of the EMPTY initial value
// asks for the smallest class, and grown pooled tables must still serve it).
//
// HBM budget (the Java HandlePool's model). The budget is
// checked against the library's own count of the device memory every live summary holds
// (gs_hbm_bytes: tables, vertex lists, staging, scratch), so a table that grew inside a
// fold or combine while handed out -- the Merger's running summary -- counts at once, not
// at its release. A create of gs_create_bytes(hint) that would pass the budget first runs
// set_budget's `collect` hook (System.gc() + System.runFinalization(): summaries a Flink
// job dropped without release() come back through their finalizers), then destroys pooled
// handles until it fits. Tables also grow in place (a reused pooled table inside the window's
// fold), so any acquire that finds the device past the budget collects first, too, and trims
// the pool back to it. The total then stays within the budget plus the table being created,
// unless live summaries alone need more.
// --------------------------------------------------------------------------
class HandlePool {
 public:
  static constexpr int kClassSlack = 2;
  static constexpr size_t kMaxFree = 64;
  static HandlePool& instance() {
    static HandlePool p;
    return p;
  }
  // gs_create's table for a capacity hint: 4 slots per expected vertex, a power of two, >= 1024
  static uint64_t slots_for(uint64_t hint) {
    const uint64_t want = std::max<uint64_t>(4 * std::max<uint64_t>(hint, 1), 1024);
    uint64_t s = 1;
    while (s < want) s <<= 1;
    return s;
  }
  static int size_class(uint64_t slots) {
    int c = 0;
    while ((2ull << c) <= slots) ++c;
    return c;
  }
  // the library's count of device memory held by live summaries on `device`
  static uint64_t device_bytes(int device) {
    uint64_t b = 0;
    gs_check(gs_hbm_bytes(device, &b));
    return b;
  }
  // budget of the device's summary HBM (0: none) and the finalization hook it runs
  void set_budget(uint64_t bytes, std::function<void()> collect) {
    budget_ = bytes;
    collect_ = std::move(collect);
  }
  gs_handle acquire(int kind, int device, uint64_t capacity_hint) {
    const int cls = size_class(slots_for(capacity_hint));
    // tables grow in place inside folds and combines, pooled or handed out: a device already
    // past the budget finalizes the dropped summaries first even when a pooled handle would
    // serve this request, takes any larger pooled table, and gives up pooled ones beyond it
    const bool over = budget_ && device_bytes(device) > budget_;
    if (over) collect();
    if (gs_handle h = take(kind, device, cls, over)) {
      if (over) evict_for(device, 0);
      return h;
    }
    uint64_t need = 0;
    gs_check(gs_create_bytes(kind, capacity_hint, &need));
    if (budget_ && device_bytes(device) + need > budget_) {
      if (!over) {
        collect();  // the dropped summaries' destructors release into this pool
        if (gs_handle h = take(kind, device, cls, true)) return h;
      }
      evict_for(device, need);  // still over: pooled handles (largest first) make room
    }
    gs_handle h = nullptr;
    gs_check(gs_create(&h, device, kind, capacity_hint));
    ++created_;
    live_.insert(h);
    note(device);
    return h;
  }
  void release(gs_handle h, int kind, int device) {
    uint64_t slots = 0;
    // the value AND the configuration (tracking, pipelining, profiling) of a fresh handle;
    // a table keeps a grown capacity across resets: pool it by its real size
    if (gs_reset_config(h) != GS_OK || gs_table_capacity(h, &slots) != GS_OK) {  // a broken handle is not pooled
      live_.erase(h);
      gs_destroy(h);
      return;
    }
    note(device);
    if (nfree_ < kMaxFree) {
      free_[{kind, device, size_class(slots)}].push_back(h);
      ++nfree_;
    } else {
      live_.erase(h);
      gs_destroy(h);
    }
  }
  size_t created() const { return created_; }
  size_t reused() const { return reused_; }
  size_t reused_larger() const { return reused_larger_; }
  size_t collections() const { return collections_; }
  uint64_t peak_total_bytes() const { return peak_total_; }  // gs_hbm_bytes seen at acquires / releases
  size_t live_handles() const { return live_.size(); }       // handed out + pooled
  ~HandlePool() {
    for (auto& kv : free_)
      for (gs_handle h : kv.second) gs_destroy(h);
  }

 private:
  // a pooled handle of class cls .. cls + kClassSlack, or (any_larger) of any larger class
  gs_handle take(int kind, int device, int cls, bool any_larger) {
    for (auto it = free_.lower_bound({kind, device, cls}); it != free_.end(); ++it) {
      const auto& k = it->first;
      if (std::get<0>(k) != kind || std::get<1>(k) != device) break;
      const bool near = std::get<2>(k) <= cls + kClassSlack;
      if (!near && !any_larger) break;
      if (it->second.empty()) continue;
      gs_handle h = it->second.back();
      it->second.pop_back();
      --nfree_;
      ++reused_;
      if (!near) ++reused_larger_;
      return h;
    }
    return nullptr;
  }
  void note(int device) { peak_total_ = std::max(peak_total_, device_bytes(device)); }
  void collect() {
    if (!collect_) return;
    ++collections_;
    collect_();
  }
  // destroy pooled handles, largest first, until a create of `need` bytes fits the budget
  void evict_for(int device, uint64_t need) {
    for (auto it = free_.rbegin(); it != free_.rend() && device_bytes(device) + need > budget_; ++it)
      while (!it->second.empty() && device_bytes(device) + need > budget_) {
        gs_handle f = it->second.back();
        it->second.pop_back();
        --nfree_;
        live_.erase(f);
        gs_destroy(f);
      }
  }
  std::map<std::tuple<int, int, int>, std::vector<gs_handle>> free_;
  std::set<gs_handle> live_;
  size_t nfree_ = 0, created_ = 0, reused_ = 0, reused_larger_ = 0, collections_ = 0;
  uint64_t budget_ = 0, peak_total_ = 0;
  std::function<void()> collect_;
};

// --------------------------------------------------------------------------
// GPU-resident summaries
// --------------------------------------------------------------------------
//
// The handle is taken from the pool at first use, not at construction: a summary built
// where no GPU work happens (the Flink job client builds the operator's initial value,
// ConnectedComponents.java:52-54, then ships it to the TaskManagers by Java
// serialization) holds no device state. writeObject / readObject model that Java
// serialization (GpuDisjointSet / GpuCandidates writeObject + readObject): a summary that
// was never used travels as a one-byte marker, any other as its gs_serialize image, which
// the copy applies on its own first use (SummaryAggregation.Merger's initialVal and
// summary fields, SummaryAggregation.java:95-103).
class GpuSummary {
 public:
  GpuSummary(int kind, int device, uint64_t capacity_hint, size_t flush_edges)
      : kind_(kind), device_(device), hint_(capacity_hint), flush_edges_(flush_edges) {}
  virtual ~GpuSummary() { release(); }
  GpuSummary(const GpuSummary&) = delete;
  GpuSummary& operator=(const GpuSummary&) = delete;

  // push one buffered edge (flushes a full micro-batch); the buffers are sized for
  // a whole micro-batch on first use, so the per-edge path is two stores and a compare
  void push(int64_t u, int64_t v) {
    if (!src_) {
      src_.reset(new int64_t[flush_edges_]);
      dst_.reset(new int64_t[flush_edges_]);
    }
    src_[n_] = u;
    dst_[n_] = v;
    if (++n_ == flush_edges_) flush();
  }
  void flush() {
    if (n_ == 0) return;
    gs_handle h = ensure();
    const auto t0 = std::chrono::steady_clock::now();
    gs_check(gs_fold(h, src_.get(), dst_.get(), n_));
    flush_seconds() += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    n_ = 0;
  }
  // the device handle, taken at first use; a pending image (readObject) or an initial
  // failed verdict (Candidates(false)) is applied to it then
  gs_handle ensure() {
    if (h_) return h_;
    // the table for the size asked for (size_for), else the pending image's vertex count
    // (its header: u32 magic, kind, ok, 0, u64 n), else the constructor's hint
    uint64_t hint = sized_ ? sized_ : hint_;
    if (!sized_ && image_.size() >= 24) {
      uint64_t n = 0;
      std::memcpy(&n, image_.data() + 16, 8);
      if (n) hint = n;
    }
    h_ = HandlePool::instance().acquire(kind_, device_, hint);
    if (!image_.empty()) {
      std::vector<uint8_t> img;
      img.swap(image_);
      gs_check(gs_deserialize(h_, img.data(), img.size()));
    } else if (failed_initially_) {
      // :194-196 fail() == new Candidates(false): the image of a failed, empty summary
      // (header only: magic 'GSS1', kind, ok = 0, n = 0)
      std::vector<uint8_t> img(24, 0);
      const uint32_t hdr[4] = {0x31535347u, (uint32_t)kind_, 0u, 0u};
      std::memcpy(img.data(), hdr, 16);
      gs_check(gs_deserialize(h_, img.data(), img.size()));
    }
    return h_;
  }
  bool acquired() const { return h_ != nullptr; }
  // size the handle taken at first use for about `vertices` vertices (GpuSummary.sizeFor: a
  // copy asks for its source's count); no effect once a handle is held
  void size_for(uint64_t vertices) {
    if (!h_) sized_ = std::max<uint64_t>(vertices, 1);
  }
  // back to the pool (the glue's explicit release of a summary the combine dropped); the
  // object reads as a fresh initial value afterwards
  void release() {
    n_ = 0;
    sized_ = 0;
    image_.clear();
    if (h_) HandlePool::instance().release(h_, kind_, device_);
    h_ = nullptr;
  }
  // Java serialization of the summary object: [0] 1 = an image follows, [1] failed
  // initially (Candidates(false)), then the gs_serialize image
  std::vector<uint8_t> writeObject() {
    std::vector<uint8_t> out = {0, (uint8_t)(failed_initially_ ? 1 : 0)};
    if (!h_ && image_.empty() && n_ == 0) return out;  // never used: no device state to ship
    const std::vector<uint8_t> img = h_ || n_ ? serialize() : image_;
    out[0] = 1;
    out.insert(out.end(), img.begin(), img.end());
    return out;
  }
  void readObjectInto(const std::vector<uint8_t>& bytes) {  // (on a fresh object)
    if (bytes.size() < 2) throw GsException(GS_ERR_INVALID, "readObject: truncated stream");
    release();
    failed_initially_ = bytes[1] != 0;
    if (bytes[0]) image_.assign(bytes.begin() + 2, bytes.end());
  }
  // host seconds spent in gs_fold (micro-batch flushes), process-wide (dropin_bench)
  static double& flush_seconds() {
    static double s = 0;
    return s;
  }
  gs_handle handle() {
    flush();
    return ensure();
  }
  size_t size() {
    uint64_t n = 0;
    gs_check(gs_num_vertices(handle(), &n));
    return (size_t)n;
  }
  void reset() {
    n_ = 0;
    image_.clear();
    gs_check(gs_reset(ensure()));
  }
  // all (vertex, canonical label, parity) rows, sorted by vertex
  struct Row {
    int64_t v, label;
    uint8_t parity;
  };
  std::vector<Row> rows() {
    gs_handle h = handle();
    uint64_t n = 0;
    gs_check(gs_num_vertices(h, &n));
    std::vector<int64_t> v(n), l(n);
    std::vector<uint8_t> s(n);
    size_t got = 0;
    if (kind_ == GS_KIND_SIGNED) {
      int ok = 1;
      gs_check(gs_bip_status(h, &ok));
      if (!ok) return {};
      gs_check(gs_export_colouring(h, l.data(), v.data(), s.data(), n, &got));
    } else {
      gs_check(gs_export_labels(h, v.data(), l.data(), n, &got));
    }
    std::vector<Row> r(got);
    for (size_t i = 0; i < got; ++i) r[i] = {v[i], l[i], (uint8_t)(kind_ == GS_KIND_SIGNED ? s[i] : 0)};
    std::sort(r.begin(), r.end(), [](const Row& a, const Row& b) { return a.v < b.v; });
    return r;
  }
  std::vector<uint8_t> serialize() {
    size_t len = 0;
    gs_check(gs_serialize(handle(), nullptr, 0, &len));
    std::vector<uint8_t> buf(len);
    gs_check(gs_serialize(h_, buf.data(), len, &len));
    buf.resize(len);
    return buf;
  }
  void deserialize(const std::vector<uint8_t>& buf) {
    n_ = 0;
    image_.clear();
    gs_check(gs_deserialize(ensure(), buf.data(), buf.size()));
  }
  int device() const { return device_; }

 protected:
  int kind_;
  int device_;
  uint64_t hint_;
  uint64_t sized_ = 0;  // size_for(): vertices of the first handle (0: hint_ / the image's count)
  size_t flush_edges_;
  gs_handle h_ = nullptr;
  std::unique_ptr<int64_t[]> src_, dst_;  // [flush_edges_] each, allocated on first push
  size_t n_ = 0;                          // buffered edges
  std::vector<uint8_t> image_;            // readObject: applied at first use
  bool failed_initially_ = false;         // Candidates(false), applied at first use
};

// DisjointSet<Long> (DisjointSet.java:25-151) over the GPU forest. find() returns
// the canonical representative (minimum id of the component): the reference
// returns an arbitrary member as root (:66-80); every caller only compares roots
// for equality or prints components, which the canonical choice preserves.
class DisjointSet : public GpuSummary {
 public:
  explicit DisjointSet(int device = 0, uint64_t capacity_hint = 1 << 16, size_t flush_edges = 1 << 20)
      : GpuSummary(GS_KIND_CC, device, capacity_hint, flush_edges) {}

  void makeSet(int64_t e) { push(e, e); }               // :53-56
  void union_(int64_t e1, int64_t e2) { push(e1, e2); }  // :92-118 ("union" is a C++ keyword)
  std::optional<int64_t> find(int64_t e) {               // :66-80 (null -> nullopt)
    int64_t label = 0;
    int found = 0;
    gs_check(gs_find(handle(), e, &label, &found));
    if (!found) return std::nullopt;
    return label;
  }
  void merge(DisjointSet& other) {  // :127-131
    if (&other == this) return;
    gs_check(gs_combine(handle(), other.handle()));
  }
  static std::shared_ptr<DisjointSet> readObject(const std::vector<uint8_t>& bytes, int device = 0,
                                                 uint64_t capacity_hint = 1 << 16) {
    auto d = std::make_shared<DisjointSet>(device, capacity_hint);
    d->readObjectInto(bytes);
    return d;
  }
  // getMatches() (:44-46) as (vertex, representative) pairs
  std::vector<std::pair<int64_t, int64_t>> getMatches() {
    std::vector<std::pair<int64_t, int64_t>> m;
    for (const Row& r : rows()) m.push_back({r.v, r.label});
    return m;
  }
  // toString() (:134-150): "{root=[members], ...}", components keyed by their
  // minimum id, members ascending (the reference prints HashMap order).
  std::string toString() {
    std::map<int64_t, std::vector<int64_t>> comps;
    for (const Row& r : rows()) comps[r.label].push_back(r.v);
    std::string s = "{";
    bool first = true;
    for (auto& kv : comps) {
      if (!first) s += ", ";
      first = false;
      s += std::to_string(kv.first) + "=[";
      for (size_t i = 0; i < kv.second.size(); ++i) s += (i ? ", " : "") + std::to_string(kv.second[i]);
      s += "]";
    }
    return s + "}";
  }
};

// Candidates (Candidates.java:27-196) over the GPU signed forest. A one-edge
// candidate (BipartitenessCheck.edgeToCandidate, :54-61) is a host-only value
// that merge() buffers; merging two GPU summaries runs gs_combine.
class Candidates : public GpuSummary {
 public:
  struct EdgeCandidate {  // {min(u,v): {min: +, max: -}}
    int64_t u, v;
  };
  explicit Candidates(bool success = true, int device = 0, uint64_t capacity_hint = 1 << 16,
                      size_t flush_edges = 1 << 20)
      : GpuSummary(GS_KIND_SIGNED, device, capacity_hint, flush_edges) {
    failed_initially_ = !success;  // applied when the handle is taken
  }
  static std::shared_ptr<Candidates> readObject(const std::vector<uint8_t>& bytes, int device = 0,
                                                uint64_t capacity_hint = 1 << 16) {
    auto c = std::make_shared<Candidates>(true, device, capacity_hint);
    c->readObjectInto(bytes);
    return c;
  }
  bool getSuccess() {  // :44-46
    int ok = 1;
    gs_check(gs_bip_status(handle(), &ok));
    return ok != 0;
  }
  // :77-139: merge(input) with input = one edge (the fold) ...
  Candidates& merge(const EdgeCandidate& e) {
    push(e.u, e.v);
    return *this;
  }
  // ... or another summary (the combine); the verdict is the AND.
  Candidates& merge(Candidates& input) {
    if (&input != this) gs_check(gs_combine(handle(), input.handle()));
    return *this;
  }
  // getMap() (:48-50): component (min id) -> {vertex -> sign}
  std::map<int64_t, std::map<int64_t, bool>> getMap() {
    std::map<int64_t, std::map<int64_t, bool>> m;
    for (const Row& r : rows()) m[r.label][r.v] = r.parity != 0;
    return m;
  }
  // Tuple2.toString(): "(true,{1={1=(1,true), 2=(2,false)}, ...})" / "(false,{})"
  std::string toString() {
    const bool ok = getSuccess();
    std::string s = std::string("(") + (ok ? "true" : "false") + ",{";
    if (ok) {
      bool first = true;
      for (auto& c : getMap()) {
        if (!first) s += ", ";
        first = false;
        s += std::to_string(c.first) + "={";
        bool f2 = true;
        for (auto& v : c.second) {
          if (!f2) s += ", ";
          f2 = false;
          s += std::to_string(v.first) + "=(" + std::to_string(v.first) + "," + (v.second ? "true" : "false") + ")";
        }
        s += "}";
      }
    }
    return s + "})";
  }
};

// --------------------------------------------------------------------------
// Operators
// --------------------------------------------------------------------------
// SummaryAggregation<K, EV, S, T> (SummaryAggregation.java:36-91)
template <typename K, typename EV, typename S, typename T>
class SummaryAggregation {
 public:
  using Fold = EdgesFold<K, EV, S>;
  using Combine = ReduceFunction<S>;
  using Transform = MapFunction<S, T>;
  using Factory = std::function<S()>;  // the initial value (Flink copies it per window)

  SummaryAggregation(std::shared_ptr<Fold> updateFun, std::shared_ptr<Combine> combineFun,
                     std::shared_ptr<Transform> transform, Factory initialValue, bool transientState)
      : updateFun_(std::move(updateFun)),
        combineFun_(std::move(combineFun)),
        transform_(std::move(transform)),
        initialValue_(std::move(initialValue)),
        transientState_(transientState) {}
  virtual ~SummaryAggregation() = default;

  std::shared_ptr<Combine> getCombineFun() const { return combineFun_; }
  std::shared_ptr<Fold> getUpdateFun() const { return updateFun_; }
  std::shared_ptr<Transform> getTransform() const { return transform_; }
  bool isTransientState() const { return transientState_; }
  S getInitialValue() const { return initialValue_(); }

  // Merger (SummaryAggregation.java:93-136): running combine at parallelism 1.
  class Merger {
   public:
    Merger(Factory initialVal, std::shared_ptr<Combine> combiner, bool transientState)
        : initialVal_(std::move(initialVal)), combiner_(std::move(combiner)), transientState_(transientState) {
      summary_ = initialVal_();
    }
    // flatMap (:107-119): summary = combine.reduce(s, summary); emit; reset if transient
    S flatMap(S s) {
      if (!combiner_) return s;
      summary_ = combiner_->reduce(s, summary_);
      S out = summary_;
      if (transientState_) summary_ = initialVal_();
      return out;
    }
    // snapshotState / restoreState (:127-135) through the summary's serializer
    S snapshotState() { return summary_; }
    void restoreState(S s) { summary_ = std::move(s); }

   private:
    Factory initialVal_;
    std::shared_ptr<Combine> combiner_;
    bool transientState_;
    S summary_;
  };

 protected:
  std::shared_ptr<Fold> updateFun_;
  std::shared_ptr<Combine> combineFun_;
  std::shared_ptr<Transform> transform_;
  Factory initialValue_;
  bool transientState_;
};

// A bounded, timestamped edge stream with a source parallelism: the stand-in for
// DataStream<Edge<K, EV>> (SimpleEdgeStream.java:69-90). Edges are dealt to the p
// fold subtasks round-robin (a rebalanced parallelism-1 source).
template <typename K, typename EV>
struct EdgeStream {
  std::vector<Edge<K, EV>> edges;
  std::vector<int64_t> timestamps;  // event/ingestion time in ms (empty: all 0)
  int parallelism = 1;
};

// SummaryBulkAggregation (SummaryBulkAggregation.java:44-131)
template <typename K, typename EV, typename S, typename T>
class SummaryBulkAggregation : public SummaryAggregation<K, EV, S, T> {
  using Base = SummaryAggregation<K, EV, S, T>;

 public:
  SummaryBulkAggregation(std::shared_ptr<typename Base::Fold> updateFun,
                         std::shared_ptr<typename Base::Combine> combineFun,
                         std::shared_ptr<typename Base::Transform> transformFun, typename Base::Factory initialVal,
                         int64_t timeMillis, bool transientState)
      : Base(std::move(updateFun), std::move(combineFun), std::move(transformFun), std::move(initialVal),
             transientState),
        timeMillis_(timeMillis) {}
  SummaryBulkAggregation(std::shared_ptr<typename Base::Fold> updateFun,
                         std::shared_ptr<typename Base::Combine> combineFun, typename Base::Factory initialVal,
                         int64_t timeMillis, bool transientState)
      : SummaryBulkAggregation(std::move(updateFun), std::move(combineFun), nullptr, std::move(initialVal),
                               timeMillis, transientState) {}

  // run (:68-90): PartitionMapper -> keyBy(partition).timeWindow(t).fold(initial,
  // PartialAgg) -> timeWindowAll(t).reduce(combine) -> Merger -> (transform).
  // Every emission (one per window that holds edges) is handed to `sink` at
  // emission time (the addSink(...) of the reference tests); the running summary
  // object is reused across windows exactly like the Merger's.
  using Sink = std::function<void(const T&)>;
  void run(const EdgeStream<K, EV>& stream, const Sink& sink) {
    const size_t n = stream.edges.size();
    const int p = std::max(1, stream.parallelism);
    typename Base::Merger merger(this->initialValue_, this->combineFun_, this->transientState_);
    size_t i = 0;
    while (i < n) {
      const int64_t w = window_of(stream, i);
      size_t j = i;
      if (stream.timestamps.empty() || timeMillis_ <= 0) {
        j = n;  // one window
      } else {  // the edges with ts / timeMillis_ == w: compared against the window's
                // bounds, not divided one by one (a 64-bit division per edge was ~5 ns)
        int64_t lo, hi;
        window_bounds(w, &lo, &hi);
        const int64_t* ts = stream.timestamps.data();
        while (j < n && ts[j] >= lo && ts[j] <= hi) ++j;
      }
      std::vector<S> partial(p);  // per-(partition, window) fold state
      const auto tf = std::chrono::steady_clock::now();
      int part = (int)(i % (size_t)p);  // PartitionMapper.map (:103-105): edge k -> k mod p
      for (size_t k = i; k < j; ++k, part = (part + 1 == p) ? 0 : part + 1) {
        if (!partial[part]) partial[part] = this->getInitialValue();
        const Edge<K, EV>& e = stream.edges[k];
        // the accumulator is handed over and returned (Java passes the reference):
        // moved, so no reference-count traffic per edge
        partial[part] =
            this->updateFun_->foldEdges(std::move(partial[part]), e.getSource(), e.getTarget(), e.getValue());
      }
      const auto tc = std::chrono::steady_clock::now();
      S acc{};
      for (int q = 0; q < p; ++q) {  // timeWindowAll reduce, arrival order = partition order
        if (!partial[q]) continue;
        acc = acc ? this->combineFun_->reduce(acc, partial[q]) : partial[q];
      }
      S emitted = merger.flatMap(acc);
      sink(emit(emitted));
      run_seconds()[0] += std::chrono::duration<double>(tc - tf).count();
      run_seconds()[1] += std::chrono::duration<double>(std::chrono::steady_clock::now() - tc).count();
      i = j;
    }
  }
  // host seconds in run(): [0] per-edge folds (incl. flushes), [1] reduce + Merger + sink
  static double* run_seconds() {
    static double t[2] = {0, 0};
    return t;
  }
  // Convenience: collect the emissions (references to live summaries; read them
  // before the next window mutates the running summary, or use the sink form).
  std::vector<T> run(const EdgeStream<K, EV>& stream) {
    std::vector<T> out;
    run(stream, [&out](const T& x) { out.push_back(x); });
    return out;
  }

 private:
  int64_t window_of(const EdgeStream<K, EV>& s, size_t i) const {
    const int64_t ts = s.timestamps.empty() ? 0 : s.timestamps[i];
    return timeMillis_ > 0 ? ts / timeMillis_ : 0;
  }
  // [lo, hi]: every ts with ts / timeMillis_ == w (C++ truncating division), saturated
  void window_bounds(int64_t w, int64_t* lo, int64_t* hi) const {
    const int64_t tm = timeMillis_;
    const int64_t base = w * tm;  // |base| <= |ts| of an existing edge: no overflow
    const int64_t kMax = std::numeric_limits<int64_t>::max(), kMin = std::numeric_limits<int64_t>::min();
    if (w > 0) {
      *lo = base;
      *hi = base > kMax - (tm - 1) ? kMax : base + (tm - 1);
    } else if (w < 0) {
      *lo = base < kMin + (tm - 1) ? kMin : base - (tm - 1);
      *hi = base;
    } else {
      *lo = -(tm - 1);
      *hi = tm - 1;
    }
  }
  T emit(S s) {
    if constexpr (std::is_same<S, T>::value) {
      if (!this->transform_) return s;
    }
    return this->transform_->map(s);
  }
  int64_t timeMillis_;
};

// EdgeDirection (flink-gelly): which endpoint keys an edge in a slice
enum class EdgeDirection { IN, OUT, ALL };

// SnapshotStream (SnapshotStream.java:61-131): the per-vertex neighbourhoods of every window
// of a sliced edge stream, read through a slice handle (gs_summary.h, the gs_slice_* section).
// Windows are cut on the host: consecutive edges whose timestamps share ts / timeMillis (the
// rule of SummaryBulkAggregation::window_bounds); no timestamps or timeMillis <= 0 is one
// window. Every method returns its emissions window after window, vertices ascending inside a
// window (the reference's order inside a window is unspecified). reduceOnEdges(gs_slice_op)
// reduces on the device; the forms that take a function run it on the host over the window's
// CSR, a vertex's entries in arrival order.
template <typename K, typename EV>
class SnapshotStream {
  static_assert(std::is_same<K, int64_t>::value, "slices are built for 64-bit integer keys");
  static_assert(std::is_same<EV, int64_t>::value || std::is_same<EV, NullValue>::value,
                "slices are built for 64-bit integer edge values and NullValue");
  static constexpr bool kHasValue = std::is_same<EV, int64_t>::value;
  template <typename F>
  struct NonDeduced {  // T of foldNeighbors comes from `initial` alone, so a lambda converts
    using type = F;
  };

 public:
  SnapshotStream(const EdgeStream<K, EV>* edges, int64_t timeMillis, EdgeDirection direction, int device)
      : edges_(edges), timeMillis_(timeMillis), dir_(direction), device_(device) {}

  // reduceOnEdges (:100-119) with one of the built-in functions, on the device. GS_SLICE_COUNT
  // is the only one a NullValue stream admits.
  std::vector<std::pair<K, int64_t>> reduceOnEdges(gs_slice_op op) const {
    std::vector<std::pair<K, int64_t>> out;
    each_window([&](gs_slices h) {
      uint64_t nv = 0, ne = 0;
      gs_check(gs_slice_size(h, &nv, &ne));
      std::vector<int64_t> v(nv + 1), r(nv + 1);
      size_t got = 0;
      gs_check(gs_slice_reduce(h, (int)op, v.data(), r.data(), v.size(), &got));
      for (size_t k = 0; k < got; ++k) out.emplace_back((K)v[k], r[k]);
    });
    return out;
  }

  // reduceOnEdges (:100-119) with a user function, applied in arrival order on the host
  std::vector<std::pair<K, EV>> reduceOnEdges(const std::function<EV(EV, EV)>& reduce) const {
    std::vector<std::pair<K, EV>> out;
    each_neighborhood([&](K vertex, const std::vector<std::pair<K, EV>>& nb) {
      EV acc = nb[0].second;
      for (size_t i = 1; i < nb.size(); ++i) acc = reduce(acc, nb[i].second);
      out.emplace_back(vertex, acc);
    });
    return out;
  }

  // foldNeighbors (:61-85): fold(accum, vertexID, neighborID, edgeValue) from `initial`
  template <typename T>
  std::vector<T> foldNeighbors(const T& initial,
                               const typename NonDeduced<std::function<T(T, K, K, EV)>>::type& fold) const {
    std::vector<T> out;
    each_neighborhood([&](K vertex, const std::vector<std::pair<K, EV>>& nb) {
      T acc = initial;
      for (const auto& e : nb) acc = fold(std::move(acc), vertex, e.first, e.second);
      out.push_back(std::move(acc));
    });
    return out;
  }
  template <typename T>
  std::vector<T> foldNeighbors(const T& initial, EdgesFold<K, EV, T>& fold) const {
    return foldNeighbors<T>(initial, [&fold](T a, K v, K n, EV e) { return fold.foldEdges(std::move(a), v, n, e); });
  }

  // applyOnNeighbors (:121-131): apply(vertexID, neighbors (id, value), collector)
  template <typename T>
  std::vector<T> applyOnNeighbors(
      const std::function<void(K, const std::vector<std::pair<K, EV>>&, std::vector<T>&)>& apply) const {
    std::vector<T> out;
    each_neighborhood([&](K vertex, const std::vector<std::pair<K, EV>>& nb) { apply(vertex, nb, out); });
    return out;
  }

 private:
  struct SliceHandle {
    gs_slices s = nullptr;
    SliceHandle(int device, size_t edges) { gs_check(gs_slice_create(&s, device, edges)); }
    ~SliceHandle() { gs_slice_destroy(s); }
    SliceHandle(const SliceHandle&) = delete;
    SliceHandle& operator=(const SliceHandle&) = delete;
  };

  // every window of the stream, in order, as the current window of one handle
  void each_window(const std::function<void(gs_slices)>& fn) const {
    const size_t n = edges_->edges.size();
    if (n == 0) return;
    const int dir = dir_ == EdgeDirection::OUT ? GS_SLICE_OUT : dir_ == EdgeDirection::IN ? GS_SLICE_IN : GS_SLICE_ALL;
    const bool one = edges_->timestamps.empty() || timeMillis_ <= 0;
    SliceHandle h(device_, 0);
    std::vector<int64_t> src, dst, val;
    size_t i = 0;
    while (i < n) {
      size_t j = n;
      if (!one) {
        const int64_t w = edges_->timestamps[i] / timeMillis_;
        for (j = i + 1; j < n && edges_->timestamps[j] / timeMillis_ == w;) ++j;
      }
      src.resize(j - i);
      dst.resize(j - i);
      if (kHasValue) val.resize(j - i);
      for (size_t k = i; k < j; ++k) {
        src[k - i] = (int64_t)edges_->edges[k].getSource();
        dst[k - i] = (int64_t)edges_->edges[k].getTarget();
        if constexpr (kHasValue) val[k - i] = edges_->edges[k].getValue();
      }
      gs_check(gs_slice_window(h.s, src.data(), dst.data(), kHasValue ? val.data() : nullptr, j - i, dir));
      fn(h.s);
      i = j;
    }
  }

  void each_neighborhood(const std::function<void(K, const std::vector<std::pair<K, EV>>&)>& fn) const {
    each_window([&](gs_slices h) {
      uint64_t nv = 0, ne = 0;
      gs_check(gs_slice_size(h, &nv, &ne));
      std::vector<int64_t> v(nv + 1), nbr(ne + 1), val(kHasValue ? ne + 1 : 0);
      std::vector<uint64_t> off(nv + 2);
      size_t gv = 0, ge = 0;
      gs_check(gs_slice_neighborhoods(h, v.data(), off.data(), nbr.data(), kHasValue ? val.data() : nullptr, nv + 1,
                                      ne + 1, &gv, &ge));
      std::vector<std::pair<K, EV>> nb;
      for (size_t k = 0; k < gv; ++k) {
        nb.clear();
        for (uint64_t e = off[k]; e < off[k + 1]; ++e) {
          if constexpr (kHasValue) nb.emplace_back((K)nbr[e], val[e]);
          else nb.emplace_back((K)nbr[e], NullValue{});
        }
        fn((K)v[k], nb);
      }
    });
  }

  const EdgeStream<K, EV>* edges_;
  int64_t timeMillis_;
  EdgeDirection dir_;
  int device_;
};

// SimpleEdgeStream.aggregate (SimpleEdgeStream.java:100-102)
template <typename K, typename EV>
class SimpleEdgeStream {
 public:
  explicit SimpleEdgeStream(EdgeStream<K, EV> edges) : edges_(std::move(edges)) {}

  // slice (SimpleEdgeStream.java:135-167): the stream cut into windows of timeMillis and keyed
  // by source (OUT, the default), target (IN) or both (ALL). The SnapshotStream reads this
  // stream's edges: keep the SimpleEdgeStream alive while it is used.
  SnapshotStream<K, EV> slice(int64_t timeMillis, EdgeDirection direction = EdgeDirection::OUT, int device = 0) const {
    return SnapshotStream<K, EV>(&edges_, timeMillis, direction, device);
  }

  template <typename S, typename T>
  void aggregate(SummaryBulkAggregation<K, EV, S, T>& summaryAggregation,
                 const typename SummaryBulkAggregation<K, EV, S, T>::Sink& sink) {
    summaryAggregation.run(edges_, sink);
  }
  template <typename S, typename T>
  std::vector<T> aggregate(SummaryBulkAggregation<K, EV, S, T>& summaryAggregation) {
    return summaryAggregation.run(edges_);
  }

  // getDegrees / getInDegrees / getOutDegrees (SimpleEdgeStream.java:406-459): the reference
  // emits a running Vertex<K, Long> per endpoint occurrence; these return the last value it
  // emits per key -- the final degree of every vertex with one, ascending by id. The stream's
  // edges are folded through a degree summary (gs_summary.h, GS_KIND_DEGREE) on `device`.
  std::vector<Vertex<K, long>> getDegrees(int device = 0) const { return degrees(GS_DEGREE_ALL, device); }
  std::vector<Vertex<K, long>> getInDegrees(int device = 0) const { return degrees(GS_DEGREE_IN, device); }
  std::vector<Vertex<K, long>> getOutDegrees(int device = 0) const { return degrees(GS_DEGREE_OUT, device); }

  // numberOfVertices (SimpleEdgeStream.java:366-386): the last value of the running count of
  // distinct endpoints.
  long numberOfVertices(int device = 0) const {
    DegreeHandle d(device, edges_.edges.size());
    fold_degrees(d.h, GS_DEGREE_ALL);
    uint64_t n = 0;
    gs_check(gs_num_vertices(d.h, &n));
    return (long)n;
  }

  // numberOfEdges (SimpleEdgeStream.java:388-404): a host count.
  long numberOfEdges() const { return (long)edges_.edges.size(); }

  // The continuous forms: every value the reference's operators emit, in arrival order, where
  // the members above return the last one. The stream's edges are folded through a degstream
  // handle (gs_summary.h, the gs_degstream_* section) on `device`.
  // getDegreeStream: the running Vertex<K, Long> of every endpoint occurrence (DegreeMapFunction,
  // SimpleEdgeStream.java:461-478); direction ALL / IN / OUT as getDegrees / getInDegrees /
  // getOutDegrees.
  std::vector<Vertex<K, long>> getDegreeStream(EdgeDirection direction = EdgeDirection::ALL, int device = 0) const {
    DegstreamHandle h(device, degree_dir(direction), edges_.edges.size());
    fold_degstream(h.d, std::vector<uint8_t>());
    uint64_t size[5] = {0, 0, 0, 0, 0};
    gs_check(gs_degstream_size(h.d, size));
    std::vector<int64_t> v(size[1] + 1);
    std::vector<uint32_t> deg(size[1] + 1);
    size_t got = 0;
    gs_check(gs_degstream_rows(h.d, v.data(), nullptr, deg.data(), v.size(), &got));
    std::vector<Vertex<K, long>> out(got);
    for (size_t i = 0; i < got; ++i) out[i] = Vertex<K, long>{(K)v[i], (long)deg[i]};
    return out;
  }

  // degreeDistributionStream: the (degree, count) record example/DegreeDistribution.java emits at
  // every change (DegreeDistribution.java:84-132), in arrival order. deletions: empty (every edge
  // an addition) or one byte per edge, bit 0 = deletion (EventType).
  std::vector<std::pair<long, long>> degreeDistributionStream(const std::vector<uint8_t>& deletions = {},
                                                              int device = 0) const {
    if (!deletions.empty() && deletions.size() != edges_.edges.size())
      throw GsException(GS_ERR_INVALID, "degreeDistributionStream: one deletion byte per edge");
    DegstreamHandle h(device, GS_DEGREE_ALL, edges_.edges.size());
    fold_degstream(h.d, deletions);
    uint64_t size[5] = {0, 0, 0, 0, 0};
    gs_check(gs_degstream_size(h.d, size));
    std::vector<uint32_t> deg(size[2] + 1), cnt(size[2] + 1);
    size_t got = 0;
    gs_check(gs_degstream_records(h.d, nullptr, deg.data(), cnt.data(), deg.size(), &got));
    std::vector<std::pair<long, long>> out(got);
    for (size_t i = 0; i < got; ++i) out[i] = std::make_pair((long)deg[i], (long)cnt[i]);
    return out;
  }

  // numberOfVerticesStream (SimpleEdgeStream.java:366-386): GlobalAggregateMapper over
  // VertexCountMapper emits k at the k-th first-seen endpoint. The first-seen endpoints are the
  // distinct handle's new vertices.
  std::vector<long> numberOfVerticesStream(int device = 0) const {
    DistinctHandle h(device, edges_.edges.size());
    fold_distinct(h.d);
    size_t got = 0;
    const int rc = gs_distinct_new_vertices(h.d, nullptr, nullptr, 0, &got);
    if (rc != GS_ERR_TRUNCATED) gs_check(rc);
    std::vector<long> out(got);
    for (size_t k = 0; k < got; ++k) out[k] = (long)(k + 1);
    return out;
  }

  // numberOfEdgesStream (SimpleEdgeStream.java:388-404): the running count 1..n, one per edge.
  std::vector<long> numberOfEdgesStream() const {
    std::vector<long> out(edges_.edges.size());
    for (size_t i = 0; i < out.size(); ++i) out[i] = (long)(i + 1);
    return out;
  }

  // distinct (SimpleEdgeStream.java:301-323): the stream of first-seen (source, target) pairs,
  // each with the value and timestamp of its first occurrence, in arrival order. The documented
  // and pinned behaviour (TestDistinct.java:38-44), not DistinctEdgeMapper's single set of
  // targets (include/gs_summary.h, the gs_distinct_* section). The stream's edges are folded
  // through a distinct handle on `device`.
  SimpleEdgeStream<K, EV> distinct(int device = 0) const {
    DistinctHandle h(device, edges_.edges.size());
    fold_distinct(h.d);
    uint64_t nv = 0, ne = 0, folded = 0, new_v = 0, new_e = 0;
    gs_check(gs_distinct_size(h.d, &nv, &ne, &folded, &new_v, &new_e));
    std::vector<uint32_t> index(new_e + 1);
    size_t got = 0;
    gs_check(gs_distinct_new_edges(h.d, index.data(), nullptr, nullptr, index.size(), &got));
    EdgeStream<K, EV> out;
    out.parallelism = edges_.parallelism;
    out.edges.reserve(got);
    for (size_t k = 0; k < got; ++k) {
      out.edges.push_back(edges_.edges[index[k]]);
      if (!edges_.timestamps.empty()) out.timestamps.push_back(edges_.timestamps[index[k]]);
    }
    return SimpleEdgeStream<K, EV>(std::move(out));
  }

  // getVertices (SimpleEdgeStream.java:116-121, 181-202): every vertex once, at its first
  // appearance (source before target), in emission order.
  std::vector<Vertex<K, NullValue>> getVertices(int device = 0) const {
    DistinctHandle h(device, edges_.edges.size());
    fold_distinct(h.d);
    uint64_t nv = 0, ne = 0, folded = 0, new_v = 0, new_e = 0;
    gs_check(gs_distinct_size(h.d, &nv, &ne, &folded, &new_v, &new_e));
    std::vector<int64_t> v(nv + 1);
    size_t got = 0;
    gs_check(gs_distinct_vertices(h.d, v.data(), v.size(), &got));
    std::vector<Vertex<K, NullValue>> out(got);
    for (size_t k = 0; k < got; ++k) out[k] = Vertex<K, NullValue>{(K)v[k], NullValue{}};
    return out;
  }

  const EdgeStream<K, EV>& getEdges() const { return edges_; }

 private:
  struct DistinctHandle {
    gs_distinct d = nullptr;
    DistinctHandle(int device, size_t edges) {
      gs_check(gs_distinct_create(&d, device, GS_DISTINCT_DIRECTED, 2 * edges, edges));
    }
    ~DistinctHandle() { gs_distinct_destroy(d); }
    DistinctHandle(const DistinctHandle&) = delete;
    DistinctHandle& operator=(const DistinctHandle&) = delete;
  };

  void fold_distinct(gs_distinct d) const {
    const size_t n = edges_.edges.size();
    std::vector<int64_t> src(n), dst(n);
    for (size_t i = 0; i < n; ++i) {
      src[i] = (int64_t)edges_.edges[i].getSource();
      dst[i] = (int64_t)edges_.edges[i].getTarget();
    }
    gs_check(gs_distinct_fold(d, src.data(), dst.data(), n));
  }

  struct DegstreamHandle {
    gs_degstream d = nullptr;
    DegstreamHandle(int device, int dir, size_t edges) { gs_check(gs_degstream_create(&d, device, dir, 2 * edges)); }
    ~DegstreamHandle() { gs_degstream_destroy(d); }
    DegstreamHandle(const DegstreamHandle&) = delete;
    DegstreamHandle& operator=(const DegstreamHandle&) = delete;
  };

  static int degree_dir(EdgeDirection direction) {
    return direction == EdgeDirection::IN ? GS_DEGREE_IN : direction == EdgeDirection::OUT ? GS_DEGREE_OUT : GS_DEGREE_ALL;
  }

  void fold_degstream(gs_degstream d, const std::vector<uint8_t>& deletions) const {
    const size_t n = edges_.edges.size();
    std::vector<int64_t> src(n), dst(n);
    for (size_t i = 0; i < n; ++i) {
      src[i] = (int64_t)edges_.edges[i].getSource();
      dst[i] = (int64_t)edges_.edges[i].getTarget();
    }
    gs_check(gs_degstream_fold(d, src.data(), dst.data(), deletions.empty() ? nullptr : deletions.data(), n));
  }

  struct DegreeHandle {
    gs_handle h = nullptr;
    DegreeHandle(int device, size_t edges) {
      gs_check(gs_create(&h, device, GS_KIND_DEGREE, std::max<size_t>(2 * edges, 16)));
    }
    ~DegreeHandle() { gs_destroy(h); }
    DegreeHandle(const DegreeHandle&) = delete;
    DegreeHandle& operator=(const DegreeHandle&) = delete;
  };

  void fold_degrees(gs_handle h, int dir) const {
    const size_t n = edges_.edges.size();
    std::vector<int64_t> src(n), dst(n);
    for (size_t i = 0; i < n; ++i) {
      src[i] = (int64_t)edges_.edges[i].getSource();
      dst[i] = (int64_t)edges_.edges[i].getTarget();
    }
    gs_check(gs_degree_fold(h, src.data(), dst.data(), nullptr, n, dir));
  }

  std::vector<Vertex<K, long>> degrees(int dir, int device) const {
    DegreeHandle d(device, edges_.edges.size());
    fold_degrees(d.h, dir);
    uint64_t nv = 0;
    gs_check(gs_num_vertices(d.h, &nv));
    std::vector<int64_t> v(nv + 1), deg(nv + 1);
    size_t got = 0;
    gs_check(gs_degree_export(d.h, v.data(), deg.data(), v.size(), &got, /*sorted=*/1));
    std::vector<Vertex<K, long>> out(got);
    for (size_t i = 0; i < got; ++i) out[i] = Vertex<K, long>{(K)v[i], (long)deg[i]};
    return out;
  }

  EdgeStream<K, EV> edges_;
};

// --------------------------------------------------------------------------
// Library algorithms
// --------------------------------------------------------------------------
using DisjointSetRef = std::shared_ptr<DisjointSet>;
using CandidatesRef = std::shared_ptr<Candidates>;

// ConnectedComponents<K, EV> (ConnectedComponents.java:41-134)
template <typename EV = NullValue>
class ConnectedComponents : public SummaryBulkAggregation<int64_t, EV, DisjointSetRef, DisjointSetRef> {
  using Base = SummaryBulkAggregation<int64_t, EV, DisjointSetRef, DisjointSetRef>;

 public:
  // UpdateCC.foldEdges (:83-86): ds.union(vertex, vertex2); return ds
  struct UpdateCC : EdgesFold<int64_t, EV, DisjointSetRef> {
    DisjointSetRef foldEdges(DisjointSetRef ds, int64_t vertex, int64_t vertex2, EV) override {
      ds->union_(vertex, vertex2);
      return ds;
    }
  };
  // CombineCC.reduce (:116-126): merge the smaller into the larger
  struct CombineCC : ReduceFunction<DisjointSetRef> {
    DisjointSetRef reduce(DisjointSetRef s1, DisjointSetRef s2) override {
      if (s1->size() <= s2->size()) {
        s2->merge(*s1);
        return s2;
      }
      s1->merge(*s2);
      return s1;
    }
  };
  // ConnectedComponents(long mergeWindowTime) (:52-54); device/capacity are the GPU knobs
  explicit ConnectedComponents(int64_t mergeWindowTime, int device = 0, uint64_t capacity_hint = 1 << 16)
      : Base(std::make_shared<UpdateCC>(), std::make_shared<CombineCC>(),
             [device, capacity_hint] { return std::make_shared<DisjointSet>(device, capacity_hint); },
             mergeWindowTime, false) {}
};

// BipartitenessCheck<K, EV> (BipartitenessCheck.java:37-133)
template <typename EV = NullValue>
class BipartitenessCheck : public SummaryBulkAggregation<int64_t, EV, CandidatesRef, CandidatesRef> {
  using Base = SummaryBulkAggregation<int64_t, EV, CandidatesRef, CandidatesRef>;

 public:
  // edgeToCandidate (:54-61)
  static Candidates::EdgeCandidate edgeToCandidate(int64_t v1, int64_t v2) {
    return {std::min(v1, v2), std::max(v1, v2)};
  }
  // updateFunction.foldEdges (:93-95): candidates.merge(edgeToCandidate(v1, v2))
  struct updateFunction : EdgesFold<int64_t, EV, CandidatesRef> {
    CandidatesRef foldEdges(CandidatesRef candidates, int64_t v1, int64_t v2, EV) override {
      candidates->merge(edgeToCandidate(v1, v2));
      return candidates;
    }
  };
  // combineFunction.reduce (:128-130): c1.merge(c2)
  struct combineFunction : ReduceFunction<CandidatesRef> {
    CandidatesRef reduce(CandidatesRef c1, CandidatesRef c2) override {
      c1->merge(*c2);
      return c1;
    }
  };
  explicit BipartitenessCheck(int64_t mergeWindowTime, int device = 0, uint64_t capacity_hint = 1 << 16)
      : Base(std::make_shared<updateFunction>(), std::make_shared<combineFunction>(),
             [device, capacity_hint] { return std::make_shared<Candidates>(true, device, capacity_hint); },
             mergeWindowTime, false) {}
};

// --------------------------------------------------------------------------
// Exact triangle counts (gs_summary.h, the gs_triangle_* section)
// --------------------------------------------------------------------------
struct TriangleHandle {
  gs_triangles t = nullptr;
  TriangleHandle(int device, size_t edges) { gs_check(gs_triangle_create(&t, device, std::max<size_t>(edges, 16))); }
  ~TriangleHandle() { gs_triangle_destroy(t); }
  TriangleHandle(const TriangleHandle&) = delete;
  TriangleHandle& operator=(const TriangleHandle&) = delete;
};

// The text reader (gs_ingest.h, the gs_text_* section): host text in, chunks of device columns
// out. next() returns false once the text's last chunk has been delivered; the arrays of a chunk
// hold until the chunk after the next is asked for.
class TextReader {
 public:
  struct Chunk {
    const int64_t* src = nullptr;
    const int64_t* dst = nullptr;
    const int64_t* val = nullptr;   // third = GS_TEXT_THIRD_LONG
    const uint8_t* del = nullptr;   // third = GS_TEXT_THIRD_EVENT
    size_t n = 0;
    const uint64_t* first = nullptr;  // window mode: the first record and the id of every whole window
    const int64_t* window = nullptr;
    size_t n_windows = 0;
  };
  explicit TextReader(int device = 0, int sep = GS_SEP_WHITESPACE, int third = GS_TEXT_THIRD_NONE, int flags = 0,
                      size_t chunk_bytes = 0) {
    gs_check(gs_text_create(&t_, device, sep, third, flags, chunk_bytes));
  }
  ~TextReader() { gs_text_destroy(t_); }
  TextReader(const TextReader&) = delete;
  TextReader& operator=(const TextReader&) = delete;
  void setWindow(int64_t size) { gs_check(gs_text_set_window(t_, size)); }
  void open(const char* text, size_t len) {
    gs_check(gs_text_open(t_, text, len));
    done_ = false;
  }
  bool next(Chunk* c) {
    if (done_) return false;
    int last = 0;
    gs_check(gs_text_next(t_, &c->src, &c->dst, &c->val, &c->del, &c->n, &c->first, &c->window, &c->n_windows, &last));
    done_ = last != 0;
    return true;
  }
  void* stream() const {
    void* s = nullptr;
    gs_check(gs_text_get_stream(t_, &s));
    return s;
  }
  void waitStream(void* s) { gs_check(gs_text_wait_stream(t_, s)); }
  gs_text handle() const { return t_; }

 private:
  gs_text t_ = nullptr;
  bool done_ = true;
};

// WindowTriangles (example/WindowTriangles.java:60-65): slice(windowTime, ALL), candidate
// edges per neighbourhood, count per window. run() returns (count, window.maxTimestamp())
// for every tumbling window that holds at least one non-loop edge, in window order. On
// windows without self-loops the counts are the reference's; its j = i candidates
// (:103-104) are not reproduced.
class WindowTriangles {
 public:
  explicit WindowTriangles(int64_t windowMillis, int device = 0) : window_(windowMillis), device_(device) {}

  template <typename K, typename EV>
  std::vector<std::pair<long, int64_t>> run(const EdgeStream<K, EV>& stream) const {
    std::map<int64_t, std::pair<std::vector<int64_t>, std::vector<int64_t>>> windows;
    for (size_t i = 0; i < stream.edges.size(); ++i) {
      const int64_t ts = stream.timestamps.empty() ? 0 : stream.timestamps[i];
      int64_t w = window_ > 0 ? ts / window_ : 0;
      if (window_ > 0 && ts % window_ < 0) --w;  // floor: TimeWindow start = ts - (ts mod size)
      auto& e = windows[w];
      e.first.push_back((int64_t)stream.edges[i].getSource());
      e.second.push_back((int64_t)stream.edges[i].getTarget());
    }
    std::vector<std::pair<long, int64_t>> out;
    if (windows.empty()) return out;
    TriangleHandle h(device_, stream.edges.size());
    for (const auto& kv : windows) {
      gs_check(gs_triangle_reset(h.t));
      gs_check(gs_triangle_fold(h.t, kv.second.first.data(), kv.second.second.data(), kv.second.first.size()));
      uint64_t tri = 0, edges = 0, vertices = 0;
      gs_check(gs_triangle_count(h.t, &tri, &edges, &vertices));
      if (edges == 0) continue;  // only self-loops
      const int64_t maxTimestamp = window_ > 0 ? kv.first * window_ + window_ - 1 : std::numeric_limits<int64_t>::max();
      out.emplace_back((long)tri, maxTimestamp);
    }
    return out;
  }

  // The reference driver's text form (WindowTriangles.java:178-186: "src trg timestamp" lines,
  // split + Long.parseLong x 3) read on the device: whole windows from a TextReader, then per
  // window reset, fold, count. A window here is a maximal run of consecutive lines with equal
  // ts / windowMillis (truncating): rows come in stream order, and on an ascending stream of
  // non-negative timestamps, the reference's input, they are run()'s rows. A malformed line
  // throws (GS_ERR_PARSE) after the windows of the chunks before it.
  std::vector<std::pair<long, int64_t>> runText(const char* text, size_t len, int sep = GS_SEP_WHITESPACE,
                                                size_t chunk_bytes = 0) const {
    if (window_ <= 0) throw std::invalid_argument("WindowTriangles::runText: the window size must be positive");
    std::vector<std::pair<long, int64_t>> out;
    TextReader reader(device_, sep, GS_TEXT_THIRD_LONG, 0, chunk_bytes);
    reader.setWindow(window_);
    reader.open(text, len);
    TriangleHandle h(device_, 1024);
    void* hs = nullptr;
    gs_check(gs_triangle_get_stream(h.t, &hs));
    TextReader::Chunk c;
    std::vector<uint64_t> first;
    std::vector<int64_t> ids;
    while (reader.next(&c)) {
      if (c.n_windows == 0) continue;
      first.resize(c.n_windows + 1);
      ids.resize(c.n_windows);
      size_t got = 0;
      gs_check(gs_text_windows(reader.handle(), first.data(), ids.data(), c.n_windows, &got));
      first[c.n_windows] = c.n;
      for (size_t w = 0; w < c.n_windows; ++w) {
        gs_check(gs_triangle_reset(h.t));
        gs_check(gs_triangle_fold_device(h.t, c.src + first[w], c.dst + first[w], first[w + 1] - first[w], 1));
        uint64_t tri = 0, edges = 0, vertices = 0;
        gs_check(gs_triangle_count(h.t, &tri, &edges, &vertices));
        if (edges == 0) continue;  // only self-loops
        out.emplace_back((long)tri, ids[w] * window_ + window_ - 1);
      }
      reader.waitStream(hs);  // the next chunk after these folds
    }
    return out;
  }

 private:
  int64_t window_;
  int device_;
};

// WindowTriangles over Flink's sliding time windows (SlidingEventTimeWindows.of(size, slide),
// offset 0): an element of timestamp ts belongs to the size / slide windows that start at
// lastStart, lastStart - slide, ... > ts - size, lastStart = ts - (ts mod slide). size must be
// a multiple of slide (refused otherwise): panes are slide ms wide and a window is the union of
// size / slide consecutive panes. The handle slides instead of re-folding: per pane one fold
// (of zero elements for a pane without edges) on a handle with refresh on, then
// gs_triangle_expire(size / slide). run() returns (count, window.maxTimestamp()) for every
// window Flink would fire that holds at least one non-loop edge, in window order: the leading
// partial windows and the trailing ones behind the last pane with edges included. With
// size == slide these are WindowTriangles' rows.
class SlidingWindowTriangles {
 public:
  SlidingWindowTriangles(int64_t sizeMillis, int64_t slideMillis, int device = 0)
      : size_(sizeMillis), slide_(slideMillis), device_(device) {
    if (slideMillis <= 0 || sizeMillis <= 0 || sizeMillis % slideMillis != 0)
      throw std::invalid_argument("SlidingWindowTriangles: size must be a positive multiple of slide");
  }

  template <typename K, typename EV>
  std::vector<std::pair<long, int64_t>> run(const EdgeStream<K, EV>& stream) const {
    std::map<int64_t, std::pair<std::vector<int64_t>, std::vector<int64_t>>> panes;
    for (size_t i = 0; i < stream.edges.size(); ++i) {
      const int64_t ts = stream.timestamps.empty() ? 0 : stream.timestamps[i];
      int64_t p = ts / slide_;
      if (ts % slide_ < 0) --p;  // floor
      auto& e = panes[p];
      e.first.push_back((int64_t)stream.edges[i].getSource());
      e.second.push_back((int64_t)stream.edges[i].getTarget());
    }
    std::vector<std::pair<long, int64_t>> out;
    if (panes.empty()) return out;
    const int64_t w = size_ / slide_;
    TriangleHandle h(device_, stream.edges.size());
    gs_check(gs_triangle_set_refresh(h.t, 1));
    auto next = panes.begin();
    // q: the last pane of the window [(q - w + 1) * slide, (q + 1) * slide)
    for (int64_t q = next->first; q < panes.rbegin()->first + w; ++q) {
      if (next != panes.end() && next->first == q) {
        gs_check(gs_triangle_fold(h.t, next->second.first.data(), next->second.second.data(), next->second.first.size()));
        ++next;
      } else {
        gs_check(gs_triangle_fold(h.t, nullptr, nullptr, 0));  // an empty pane ages the others
      }
      gs_check(gs_triangle_expire(h.t, (uint64_t)w));
      uint64_t tri = 0, edges = 0, vertices = 0;
      gs_check(gs_triangle_count(h.t, &tri, &edges, &vertices));
      if (edges == 0) {
        // nothing is held: the empty panes up to the next one with edges would change nothing
        if (next != panes.end() && next->first > q + 1) q = next->first - 1;
        continue;
      }
      out.emplace_back((long)tri, (q + 1) * slide_ - 1);
    }
    return out;
  }

 private:
  int64_t size_, slide_;
  int device_;
};

// ExactTriangleCount (example/ExactTriangleCount.java:52-56): buildNeighborhood,
// IntersectNeighborhoods, SumAndEmitCounters. stream() returns every emitted tuple in order;
// run() folds the stream in batches of `batch` edges and returns the final counter map: key -1
// the total, every other key a vertex with at least one triangle. Equal to the reference's final counters on a stream
// without repeated edges and self-loops (it counts a repeated edge's triangles again).
class ExactTriangleCount {
 public:
  explicit ExactTriangleCount(int device = 0) : device_(device) {}

  template <typename K, typename EV>
  std::map<int64_t, long> run(const EdgeStream<K, EV>& stream, size_t batch) const {
    const size_t n = stream.edges.size();
    TriangleHandle h(device_, n);
    std::vector<int64_t> src(n), dst(n);
    for (size_t i = 0; i < n; ++i) {
      src[i] = (int64_t)stream.edges[i].getSource();
      dst[i] = (int64_t)stream.edges[i].getTarget();
    }
    if (batch == 0) batch = n;
    for (size_t i = 0; i < n; i += batch)
      gs_check(gs_triangle_fold(h.t, src.data() + i, dst.data() + i, std::min(batch, n - i)));
    uint64_t tri = 0, edges = 0, vertices = 0;
    gs_check(gs_triangle_count(h.t, &tri, &edges, &vertices));
    std::vector<int64_t> v(vertices + 1), c(vertices + 1);
    size_t got = 0;
    gs_check(gs_triangle_export(h.t, v.data(), c.data(), v.size(), &got, /*nonzero_only=*/1));
    std::map<int64_t, long> out;
    for (size_t i = 0; i < got; ++i) out[v[i]] = (long)c[i];
    out[-1] = (long)tri;
    return out;
  }

  // stream(): the example's continuous output, every Tuple2 SumAndEmitCounters emits
  // (ExactTriangleCount.java:121-133), through a tristream handle in the reference's mode (a
  // repeated edge is intersected again): per arrival that closes triangles the running counts of
  // the common neighbours, ascending, of the two endpoints, and (-1, total). The sequence does
  // not depend on `batch`. Self-loops emit nothing (the reference's artefacts are not
  // reproduced).
  template <typename K, typename EV>
  std::vector<std::pair<int64_t, long>> stream(const EdgeStream<K, EV>& stream, size_t batch = 0) const {
    const size_t n = stream.edges.size();
    TristreamHandle h(device_, n);
    std::vector<int64_t> src(n), dst(n);
    for (size_t i = 0; i < n; ++i) {
      src[i] = (int64_t)stream.edges[i].getSource();
      dst[i] = (int64_t)stream.edges[i].getTarget();
    }
    if (batch == 0) batch = std::max<size_t>(n, 1);
    batch = std::min<size_t>(batch, (size_t)1 << 22);  // (the largest fold whose rows the handle keeps)
    std::vector<std::pair<int64_t, long>> out;
    std::vector<uint32_t> closed, arrival;
    std::vector<int64_t> total, vertex, count;
    for (size_t i = 0; i < n; i += batch) {
      const size_t len = std::min(batch, n - i);
      gs_check(gs_tristream_fold(h.d, src.data() + i, dst.data() + i, len));
      uint64_t size[4] = {0, 0, 0, 0};
      gs_check(gs_tristream_size(h.d, size));
      closed.resize(size[0] + 1), total.resize(size[0] + 1);
      arrival.resize(size[1] + 1), vertex.resize(size[1] + 1), count.resize(size[1] + 1);
      size_t rows = 0, recs = 0;
      gs_check(gs_tristream_rows(h.d, closed.data(), total.data(), closed.size(), &rows));
      gs_check(gs_tristream_records(h.d, arrival.data(), vertex.data(), count.data(), arrival.size(), &recs));
      size_t r = 0;
      for (size_t a = 0; a < rows; ++a) {
        for (; r < recs && arrival[r] == a; ++r) out.push_back(std::make_pair(vertex[r], (long)count[r]));
        if (closed[a]) out.push_back(std::make_pair((int64_t)-1, (long)total[a]));
      }
    }
    return out;
  }

 private:
  struct TristreamHandle {
    gs_tristream d = nullptr;
    TristreamHandle(int device, size_t edges) { gs_check(gs_tristream_create(&d, device, GS_TRISTREAM_COUNT, edges)); }
    ~TristreamHandle() { gs_tristream_destroy(d); }
    TristreamHandle(const TristreamHandle&) = delete;
    TristreamHandle& operator=(const TristreamHandle&) = delete;
  };
  int device_;
};

// --------------------------------------------------------------------------
// k-spanner (gs_summary.h, the gs_spanner_* section)
// --------------------------------------------------------------------------
// AdjacencyListGraph (summaries/AdjacencyListGraph.java:27-140) backed by a spanner handle.
// addEdge and the spanner's per-edge update are buffered and reach the device as one batch on
// any read, like DisjointSet's unions; a batch holds calls of one kind only, so their order is
// kept. k is the handle's distance bound: what updateLocal and combine decide by.
class AdjacencyListGraph {
 public:
  explicit AdjacencyListGraph(int k = 3, int device = 0, uint64_t edge_hint = 1 << 10)
      : k_(k), device_(device), hint_(edge_hint) {}
  ~AdjacencyListGraph() { gs_spanner_destroy(h_); }
  AdjacencyListGraph(const AdjacencyListGraph&) = delete;
  AdjacencyListGraph& operator=(const AdjacencyListGraph&) = delete;

  // addEdge (:46-67): the edge joins the graph, whatever the distance of its endpoints
  void addEdge(int64_t src, int64_t trg) { push(src, trg, false); }
  // Spanner.UpdateLocal.foldEdges (Spanner.java:71-77): if (!boundedBFS(src, trg, k)) addEdge
  void updateLocal(int64_t src, int64_t trg) { push(src, trg, true); }
  // boundedBFS (:79-116)
  bool boundedBFS(int64_t src, int64_t trg, int k) {
    flush();
    uint8_t out = 0;
    gs_check(gs_spanner_within(handle(), &src, &trg, 1, k, &out));
    return out != 0;
  }
  // getAdjacencyMap (:37-39): vertex -> its neighbours (a loop holds its own vertex once)
  std::map<int64_t, std::set<int64_t>> getAdjacencyMap() {
    flush();
    uint64_t edges = 0, vertices = 0;
    gs_check(gs_spanner_count(handle(), &edges, &vertices));
    std::vector<int64_t> v(vertices + 1), nb(2 * edges + 1);
    std::vector<uint64_t> off(vertices + 2);
    size_t nv = 0, ne = 0;
    gs_check(gs_spanner_neighbors(h_, v.data(), off.data(), nb.data(), v.size(), nb.size(), &nv, &ne));
    std::map<int64_t, std::set<int64_t>> out;
    for (size_t i = 0; i < nv; ++i) out[v[i]].insert(nb.begin() + (long)off[i], nb.begin() + (long)off[i + 1]);
    return out;
  }
  // getAdjacencyMap().size(), what CombineSpanners compares
  size_t size() {
    flush();
    uint64_t edges = 0, vertices = 0;
    gs_check(gs_spanner_count(handle(), &edges, &vertices));
    return (size_t)vertices;
  }
  // the edges (lo <= hi) ascending
  std::vector<std::pair<int64_t, int64_t>> edges() {
    flush();
    uint64_t edges = 0, vertices = 0;
    gs_check(gs_spanner_count(handle(), &edges, &vertices));
    std::vector<int64_t> lo(edges + 1), hi(edges + 1);
    size_t n = 0;
    gs_check(gs_spanner_export(h_, lo.data(), hi.data(), lo.size(), &n));
    std::vector<std::pair<int64_t, int64_t>> out(n);
    for (size_t i = 0; i < n; ++i) out[i] = {lo[i], hi[i]};
    return out;
  }
  // the edges of `other`, ascending by (lo, hi), through updateLocal; `other` is unchanged
  void combine(AdjacencyListGraph& other) {
    flush();
    other.flush();
    if (other.h_) gs_check(gs_spanner_combine(handle(), other.h_));
  }
  // reset (:118-120)
  void reset() {
    src_.clear();
    dst_.clear();
    if (h_) gs_check(gs_spanner_reset(h_));
  }
  int k() const { return k_; }
  gs_spanner handle() {
    if (!h_) gs_check(gs_spanner_create(&h_, device_, k_, hint_));
    return h_;
  }
  void flush() {
    if (src_.empty()) return;
    if (conditional_) gs_check(gs_spanner_fold(handle(), src_.data(), dst_.data(), src_.size(), nullptr));
    else gs_check(gs_spanner_add(handle(), src_.data(), dst_.data(), src_.size()));
    src_.clear();
    dst_.clear();
  }

 private:
  void push(int64_t s, int64_t t, bool conditional) {
    if (conditional != conditional_) flush();
    conditional_ = conditional;
    src_.push_back(s);
    dst_.push_back(t);
  }
  int k_, device_;
  uint64_t hint_;
  gs_spanner h_ = nullptr;
  std::vector<int64_t> src_, dst_;
  bool conditional_ = false;
};
using AdjacencyListGraphRef = std::shared_ptr<AdjacencyListGraph>;

// Spanner<K, EV> (library/Spanner.java:40-118)
template <typename EV = NullValue>
class Spanner : public SummaryBulkAggregation<int64_t, EV, AdjacencyListGraphRef, AdjacencyListGraphRef> {
  using Base = SummaryBulkAggregation<int64_t, EV, AdjacencyListGraphRef, AdjacencyListGraphRef>;

 public:
  // UpdateLocal.foldEdges (:71-77)
  struct UpdateLocal : EdgesFold<int64_t, EV, AdjacencyListGraphRef> {
    AdjacencyListGraphRef foldEdges(AdjacencyListGraphRef g, int64_t src, int64_t trg, EV) override {
      g->updateLocal(src, trg);
      return g;
    }
  };
  // CombineSpanners.reduce (:92-116): the spanner with strictly more vertices takes the other's
  // edges; on a tie g2 takes g1's. The edges arrive ascending by (lo, hi) (gs_spanner_combine).
  struct CombineSpanners : ReduceFunction<AdjacencyListGraphRef> {
    AdjacencyListGraphRef reduce(AdjacencyListGraphRef g1, AdjacencyListGraphRef g2) override {
      if (g1->size() > g2->size()) {
        g1->combine(*g2);
        return g1;
      }
      g2->combine(*g1);
      return g2;
    }
  };
  // Spanner(long mergeWindowTime, int k) (:50-53); device is the GPU knob
  Spanner(int64_t mergeWindowTime, int k, int device = 0)
      : Base(std::make_shared<UpdateLocal>(), std::make_shared<CombineSpanners>(),
             [k, device] { return std::make_shared<AdjacencyListGraph>(k, device); }, mergeWindowTime, false) {}
};

// ---------------------------------------------------------------------------
// weighted matching (gs_summary.h, the gs_matching_* section)
// ---------------------------------------------------------------------------
// MatchingEvent (util/MatchingEvent.java:25-44): a Tuple2 (f0 = type, f1 = edge)
struct MatchingEvent {
  enum class Type { ADD = GS_MATCH_ADD, REMOVE = GS_MATCH_REMOVE };  // :27
  Type type;
  Edge<int64_t, int64_t> edge;
  Type geType() const { return type; }  // (:36, the reference's spelling)
  Type getType() const { return type; }
  const Edge<int64_t, int64_t>& getEdge() const { return edge; }
  bool operator==(const MatchingEvent& o) const {
    return type == o.type && edge.f0 == o.edge.f0 && edge.f1 == o.edge.f1 && edge.f2 == o.edge.f2;
  }
};

// CentralizedWeightedMatching (example/CentralizedWeightedMatching.java:36-110): the
// WeightedMatchingFlatMapper at parallelism 1 over the edge stream. The matching lives on the
// device; `batch` arrivals are folded per call, with the same events whatever the batch size.
// An arrival's REMOVE events come with the edge at its source endpoint first (the reference
// iterates a HashSet there).
class CentralizedWeightedMatching {
 public:
  explicit CentralizedWeightedMatching(int device = 0) { gs_check(gs_matching_create(&h_, device, 0)); }
  ~CentralizedWeightedMatching() { gs_matching_destroy(h_); }
  CentralizedWeightedMatching(const CentralizedWeightedMatching&) = delete;
  CentralizedWeightedMatching& operator=(const CentralizedWeightedMatching&) = delete;

  // flatMap (:79-106) over the whole stream, in order
  std::vector<MatchingEvent> run(const EdgeStream<int64_t, int64_t>& stream, size_t batch = 1 << 16) {
    std::vector<MatchingEvent> out;
    if (batch == 0) batch = 1;
    const size_t n = stream.edges.size();
    std::vector<int64_t> s, d, w, es, ed, ew;
    std::vector<uint8_t> type;
    for (size_t at = 0; at < n; at += batch) {
      const size_t len = std::min(batch, n - at);
      s.resize(len);
      d.resize(len);
      w.resize(len);
      for (size_t i = 0; i < len; ++i) {
        s[i] = stream.edges[at + i].f0;
        d[i] = stream.edges[at + i].f1;
        w[i] = stream.edges[at + i].f2;
      }
      gs_check(gs_matching_fold(h_, s.data(), d.data(), w.data(), len, nullptr));
      size_t rows = 0;
      const int rc = gs_matching_events(h_, nullptr, nullptr, nullptr, nullptr, nullptr, 0, &rows);
      if (rc != GS_ERR_TRUNCATED) gs_check(rc);
      if (rows == 0) continue;
      type.resize(rows);
      es.resize(rows);
      ed.resize(rows);
      ew.resize(rows);
      gs_check(gs_matching_events(h_, nullptr, type.data(), es.data(), ed.data(), ew.data(), rows, &rows));
      for (size_t r = 0; r < rows; ++r)
        out.push_back({type[r] == GS_MATCH_ADD ? MatchingEvent::Type::ADD : MatchingEvent::Type::REMOVE,
                       {es[r], ed[r], ew[r]}});
    }
    return out;
  }

  // the matching as it stands, in order of acceptance
  std::vector<Edge<int64_t, int64_t>> matching() const {
    uint64_t edges = 0, vertices = 0;
    int64_t weight = 0;
    gs_check(gs_matching_count(h_, &edges, &vertices, &weight));
    std::vector<int64_t> s(edges + 1), d(edges + 1), w(edges + 1);
    size_t n = 0;
    gs_check(gs_matching_export(h_, s.data(), d.data(), w.data(), nullptr, s.size(), &n));
    std::vector<Edge<int64_t, int64_t>> out;
    for (size_t i = 0; i < n; ++i) out.push_back({s[i], d[i], w[i]});
    return out;
  }
  int64_t weight() const {
    uint64_t edges = 0, vertices = 0;
    int64_t weight = 0;
    gs_check(gs_matching_count(h_, &edges, &vertices, &weight));
    return weight;
  }
  gs_matching handle() const { return h_; }

 private:
  gs_matching h_ = nullptr;
};

// ---------------------------------------------------------------------------
// sampling triangle estimate (gs_summary.h, the gs_trisample_* section)
// ---------------------------------------------------------------------------
// TriangleEstimate (util/TriangleEstimate.java:23-44): a Tuple3 (f0 = source subtask,
// f1 = edge count, f2 = beta sum)
struct TriangleEstimate {
  int f0 = 0, f1 = 0, f2 = 0;
  TriangleEstimate() = default;
  TriangleEstimate(int source, int edges, int beta) : f0(source), f1(edges), f2(beta) {}
  int getSource() const { return f0; }
  int getEdgeCount() const { return f1; }
  int getBeta() const { return f2; }
};

// BroadcastTriangleCount (example/BroadcastTriangleCount.java:41-174): TriangleSampler and
// TriangleSummer at parallelism 1 over the edge stream, the coin seeded as in
// example/IncidenceSamplingTriangleCount.java. The instances live on the device; `batch` arrivals
// are folded per call, with the same rows whatever the batch size.
class BroadcastTriangleCount {
 public:
  static constexpr int64_t kSeed = -559038737;  // new Random(0xDEADBEEF)
  explicit BroadcastTriangleCount(int samples = 10000, int vertexCount = 1000, int device = 0, int64_t seed = kSeed,
                                  uint64_t thirdSeed = 0) {
    gs_check(gs_trisample_create(&h_, device, (uint64_t)(samples < 0 ? 0 : samples), vertexCount, seed, thirdSeed));
  }
  ~BroadcastTriangleCount() { gs_trisample_destroy(h_); }
  BroadcastTriangleCount(const BroadcastTriangleCount&) = delete;
  BroadcastTriangleCount& operator=(const BroadcastTriangleCount&) = delete;

  // the (edge count, estimate) tuples TriangleSummer collects (:155-172), in order
  template <typename K, typename EV>
  std::vector<std::pair<int, int>> run(const EdgeStream<K, EV>& stream, size_t batch = 1 << 16) {
    std::vector<std::pair<int, int>> out;
    if (batch == 0) batch = 1;
    const size_t n = stream.edges.size();
    std::vector<int64_t> s, d;
    std::vector<int32_t> edges, estimate;
    sampler_.clear();
    for (size_t at = 0; at < n; at += batch) {
      const size_t len = std::min(batch, n - at);
      s.resize(len);
      d.resize(len);
      for (size_t i = 0; i < len; ++i) {
        s[i] = (int64_t)stream.edges[at + i].getSource();
        d[i] = (int64_t)stream.edges[at + i].getTarget();
      }
      size_t rows = 0;
      gs_check(gs_trisample_fold(h_, s.data(), d.data(), len, &rows));
      if (rows == 0) continue;
      edges.resize(rows);
      estimate.resize(rows);
      std::vector<int32_t> beta(rows);
      gs_check(gs_trisample_rows(h_, edges.data(), estimate.data(), beta.data(), rows, &rows));
      for (size_t r = 0; r < rows; ++r) {
        out.push_back({edges[r], estimate[r]});
        sampler_.push_back(TriangleEstimate(0, edges[r], beta[r]));
      }
    }
    return out;
  }
  // the TriangleEstimates behind the last run's rows (source subtask 0)
  const std::vector<TriangleEstimate>& estimates() const { return sampler_; }
  // (arrivals folded, beta sum now, last emitted estimate)
  std::tuple<uint64_t, int, int> estimate() const {
    uint64_t arrivals = 0;
    int32_t beta = 0, est = 0;
    gs_check(gs_trisample_estimate(h_, &arrivals, &beta, &est));
    return {arrivals, beta, est};
  }
  gs_trisample handle() const { return h_; }

 private:
  gs_trisample h_ = nullptr;
  std::vector<TriangleEstimate> sampler_;
};

}  // namespace gelly
