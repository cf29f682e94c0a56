// gs_own.hpp -- Event, Stream, HostBuf<T>, SpanTimer: the one owner each of a HIP event, a HIP
// stream, a pinned host allocation and a pool of timing events.
//
// Like DevBuf (gs_devbuf.hpp) they release what they hold when they go out of scope, so a handle
// made of them names no member in its destroy function, and a set of resources that a call
// creates on first use is filled in a local and moved into the handle only when complete. Each
// is move-only, converts to its raw handle, and is empty after a failed create. What has to be
// waited for before a release stays with the callers. Not here: ParseCache (gs_ingest.hip) is
// thread-local and its release reports a return code to gs_parse_release; a thread-exit
// destructor must not call HIP, so it keeps its explicit free.
//
// Only the HIP API header and standard headers are read here: a host compiler can build a
// stand-alone check of the types (tests/cpp/own_sanitize.cpp).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <string.h>

#include <utility>
#include <vector>

namespace gsi {

// The owner of one raw handle that Destroy releases (null: nothing held); the types below
// convert to it.
template <typename Raw, hipError_t (*Destroy)(Raw)>
class Owned {
 public:
  Owned() = default;
  Owned(Owned&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  Owned& operator=(Owned&& o) noexcept {
    Owned t(std::move(o));  // (a self-move takes it and puts it back)
    std::swap(h_, t.h_);
    return *this;
  }
  ~Owned() { reset(); }
  void reset() {
    if (h_) (void)Destroy(h_);
    h_ = nullptr;
  }

 protected:
  // create(): releases what is held, then holds what `make` makes; empty on failure
  template <class Make>
  hipError_t remake(Make make) {
    reset();
    const hipError_t e = make(&h_);
    if (e != hipSuccess) h_ = nullptr;
    return e;
  }
  Raw h_ = nullptr;
};

struct Event : Owned<hipEvent_t, hipEventDestroy> {
  operator hipEvent_t() const { return h_; }
  hipError_t create(unsigned flags = hipEventDisableTiming) {
    return remake([&](hipEvent_t* e) { return hipEventCreateWithFlags(e, flags); });
  }
};

// Never holds the null stream: a Stream that was not created owns, and destroys, nothing.
struct Stream : Owned<hipStream_t, hipStreamDestroy> {
  operator hipStream_t() const { return h_; }
  hipError_t create(unsigned flags = hipStreamNonBlocking) {
    return remake([&](hipStream_t* s) { return hipStreamCreateWithFlags(s, flags); });
  }
  hipError_t create_with_priority(unsigned flags, int prio) {
    return remake([&](hipStream_t* s) { return hipStreamCreateWithPriority(s, flags, prio); });
  }
};

// Pinned host memory (hipHostMalloc) of `count` elements. A block allocated with
// hipHostMallocMapped holds words that the host and the device read before either writes them:
// it is zero-filled and dev() is its device mapping. Any other block is staging that the host
// fills before every use: it is left as allocated (zeroing the 34 MB of a summary's host-fold
// staging costs milliseconds inside its first large fold) and dev() is null.
template <typename T>
class HostBuf : Owned<void*, hipHostFree> {
 public:
  using Owned::reset;
  // Frees what it holds, then allocates; empty on failure (a block whose device mapping cannot
  // be taken is freed again).
  hipError_t alloc(size_t count, unsigned flags) {
    hipError_t e = remake([&](void** p) { return hipHostMalloc(p, count * sizeof(T), flags); });
    d_ = nullptr;
    n_ = count;
    if (e != hipSuccess || !(flags & hipHostMallocMapped)) return e;
    if ((e = hipHostGetDevicePointer(&d_, h_, 0)) != hipSuccess) reset();
    else memset(h_, 0, count * sizeof(T));
    return e;
  }
  T* get() const { return static_cast<T*>(h_); }
  operator T*() const { return get(); }
  // (a move leaves d_ and n_ behind: they count only while a block is held)
  T* dev() const { return h_ ? static_cast<T*>(d_) : nullptr; }
  size_t size() const { return h_ ? n_ : 0; }  // elements

 private:
  void* d_ = nullptr;
  size_t n_ = 0;
};

// Times spans of stream work with pooled timing events: begin(st) records and returns a span's
// start event (null if none could be created), end(id, start, st) records its end and queues
// it, drain(f) waits for every queued span and calls f(id, ms) for each whose time could be
// read. Whether spans are taken at all, and what the times add up to, stays with the caller.
// A start that gets no end() goes back with cancel(); one that is dropped is only lost to the
// pool. Destroying the timer destroys every event it made (the caller has their streams idle).
class SpanTimer {
 public:
  SpanTimer() = default;
  SpanTimer(SpanTimer&&) = default;
  SpanTimer& operator=(SpanTimer&&) = default;
  hipEvent_t begin(hipStream_t st) {
    const hipEvent_t a = take();
    if (a) (void)hipEventRecord(a, st);
    return a;
  }
  void end(int id, hipEvent_t start, hipStream_t st) {
    const hipEvent_t b = start ? take() : nullptr;
    if (!b) return cancel(start);
    (void)hipEventRecord(b, st);
    pending_.push_back({id, start, b});
  }
  void cancel(hipEvent_t start) {
    if (start) free_.push_back(start);
  }
  template <class F>
  void drain(F f) {
    for (const Span& s : pending_) {
      float ms = 0.f;
      if (hipEventSynchronize(s.b) == hipSuccess && hipEventElapsedTime(&ms, s.a, s.b) == hipSuccess) f(s.id, ms);
      free_.push_back(s.a);
      free_.push_back(s.b);
    }
    pending_.clear();
  }

 private:
  struct Span {
    int id;
    hipEvent_t a, b;
  };
  hipEvent_t take() {  // a pooled event, or a new one (null if it cannot be created)
    if (free_.empty()) {
      Event e;
      if (e.create(hipEventDefault) != hipSuccess) return nullptr;
      made_.push_back(std::move(e));
      return made_.back();
    }
    const hipEvent_t e = free_.back();
    free_.pop_back();
    return e;
  }
  std::vector<Event> made_;       // the owners of every event below
  std::vector<hipEvent_t> free_;  // the pool
  std::vector<Span> pending_;
};

}  // namespace gsi
