// own_sanitize.cpp -- stand-alone check of gsi::Event, Stream, HostBuf and SpanTimer
// (csrc/gs_own.hpp), alone and mixed with DevBuf in a handle-like struct, under the address and
// undefined-behaviour sanitizers (tests/test_own.py). The program supplies the HIP calls the
// two headers use itself, over malloc / free with a live set per kind of resource, a log of
// the releases and a switch that fails the k-th creating call; it needs no device.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <utility>
#include <vector>

#include "gs_devbuf.hpp"
#include "gs_own.hpp"

namespace {

enum Kind { EVENT = 0, STREAM = 1, HOST = 2, DEV = 3, KINDS = 4 };
std::set<void*> g_live[KINDS];
long g_made[KINDS] = {};
std::vector<std::pair<Kind, void*>> g_released;  // in order
std::map<void*, long> g_tick;                    // event -> the tick of its last record
long g_now = 0;
long g_fail_at = -1;  // the creating call (counted from 0 at arm()) that fails; -1: none
long g_seen = 0;

int g_failed = 0;
#define CHECK(cond)                                                 \
  do {                                                              \
    if (!(cond)) {                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                                   \
    }                                                               \
  } while (0)

void arm(long k) {
  g_fail_at = k;
  g_seen = 0;
}
bool fails_now() { return g_fail_at >= 0 && g_seen++ == g_fail_at; }

hipError_t make(Kind k, void** out, size_t bytes) {
  if (fails_now()) return hipErrorOutOfMemory;
  *out = std::malloc(bytes ? bytes : 1);
  if (!*out) return hipErrorOutOfMemory;
  if (k == HOST) {  // not zero: a block that has to be zero is filled by HostBuf
    for (size_t i = 0; i < bytes; ++i) static_cast<unsigned char*>(*out)[i] = 0xA5;
  }
  g_live[k].insert(*out);
  ++g_made[k];
  return hipSuccess;
}

hipError_t release(Kind k, void* p) {
  if (!g_live[k].erase(p)) {  // released twice, or never made here (the null stream included)
    std::printf("FAILED: release of a resource of kind %d that is not live\n", (int)k);
    ++g_failed;
    return hipErrorInvalidValue;
  }
  g_released.push_back({k, p});
  std::free(p);
  return hipSuccess;
}

size_t live_total() { return g_live[EVENT].size() + g_live[STREAM].size() + g_live[HOST].size() + g_live[DEV].size(); }

}  // namespace

extern "C" {
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return make(EVENT, reinterpret_cast<void**>(e), 1); }
hipError_t hipEventDestroy(hipEvent_t e) {
  g_tick.erase(e);
  return release(EVENT, e);
}
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { return make(STREAM, reinterpret_cast<void**>(s), 1); }
hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned, int) {
  return make(STREAM, reinterpret_cast<void**>(s), 1);
}
hipError_t hipStreamDestroy(hipStream_t s) { return release(STREAM, s); }
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) { return make(HOST, p, bytes); }
hipError_t hipHostFree(void* p) { return release(HOST, p); }
hipError_t hipHostGetDevicePointer(void** d, void* p, unsigned) {
  if (fails_now()) return hipErrorInvalidValue;
  *d = static_cast<char*>(p) + 1;  // (never dereferenced)
  return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t) {
  if (!g_live[EVENT].count(e)) return hipErrorInvalidHandle;
  g_tick[e] = ++g_now;
  return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t e) { return g_live[EVENT].count(e) ? hipSuccess : hipErrorInvalidHandle; }
hipError_t hipEventElapsedTime(float* ms, hipEvent_t a, hipEvent_t b) {
  if (!g_tick.count(a) || !g_tick.count(b)) return hipErrorInvalidHandle;
  *ms = 0.5f * (float)(g_tick[b] - g_tick[a]);
  return hipSuccess;
}
}

namespace gsi {
hipError_t dmalloc(void** p, size_t bytes) { return make(DEV, p, bytes); }
hipError_t dfree(void* p) { return p ? release(DEV, p) : hipSuccess; }
}  // namespace gsi

using gsi::DevBuf;
using gsi::Event;
using gsi::HostBuf;
using gsi::SpanTimer;
using gsi::Stream;

namespace {

constexpr unsigned kMapped = hipHostMallocMapped | hipHostMallocCoherent;

// create, both moves, self-move, reset twice, failed create; fill(x) creates what x holds and
// raw(x) is the handle it converts to
template <class T, class Fill, class Raw>
void test_owner(Kind kind, Fill fill, Raw raw) {
  const size_t before = g_live[kind].size();
  const size_t released = g_released.size();
  {
    T a;
    CHECK(!a && raw(a) == nullptr);
    CHECK(fill(a) == hipSuccess && a && g_live[kind].size() == before + 1);
    void* p = raw(a);
    CHECK(g_live[kind].count(p) == 1);
    T b(std::move(a));  // move construction
    CHECK(!a && raw(b) == p && g_live[kind].size() == before + 1);
    T c;
    CHECK(fill(c) == hipSuccess);
    void* q = raw(c);
    c = std::move(b);  // move assignment onto a full object: q is released, b ends empty
    CHECK(!b && raw(c) == p && g_live[kind].count(q) == 0 && g_live[kind].size() == before + 1);
    T& self = c;
    c = std::move(self);  // self-move keeps it
    CHECK(raw(c) == p && g_live[kind].count(p) == 1);
    CHECK(fill(c) == hipSuccess && g_live[kind].count(p) == 0);  // create on a full object releases first
    p = raw(c);
    c.reset();
    CHECK(!c && g_live[kind].size() == before);
    c.reset();  // empty: nothing to release
    CHECK(g_released.size() == released + 3);
    CHECK(fill(c) == hipSuccess);
    arm(0);
    CHECK(fill(c) != hipSuccess);  // a failed create: what it held is gone, the object empty
    arm(-1);
    CHECK(!c && raw(c) == nullptr && g_live[kind].size() == before);
    CHECK(fill(c) == hipSuccess && c);  // usable afterwards; released at scope exit
  }
  CHECK(g_live[kind].size() == before && live_total() == 0);
}

void test_owners() {
  test_owner<Event>(EVENT, [](Event& e) { return e.create(); }, [](const Event& e) -> void* { return (hipEvent_t)e; });
  test_owner<Stream>(STREAM, [](Stream& s) { return s.create(); },
                     [](const Stream& s) -> void* { return (hipStream_t)s; });
  test_owner<Stream>(STREAM, [](Stream& s) { return s.create_with_priority(hipStreamNonBlocking, -1); },
                     [](const Stream& s) -> void* { return (hipStream_t)s; });
  test_owner<HostBuf<uint32_t>>(HOST, [](HostBuf<uint32_t>& b) { return b.alloc(16, hipHostMallocDefault); },
                                [](const HostBuf<uint32_t>& b) -> void* { return b.get(); });
  test_owner<HostBuf<char>>(HOST, [](HostBuf<char>& b) { return b.alloc(33, kMapped); },
                            [](const HostBuf<char>& b) -> void* { return b.get(); });
  Stream none;  // never created: owns nothing, and a destroy of the null stream would fail the run
  none.reset();
}

void test_hostbuf() {
  HostBuf<uint64_t> b;
  CHECK(b.size() == 0 && b.dev() == nullptr);
  CHECK(b.alloc(9, hipHostMallocDefault) == hipSuccess && b.size() == 9 && b.dev() == nullptr);
  for (size_t i = 0; i < 9; ++i) CHECK(b[i] == 0xA5A5A5A5A5A5A5A5ull);  // staging: left as the fake made it
  b[8] = 7;                                                            // the whole block is writable
  CHECK(b.alloc(5, kMapped) == hipSuccess && b.size() == 5 && b.dev() != nullptr);
  for (size_t i = 0; i < 5; ++i) CHECK(b[i] == 0);  // mapped: zero-filled
  HostBuf<uint64_t> c(std::move(b));  // the mapping and the size move with the block
  CHECK(b.dev() == nullptr && b.size() == 0 && c.dev() != nullptr && c.size() == 5);
  arm(1);  // the block is made, its device mapping cannot be taken
  CHECK(c.alloc(4, kMapped) != hipSuccess);
  arm(-1);
  CHECK(!c && c.dev() == nullptr && c.size() == 0 && g_live[HOST].empty());
  arm(1);  // unmapped: no mapping is asked for, so nothing fails
  CHECK(c.alloc(4, hipHostMallocDefault) == hipSuccess && c);
  arm(-1);
}

// a handle-like struct: a base that holds the stream, then buffers, events and streams, in
// arrays too, created one after the other (kCreates creating calls)
struct Base {
  Stream stream;
  Event ext;
};
struct Lane {
  Stream st;
  Event ev;
};
struct Handle : Base {
  DevBuf<int64_t> tab;
  HostBuf<uint32_t> flags;
  Event ev[2];
  Lane lane[2];
  DevBuf<uint8_t> arr[2];
  HostBuf<char> text;
  static constexpr long kCreates = 14;
  hipError_t fill() {
    hipError_t e;
    if ((e = stream.create()) != hipSuccess) return e;
    if ((e = ext.create()) != hipSuccess) return e;
    if ((e = tab.alloc(64)) != hipSuccess) return e;
    if ((e = flags.alloc(16, kMapped)) != hipSuccess) return e;  // two calls
    for (Event& x : ev)
      if ((e = x.create()) != hipSuccess) return e;
    for (Lane& l : lane) {
      if ((e = l.st.create()) != hipSuccess) return e;
      if ((e = l.ev.create()) != hipSuccess) return e;
    }
    for (auto& x : arr)
      if ((e = x.alloc(8)) != hipSuccess) return e;
    return text.alloc(100, hipHostMallocDefault);
  }
};

void test_handle_after_midway_failure() {
  for (long k = 0; k <= Handle::kCreates; ++k) {  // (k == kCreates: nothing fails)
    CHECK(live_total() == 0);
    g_released.clear();
    void* stream = nullptr;
    {
      Handle* h = new Handle();
      arm(k);
      CHECK((h->fill() == hipSuccess) == (k == Handle::kCreates));
      CHECK(g_seen == (k < Handle::kCreates ? k + 1 : Handle::kCreates));
      arm(-1);
      stream = (hipStream_t)h->stream;
      CHECK((stream != nullptr) == (k > 0));
      delete h;
    }
    CHECK(live_total() == 0);
    // the handle's stream goes last, after every buffer, event and lane
    if (stream) CHECK(!g_released.empty() && g_released.back() == std::make_pair(STREAM, stream));
    if (k == Handle::kCreates) CHECK(g_released.size() == 13);
  }
}

// the first-use rule: a set filled in a local and moved into its place only when complete
struct TextSet {
  HostBuf<char> h_text;
  Event ev[2];
  DevBuf<int64_t> d_src;
  Stream st;
  static constexpr long kCreates = 5;
  bool complete() const { return h_text && ev[0] && ev[1] && d_src && st; }
  bool empty() const { return !h_text && !ev[0] && !ev[1] && !d_src && !st; }
};
hipError_t first_use(TextSet& target) {
  if (target.h_text) return hipSuccess;
  TextSet t;
  hipError_t e;
  if ((e = t.h_text.alloc(40, hipHostMallocDefault)) != hipSuccess) return e;
  for (Event& x : t.ev)
    if ((e = x.create()) != hipSuccess) return e;
  if ((e = t.d_src.alloc(5)) != hipSuccess) return e;
  if ((e = t.st.create()) != hipSuccess) return e;
  target = std::move(t);
  return hipSuccess;
}

void test_first_use() {
  TextSet target;
  for (long k = 0; k < TextSet::kCreates; ++k) {
    arm(k);
    CHECK(first_use(target) != hipSuccess);
    arm(-1);
    CHECK(target.empty() && live_total() == 0);  // as it was: the next call starts from the start
  }
  CHECK(first_use(target) == hipSuccess && target.complete() && live_total() == 5);
  const long made = g_made[EVENT];
  CHECK(first_use(target) == hipSuccess && g_made[EVENT] == made && live_total() == 5);  // not again
}

void test_span_timer() {
  const long made0 = g_made[EVENT];
  constexpr int m = 3;
  {
    SpanTimer t;
    std::map<int, std::vector<float>> got;
    auto note = [&](int id, float ms) { got[id].push_back(ms); };
    for (int round = 0; round < 100; ++round) {
      const int n = 1 + round % m;  // spans pending this round
      std::map<int, float> want;
      for (int i = 0; i < n; ++i) {
        const long start = g_now + 1;  // the tick begin() records at
        hipEvent_t a = t.begin(nullptr);
        CHECK(a != nullptr);
        g_now += i;  // other work on the stream
        t.end(round * m + i, a, nullptr);
        want[round * m + i] = 0.5f * (float)(g_now - start);
      }
      got.clear();
      t.drain(note);
      CHECK(got.size() == (size_t)n);
      for (auto& w : want) CHECK(got[w.first].size() == 1 && got[w.first][0] == w.second);  // once, the fake's time
      got.clear();
      t.drain(note);  // nothing pending: nothing reported
      CHECK(got.empty());
    }
    CHECK(g_made[EVENT] - made0 <= 2 * m);
    CHECK(t.begin(nullptr) != nullptr);  // a start without an end, one cancelled, one never started
    t.cancel(t.begin(nullptr));
    t.end(7, nullptr, nullptr);
    CHECK(g_made[EVENT] - made0 <= 2 * m);
    arm(0);
    CHECK(SpanTimer().begin(nullptr) == nullptr);  // no event to be had: no span
    arm(-1);
    SpanTimer u(std::move(t));  // moves: the events go along
    t = std::move(u);
    SpanTimer& self = t;
    t = std::move(self);
    hipEvent_t a = t.begin(nullptr), b = t.begin(nullptr);
    t.end(1, a, nullptr);
    t.end(2, b, nullptr);
    CHECK(!g_live[EVENT].empty());
  }  // destroyed with spans pending
  CHECK(g_live[EVENT].empty() && live_total() == 0);
}

}  // namespace

int main() {
  test_owners();
  test_hostbuf();
  CHECK(live_total() == 0);
  test_handle_after_midway_failure();
  test_first_use();
  CHECK(live_total() == 0);
  test_span_timer();
  if (g_failed) {
    std::printf("%d checks failed\n", g_failed);
    return 1;
  }
  std::printf("all checks passed (%ld events, %ld streams, %ld host blocks, %ld device blocks)\n", g_made[EVENT],
              g_made[STREAM], g_made[HOST], g_made[DEV]);
  return 0;
}
