// grow_sanitize.cpp -- stand-alone check of gsi::grow_group / gsi::alloc_each (csrc/gs_grow.hpp)
// under the address and undefined-behaviour sanitizers (tests/test_grow.py). The program
// supplies gsi::dmalloc / gsi::dfree and hipStreamSynchronize itself, over malloc / free with a
// live-byte count, a log of the calls and switches that fail the k-th allocation or the wait; it
// makes no HIP runtime call and needs no device.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>

#include "gs_grow.hpp"

namespace {

std::map<void*, size_t> g_live;  // block -> bytes
size_t g_live_bytes = 0;
std::string g_log;    // one letter per call: W wait, A allocation, F free of a live block
long g_fail_at = -1;  // the allocation (counted from 0 at arm()) that fails; -1: none
long g_seen = 0;
bool g_fail_wait = false;
hipStream_t g_waited = nullptr;

void arm(long k) {
  g_fail_at = k;
  g_seen = 0;
}

int g_failed = 0;
#define CHECK(cond)                                                 \
  do {                                                              \
    if (!(cond)) {                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                                   \
    }                                                               \
  } while (0)

}  // namespace

extern "C" hipError_t hipStreamSynchronize(hipStream_t stream) {
  g_log += 'W';
  g_waited = stream;
  return g_fail_wait ? hipErrorLaunchFailure : hipSuccess;
}

namespace gsi {

hipError_t dmalloc(void** p, size_t bytes) {
  if (g_fail_at >= 0 && g_seen++ == g_fail_at) return hipErrorOutOfMemory;
  *p = std::malloc(bytes ? bytes : 1);
  if (!*p) return hipErrorOutOfMemory;
  g_live[*p] = bytes;
  g_live_bytes += bytes;
  g_log += 'A';
  return hipSuccess;
}

hipError_t dfree(void* p) {
  if (!p) return hipSuccess;
  auto it = g_live.find(p);
  if (it == g_live.end()) {  // a block freed twice, or never allocated here
    std::printf("FAILED: dfree of a block that is not live\n");
    ++g_failed;
    return hipErrorInvalidValue;
  }
  g_live_bytes -= it->second;
  g_live.erase(it);
  g_log += 'F';
  std::free(p);
  return hipSuccess;
}

}  // namespace gsi

using gsi::alloc_each;
using gsi::DevBuf;
using gsi::grow_group;

namespace {

// a scratch group as the handles have them: five buffers of three element types and three sizes
struct Group {
  uint64_t cap = 0;
  DevBuf<int64_t> a, b;  // [cap]
  DevBuf<uint8_t> c;     // [2 cap]
  DevBuf<uint32_t> d;    // [cap / 4 + 1]
  DevBuf<void> bytes;    // [cap] bytes
  static constexpr long kBufs = 5;
  hipStream_t stream = reinterpret_cast<hipStream_t>(0x51);

  hipError_t ensure(uint64_t need) {
    return grow_group(stream, cap, need, need + need / 4, [&](uint64_t n) {
      hipError_t e = alloc_each(n, a, b, bytes);
      if (e == hipSuccess) e = c.alloc(2 * n);
      if (e == hipSuccess) e = d.alloc(n / 4 + 1);
      return e;
    });
  }
  size_t bytes_at(uint64_t n) const { return 8 * n + 8 * n + n + 2 * n + 4 * (n / 4 + 1); }
  bool whole(uint64_t n) const {
    return cap == n && a.size() == n && b.size() == n && bytes.size() == n && c.size() == 2 * n &&
           d.size() == n / 4 + 1;
  }
  void touch() {  // every buffer is writable over its whole size
    a.get()[cap - 1] = 1;
    b.get()[cap - 1] = 2;
    c.get()[2 * cap - 1] = 3;
    d.get()[cap / 4] = 4;
    static_cast<char*>(bytes.get())[cap - 1] = 5;
  }
};

void test_alloc_each() {
  DevBuf<int64_t> x;
  DevBuf<uint8_t> y;
  DevBuf<uint32_t> z;
  CHECK(alloc_each(7) == hipSuccess);  // an empty pack
  CHECK(alloc_each(7, x, y, z) == hipSuccess);
  CHECK(x.size() == 7 && y.size() == 7 && z.size() == 7 && g_live_bytes == 7 * 13);
  arm(1);  // the second fails: the first is reallocated, the third untouched
  CHECK(alloc_each(9, x, y, z) == hipErrorOutOfMemory);
  arm(-1);
  CHECK(x.size() == 9 && !y && z.size() == 7);
}

void test_grows_only_when_it_must() {
  Group g;
  g_log.clear();
  CHECK(g.ensure(100) == hipSuccess);
  CHECK(g.whole(125) && g_live_bytes == g.bytes_at(125));
  CHECK(g_log == "WAAAAA");  // (nothing held yet: no free)
  CHECK(g_waited == g.stream);
  g.touch();
  // large enough: no wait, no allocation, no free
  g_log.clear();
  CHECK(g.ensure(100) == hipSuccess && g.ensure(125) == hipSuccess && g.ensure(0) == hipSuccess);
  CHECK(g_log.empty() && g.whole(125));
  // one more than it holds: exactly one wait, before the first free
  CHECK(g.ensure(126) == hipSuccess);
  CHECK(g.whole(157) && g_live_bytes == g.bytes_at(157));
  CHECK(g_log == "WFAFAFAFAFA");
  g.touch();
}

void test_failed_allocation(long k) {
  Group g;
  CHECK(g.ensure(40) == hipSuccess && g.whole(50));
  g_log.clear();
  arm(k);
  CHECK(g.ensure(51) == hipErrorOutOfMemory);
  arm(-1);
  CHECK(g.cap == 0);  // half-built: the next call rebuilds the whole group
  CHECK(g_log[0] == 'W' && g_log.find('W', 1) == std::string::npos);
  // every live block is one of the group's (nothing leaked), no larger than asked for
  size_t held = 0;
  const void* ptrs[] = {g.a.get(), g.b.get(), g.c.get(), g.d.get(), g.bytes.get()};
  for (const void* p : ptrs)
    if (p) {
      CHECK(g_live.count(const_cast<void*>(p)) == 1);
      held += g_live[const_cast<void*>(p)];
    }
  CHECK(held == g_live_bytes);
  // a need the old capacity covered grows too, now that the group is not whole
  g_log.clear();
  CHECK(g.ensure(10) == hipSuccess);
  CHECK(g.whole(12) && g_live_bytes == g.bytes_at(12) && g_log[0] == 'W');
  g.touch();
  CHECK(g.ensure(300) == hipSuccess && g.whole(375) && g_live_bytes == g.bytes_at(375));
  g.touch();
}

void test_failed_wait() {
  Group g;
  CHECK(g.ensure(8) == hipSuccess && g.whole(10));
  const int64_t* a = g.a;
  g_log.clear();
  g_fail_wait = true;
  CHECK(g.ensure(11) == hipErrorLaunchFailure);
  g_fail_wait = false;
  CHECK(g_log == "W");  // nothing freed, nothing allocated
  CHECK(g.whole(10) && g.a.get() == a && g_live_bytes == g.bytes_at(10));
  g.touch();
  CHECK(g.ensure(11) == hipSuccess && g.whole(13));
}

}  // namespace

int main() {
  test_alloc_each();
  CHECK(g_live_bytes == 0 && g_live.empty());
  test_grows_only_when_it_must();
  CHECK(g_live_bytes == 0 && g_live.empty());
  for (long k = 0; k < Group::kBufs; ++k) {
    test_failed_allocation(k);
    CHECK(g_live_bytes == 0 && g_live.empty());
  }
  test_failed_wait();
  CHECK(g_live_bytes == 0 && g_live.empty());
  if (g_failed) {
    std::printf("%d checks failed\n", g_failed);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
