// devbuf_sanitize.cpp -- stand-alone check of gsi::DevBuf (csrc/gs_devbuf.hpp) under the address
// and undefined-behaviour sanitizers (tests/test_devbuf.py). The program supplies gsi::dmalloc /
// gsi::dfree itself, over malloc / free with a live-byte count and a switch that fails the k-th
// allocation; it makes no HIP runtime call and needs no device.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>

#include "gs_devbuf.hpp"

namespace {

std::map<void*, size_t> g_live;  // block -> bytes
size_t g_live_bytes = 0;
long g_allocs = 0, g_frees = 0;
long g_fail_at = -1;  // the allocation (counted from 0 at arm()) that fails; -1: none
long g_seen = 0;

void arm(long k) {
  g_fail_at = k;
  g_seen = 0;
}

int g_failed = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                                \
    }                                                            \
  } while (0)

}  // namespace

namespace gsi {

hipError_t dmalloc(void** p, size_t bytes) {
  if (g_fail_at >= 0 && g_seen++ == g_fail_at) return hipErrorOutOfMemory;
  *p = std::malloc(bytes ? bytes : 1);
  if (!*p) return hipErrorOutOfMemory;
  g_live[*p] = bytes;
  g_live_bytes += bytes;
  ++g_allocs;
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
  ++g_frees;
  std::free(p);
  return hipSuccess;
}

}  // namespace gsi

using gsi::DevBuf;

namespace {

// a handle-like struct: several buffers allocated one after the other
struct Group {
  DevBuf<int64_t> a, b;
  DevBuf<uint8_t> c;
  DevBuf<void> bytes;
  DevBuf<uint32_t> arr[2];
  hipError_t fill(uint64_t n) {
    hipError_t e;
    if ((e = a.alloc(n)) != hipSuccess) return e;
    if ((e = b.alloc(n)) != hipSuccess) return e;
    if ((e = c.alloc(n)) != hipSuccess) return e;
    if ((e = bytes.alloc(3 * n)) != hipSuccess) return e;
    for (auto& x : arr)
      if ((e = x.alloc(n)) != hipSuccess) return e;
    return hipSuccess;
  }
};

void test_alloc_twice() {
  DevBuf<int64_t> b;
  CHECK(!b && b.get() == nullptr && b.size() == 0);
  CHECK(b.alloc(10) == hipSuccess);
  CHECK(b && b.size() == 10 && g_live_bytes == 80);
  int64_t* first = b;
  first[9] = 7;  // the whole block is writable
  const long frees = g_frees;
  CHECK(b.alloc(20) == hipSuccess);
  CHECK(g_frees == frees + 1);  // the old block, once
  CHECK(g_live.count(first) == 0 || b.get() == first);
  CHECK(b.size() == 20 && g_live_bytes == 160);
  b.get()[19] = 1;
  b.reset();
  CHECK(!b && b.size() == 0 && g_live_bytes == 0);
  b.reset();  // empty: nothing to free
  CHECK(g_frees == frees + 2);
}

void test_failed_alloc() {
  DevBuf<uint32_t> b;
  const size_t before = g_live_bytes;
  arm(0);
  CHECK(b.alloc(100) == hipErrorOutOfMemory);
  arm(-1);
  CHECK(!b && b.size() == 0 && g_live_bytes == before);
  // a failure on a buffer that holds a block: the block is gone, the object empty
  CHECK(b.alloc(5) == hipSuccess && g_live_bytes == before + 20);
  arm(0);
  CHECK(b.alloc(50) == hipErrorOutOfMemory);
  arm(-1);
  CHECK(!b && b.get() == nullptr && b.size() == 0 && g_live_bytes == before);
  CHECK(b.alloc(3) == hipSuccess && b.size() == 3);  // usable afterwards
}

void test_void_counts_bytes() {
  DevBuf<void> b;
  CHECK(b.alloc(123) == hipSuccess);
  CHECK(b.size() == 123 && g_live_bytes == 123);
  void* p = b;
  CHECK(p == b.get() && p != nullptr);
}

void test_moves() {
  const long frees = g_frees;
  {
    DevBuf<int64_t> a;
    CHECK(a.alloc(4) == hipSuccess);
    int64_t* p = a;
    DevBuf<int64_t> b(std::move(a));  // move construction
    CHECK(!a && a.size() == 0 && b.get() == p && b.size() == 4);
    DevBuf<int64_t> c;
    CHECK(c.alloc(6) == hipSuccess);
    int64_t* q = c;
    c = std::move(b);  // move assignment: c's block is freed, b ends empty
    CHECK(g_frees == frees + 1 && g_live.count(q) == 0);
    CHECK(!b && b.size() == 0 && c.get() == p && c.size() == 4);
    DevBuf<int64_t>& self = c;
    c = std::move(self);  // self-assignment keeps the block
    CHECK(c.get() == p && c.size() == 4 && g_live_bytes == 32);
    DevBuf<int64_t> d;
    c = std::move(d);  // from an empty one: c is emptied
    CHECK(!c && g_live_bytes == 0 && g_frees == frees + 2);
  }
  CHECK(g_frees == frees + 2 && g_live_bytes == 0);  // no double free at scope exit
}

void test_swap() {
  DevBuf<uint8_t> a, b;
  CHECK(a.alloc(7) == hipSuccess && b.alloc(9) == hipSuccess);
  uint8_t *pa = a, *pb = b;
  const long frees = g_frees;
  a.swap(b);
  CHECK(a.get() == pb && a.size() == 9 && b.get() == pa && b.size() == 7 && g_frees == frees);
  DevBuf<uint8_t> e;
  a.swap(e);  // with an empty one: the table-rebuild pattern (old table kept aside)
  CHECK(!a && e.get() == pb && e.size() == 9 && g_live_bytes == 16);
}

void test_scope_exit() {
  const size_t before = g_live_bytes;
  {
    DevBuf<int64_t> v, l;
    DevBuf<uint8_t> p;
    CHECK(v.alloc(11) == hipSuccess && l.alloc(11) == hipSuccess && p.alloc(11) == hipSuccess);
    CHECK(g_live_bytes == before + 11 * 17);
  }
  CHECK(g_live_bytes == before);
}

void test_struct_after_midway_failure() {
  CHECK(g_live_bytes == 0);
  for (long k = 0; k < 6; ++k) {
    Group* g = new Group();
    CHECK(g->fill(8) == hipSuccess);  // holds six blocks
    arm(k);
    CHECK(g->fill(32) == hipErrorOutOfMemory);  // the k-th of the regrowth fails
    arm(-1);
    CHECK(g_live_bytes > 0 || k == 0);
    delete g;
    CHECK(g_live_bytes == 0 && g_live.empty());
  }
  {
    Group g;
    arm(3);
    CHECK(g.fill(16) == hipErrorOutOfMemory);
    arm(-1);
    CHECK(g.a && g.b && g.c && !g.bytes && !g.arr[0] && !g.arr[1]);
  }
  CHECK(g_live_bytes == 0 && g_live.empty());
}

}  // namespace

int main() {
  test_alloc_twice();
  CHECK(g_live_bytes == 0);
  test_failed_alloc();
  CHECK(g_live_bytes == 0);
  test_void_counts_bytes();
  CHECK(g_live_bytes == 0);
  test_moves();
  test_swap();
  CHECK(g_live_bytes == 0);
  test_scope_exit();
  test_struct_after_midway_failure();
  CHECK(g_live_bytes == 0 && g_live.empty() && g_allocs == g_frees);
  if (g_failed) {
    std::printf("%d checks failed\n", g_failed);
    return 1;
  }
  std::printf("all checks passed (%ld allocations)\n", g_allocs);
  return 0;
}
