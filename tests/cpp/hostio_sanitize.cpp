// hostio_sanitize.cpp -- stand-alone check of gsi::ColumnCopy, gsi::OutStage and gsi::FoldStage
// (csrc/gs_hostio.hpp) and of gsi::sort_skip_above (csrc/gs_sort.hpp) under the address and
// undefined-behaviour sanitizers (tests/test_hostio.py). The program supplies gsi::dmalloc /
// gsi::dfree, hipMemcpyAsync and hipStreamSynchronize itself, over malloc / free / memcpy with a
// log of the calls and a switch that fails the k-th allocation: a copy past the end of a staging
// column is a heap overflow the sanitizer reports. It makes no HIP runtime call and needs no device.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "gs_hostio.hpp"
#include "gs_sort.hpp"

namespace {

struct Copy {
  void* dst;
  const void* src;
  size_t bytes;
  hipMemcpyKind kind;
  hipStream_t stream;
};

std::map<void*, size_t> g_live;  // block -> bytes
size_t g_live_bytes = 0;
std::string g_log;  // one letter per call: W wait, A allocation, F free of a live block, C copy
std::vector<Copy> g_copies;
long g_fail_at = -1;  // the allocation (counted from 0 at arm()) that fails; -1: none
long g_seen = 0;
hipStream_t const kStream = reinterpret_cast<hipStream_t>(0x51);

void arm(long k) {
  g_fail_at = k;
  g_seen = 0;
}
void clear_log() {
  g_log.clear();
  g_copies.clear();
}
long count(char c) {
  long n = 0;
  for (char x : g_log) n += x == c;
  return n;
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
  CHECK(stream == kStream);
  return hipSuccess;
}

extern "C" hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t stream) {
  g_log += 'C';
  g_copies.push_back({dst, src, bytes, kind, stream});
  CHECK(stream == kStream);
  std::memcpy(dst, src, bytes);
  return hipSuccess;
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

using gsi::ColumnCopy;
using gsi::DevBuf;
using gsi::FoldStage;
using gsi::OutStage;

namespace {

// ---- ColumnCopy ----

template <class T>
void copy_one(bool to_host, uint64_t rows) {
  DevBuf<T> dev;
  CHECK(dev.alloc(rows) == hipSuccess);
  for (uint64_t i = 0; i < rows; ++i) dev.get()[i] = (T)(i + 3);
  std::vector<T> user(rows, (T)0);
  const ColumnCopy copy(kStream, to_host);
  clear_log();
  CHECK(copy.col((T*)nullptr, dev.get(), rows) == hipSuccess);
  CHECK(g_log.empty());  // a null column queues nothing
  CHECK(copy.col(user.data(), dev.get(), rows) == hipSuccess);
  CHECK(g_log == "C" && g_copies.size() == 1);
  CHECK(g_copies[0].bytes == rows * sizeof(T) && g_copies[0].dst == user.data() && g_copies[0].src == dev.get());
  CHECK(g_copies[0].kind == (to_host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice));
  CHECK(user[rows - 1] == (T)(rows + 2));
}

void test_column_copy() {
  for (int to_host = 0; to_host < 2; ++to_host) {
    copy_one<uint8_t>(to_host, 5);
    copy_one<uint32_t>(to_host, 5);
    copy_one<int64_t>(to_host, 5);
    copy_one<int32_t>(to_host, 3000);
    const ColumnCopy copy(kStream, to_host);
    clear_log();
    CHECK(copy.done() == hipSuccess);
    CHECK(g_log == (to_host ? "W" : ""));  // exactly one wait for host arrays, none otherwise
  }
}

// ---- OutStage ----

void test_out_dev() {
  OutStage s;
  CHECK(s.ensure(3, 4, kStream) == hipSuccess);
  int64_t user[4];
  unsigned long long user_u[4];
  CHECK(s.dev(0, user, false) == user);                                   // a device array: written in place
  CHECK(s.dev(1, user, true) == s.column[1].get() && s.column[1].get());  // a host array: staged
  CHECK(s.dev(2, user_u, true) == reinterpret_cast<unsigned long long*>(s.column[2].get()));
  CHECK(s.dev(2, user_u, false) == user_u);
  CHECK(s.dev(0, (int64_t*)nullptr, true) == nullptr && s.dev(0, (int64_t*)nullptr, false) == nullptr);
}

bool out_whole(const OutStage& s, int cols, uint64_t cap) {
  if (s.cap != cap) return false;
  for (int i = 0; i < OutStage::kMaxCols; ++i)
    if (i < cols ? s.column[i].size() != cap : (bool)s.column[i]) return false;
  return true;
}

void test_out_ensure(int cols, const uint64_t (&rows)[3]) {
  OutStage s;
  uint64_t held = 0;
  for (uint64_t r : rows) {
    clear_log();
    CHECK(s.ensure(cols, r, kStream) == hipSuccess);
    if (r <= held) {
      CHECK(g_log.empty());  // fewer rows: no wait, no allocation, no free
    } else {
      // exactly `cols` columns, one wait, before the first free
      CHECK(count('A') == cols && count('W') == 1 && g_log[0] == 'W' && count('F') == (held ? cols : 0));
      held = r + r / 4;
    }
    CHECK(out_whole(s, cols, held) && g_live_bytes == held * 8 * cols);
    for (int i = 0; i < cols; ++i) s.column[i].get()[held - 1] = i;  // writable over the whole size
  }
}

void test_out_failed_allocation(int cols, long k) {
  OutStage s;
  CHECK(s.ensure(cols, 40, kStream) == hipSuccess && out_whole(s, cols, 50));
  arm(k);
  clear_log();
  CHECK(s.ensure(cols, 51, kStream) == hipErrorOutOfMemory);
  arm(-1);
  CHECK(s.cap == 0);  // half-built
  CHECK(count('W') == 1 && g_log[0] == 'W');
  // a need the old capacity covered rebuilds the whole stage
  clear_log();
  CHECK(s.ensure(cols, 10, kStream) == hipSuccess);
  CHECK(out_whole(s, cols, 12) && count('A') == cols && g_live_bytes == (size_t)12 * 8 * cols);
}

void test_out_finish(uint64_t rows) {
  OutStage s;
  CHECK(s.ensure(4, rows, kStream) == hipSuccess);
  for (int i = 0; i < 4; ++i)
    for (uint64_t r = 0; r < rows; ++r) s.column[i].get()[r] = (int64_t)(1000 * i + r);
  std::vector<int64_t> a(rows, -1), c(rows, -1);
  std::vector<uint64_t> d(rows, 7);
  clear_log();
  CHECK(s.finish(kStream, rows, a.data(), (int64_t*)nullptr, c.data(), d.data()) == hipSuccess);
  CHECK(g_log == "CCCW");  // only the non-null columns, then the one wait
  CHECK(g_copies[0].dst == a.data() && g_copies[0].src == s.column[0].get());
  CHECK(g_copies[1].dst == c.data() && g_copies[1].src == s.column[2].get());
  CHECK(g_copies[2].dst == d.data() && g_copies[2].src == s.column[3].get());
  for (const Copy& cp : g_copies) CHECK(cp.bytes == rows * 8 && cp.kind == hipMemcpyDeviceToHost);
  CHECK(a[rows - 1] == (int64_t)(rows - 1) && c[rows - 1] == (int64_t)(2000 + rows - 1) && d[0] == 3000);
  clear_log();
  CHECK(s.finish(kStream, rows, (int64_t*)nullptr, (int64_t*)nullptr) == hipSuccess);
  CHECK(g_log == "W");  // the wait stands whatever was asked for
}

// ---- FoldStage ----

void test_fold_stage() {
  std::vector<int64_t> hs(900), hd(900), hv(900);
  std::vector<uint8_t> hb(900);
  for (int i = 0; i < 900; ++i) {
    hs[i] = i;
    hd[i] = 5000 + i;
    hv[i] = -i;
    hb[i] = (uint8_t)(i % 3);
  }
  {  // two columns and the byte column
    FoldStage f;
    const int64_t* col[2] = {hs.data(), hd.data()};
    const uint8_t* byte = hb.data();
    clear_log();
    CHECK(f.put(kStream, 100, 1000, col, &byte) == hipSuccess);
    CHECK(f.cap == 125 && f.block.size() == 250 && f.bytes.size() == 125);
    CHECK(g_log == "WAACCC");
    // column i at offset i * cap of the current capacity, not of len
    CHECK(col[0] == f.block.get() && col[1] == f.block.get() + 125 && byte == f.bytes.get());
    CHECK(g_copies[0].bytes == 800 && g_copies[1].bytes == 800 && g_copies[2].bytes == 100);
    CHECK(g_copies[0].src == hs.data() && g_copies[1].src == hd.data() && g_copies[2].src == hb.data());
    for (const Copy& cp : g_copies) CHECK(cp.kind == hipMemcpyHostToDevice);
    CHECK(col[0][99] == 99 && col[1][0] == 5000 && col[1][99] == 5099 && byte[98] == 98 % 3);
    // a second, shorter piece reuses the buffers; without deletion bytes the byte column is not copied
    const int64_t* col2[2] = {hs.data() + 100, hd.data() + 100};
    const uint8_t* none = nullptr;
    clear_log();
    CHECK(f.put(kStream, 40, 1000, col2, &none) == hipSuccess);
    CHECK(g_log == "CC" && none == nullptr);
    CHECK(col2[0] == f.block.get() && col2[1] == f.block.get() + 125 && f.cap == 125);
    CHECK(col2[0][0] == 100 && col2[1][39] == 5139);
    // the clamp: 900 + 225 passes the largest piece
    const int64_t* col3[2] = {hs.data(), hd.data()};
    byte = hb.data();
    clear_log();
    CHECK(f.put(kStream, 900, 1000, col3, &byte) == hipSuccess);
    CHECK(f.cap == 1000 && f.block.size() == 2000 && f.bytes.size() == 1000);
    CHECK(g_log == "WFAFACCC" && col3[1] == f.block.get() + 1000 && col3[1][899] == 5899 && byte[899] == 899 % 3);
    // a piece of exactly the largest size fits what the clamp left
    clear_log();
    CHECK(f.put(kStream, 900, 900, col3, &byte) == hipSuccess && count('A') == 0);
  }
  CHECK(g_live_bytes == 0);
  {  // three columns, no byte column: none is allocated
    FoldStage f;
    const int64_t* col[3] = {hs.data(), hd.data(), hv.data()};
    clear_log();
    CHECK(f.put(kStream, 3, 1000, col) == hipSuccess);
    CHECK(f.cap == 3 && f.block.size() == 9 && !f.bytes && g_log == "WACCC" && g_live_bytes == 72);
    CHECK(col[2] == f.block.get() + 6 && col[2][2] == -2 && col[1][2] == 5002);
    // a failing allocation leaves capacity 0 and queues no copy
    const int64_t* col2[3] = {hs.data(), hd.data(), hv.data()};
    arm(0);
    clear_log();
    CHECK(f.put(kStream, 50, 1000, col2) == hipErrorOutOfMemory);
    arm(-1);
    CHECK(f.cap == 0 && count('C') == 0 && col2[0] == hs.data());
    CHECK(f.put(kStream, 1, 1000, col2) == hipSuccess && f.cap == 1 && col2[1] == f.block.get() + 1);
  }
}

// ---- sort_skip_above ----

void test_skip_above() {
  // skip[p] = bound != 0 && p > 0 && (bound >> (8 * p)) == 0, written out: pass p is character p
  const struct {
    uint64_t bound;
    const char* skip;
  } table[] = {
      {0, "00000000"},          {1, "01111111"},          {255, "01111111"},        {256, "00111111"},
      {257, "00111111"},        {65535, "00111111"},      {65536, "00011111"},      {1ull << 32, "00000111"},
      {1ull << 56, "00000000"}, {1ull << 63, "00000000"},
  };
  static_assert(gs::kSortPasses == 8, "eight digits of a 64-bit key");
  for (const auto& row : table) {
    bool skip[gs::kSortPasses];
    gsi::sort_skip_above(row.bound, skip);
    for (int p = 0; p < 8; ++p) CHECK(skip[p] == (row.skip[p] == '1'));
  }
}

}  // namespace

int main() {
  test_column_copy();
  CHECK(g_live_bytes == 0 && g_live.empty());
  test_out_dev();
  const uint64_t up[3] = {1, 3, 3000}, down[3] = {3000, 3, 1};
  for (int cols = 1; cols <= OutStage::kMaxCols; ++cols) {
    test_out_ensure(cols, up);
    test_out_ensure(cols, down);
    CHECK(g_live_bytes == 0 && g_live.empty());
    for (long k = 0; k < cols; ++k) test_out_failed_allocation(cols, k);
    CHECK(g_live_bytes == 0 && g_live.empty());
  }
  for (uint64_t rows : up) test_out_finish(rows);
  for (uint64_t rows : down) test_out_finish(rows);
  CHECK(g_live_bytes == 0 && g_live.empty());
  test_fold_stage();
  CHECK(g_live_bytes == 0 && g_live.empty());
  test_skip_above();
  if (g_failed) {
    std::printf("%d checks failed\n", g_failed);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
