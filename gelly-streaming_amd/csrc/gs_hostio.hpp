// gs_hostio.hpp -- the host-array forms of the stand-alone summaries: how rows reach a caller's
// arrays and how a host fold's columns reach the device.
//
// Every export has a device form and a host form that differ only in where the rows end. Rows
// that already lie in device arrays go through a ColumnCopy: one copy per column the caller asked
// for, one wait when the arrays are host arrays. Rows a kernel writes go through an OutStage: the
// kernel writes the caller's device arrays, or staging columns that are copied out afterwards. A
// host fold goes through a FoldStage: its columns are copied into one device block, piece by
// piece. None of them decides what is launched or when; the handles keep that.
//
// Only the HIP API header, standard headers, gs_devbuf.hpp and gs_grow.hpp are read here: a host
// compiler can build a stand-alone check (tests/cpp/hostio_sanitize.cpp).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "gs_devbuf.hpp"
#include "gs_grow.hpp"

namespace gsi {

// Columns that lie in device arrays, copied to the caller's arrays: device arrays, or host arrays
// (to_host) that done() waits for.
struct ColumnCopy {
  hipStream_t stream;
  bool to_host;
  ColumnCopy(hipStream_t s, bool host) : stream(s), to_host(host) {}

  // nothing for a null dst (a column the caller does not want)
  template <class T>
  hipError_t col(T* dst, const T* src, uint64_t rows) const {
    if (!dst) return hipSuccess;
    return hipMemcpyAsync(dst, src, rows * sizeof(T), to_host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, stream);
  }
  hipError_t done() const { return to_host ? hipStreamSynchronize(stream) : hipSuccess; }
};

// Device staging of an export whose rows a kernel writes: up to four columns of 8-byte elements
// behind one capacity word.
struct OutStage {
  static constexpr int kMaxCols = 4;
  uint64_t cap = 0;  // rows every allocated column holds
  DevBuf<int64_t> column[kMaxCols];

  // the first `cols` columns for `rows` rows, with a quarter of headroom (grow_group)
  hipError_t ensure(int cols, uint64_t rows, hipStream_t stream) {
    return grow_group(stream, cap, rows, rows + rows / 4, [&](uint64_t c) {
      hipError_t e = hipSuccess;
      for (int i = 0; i < cols && e == hipSuccess; ++i) e = column[i].alloc(c);
      return e;
    });
  }
  // where the kernel writes column i: the caller's device array, staging column i for a host
  // array, null for a column the caller does not want
  template <class T>
  T* dev(int i, T* user, bool to_host) const {
    static_assert(sizeof(T) == 8, "a staging column holds 8-byte elements");
    return to_host && user ? reinterpret_cast<T*>(column[i].get()) : user;
  }
  // staging column i to host[i] for every non-null one, then the one wait
  template <class... T>
  hipError_t finish(hipStream_t stream, uint64_t rows, T*... host) const {
    static_assert(sizeof...(T) <= kMaxCols, "at most four columns");
    void* const to[] = {host...};
    for (int i = 0; i < (int)sizeof...(T); ++i) {
      if (!to[i]) continue;
      const hipError_t e = hipMemcpyAsync(to[i], column[i], rows * 8, hipMemcpyDeviceToHost, stream);
      if (e != hipSuccess) return e;
    }
    return hipStreamSynchronize(stream);
  }
};

// Device staging of a host fold: k int64_t columns in one block, column i at offset i * cap, and
// a byte column for the handles that take one.
struct FoldStage {
  uint64_t cap = 0;  // rows per column
  DevBuf<int64_t> block;  // [k][cap]
  DevBuf<uint8_t> bytes;  // [cap], only with a byte column

  // A piece of len host rows: the stage grows to min(max_piece, len + len / 4) if it must
  // (grow_group), col[0 .. K) are copied in and become their device addresses. byte: null for a
  // handle without a byte column; else *byte is copied and replaced likewise unless it is null.
  // The copies are queued, not waited for.
  template <int K>
  hipError_t put(hipStream_t stream, uint64_t len, uint64_t max_piece, const int64_t* (&col)[K],
                 const uint8_t** byte = nullptr) {
    const uint64_t want = len + len / 4;
    hipError_t e = grow_group(stream, cap, len, want < max_piece ? want : max_piece, [&](uint64_t c) {
      const hipError_t a = block.alloc(K * c);
      return a != hipSuccess || !byte ? a : bytes.alloc(c);
    });
    for (int i = 0; i < K && e == hipSuccess; ++i) {
      int64_t* const to = block.get() + i * cap;
      e = hipMemcpyAsync(to, col[i], len * 8, hipMemcpyHostToDevice, stream);
      col[i] = to;
    }
    if (e == hipSuccess && byte && *byte) {
      e = hipMemcpyAsync(bytes, *byte, len, hipMemcpyHostToDevice, stream);
      *byte = bytes;
    }
    return e;
  }
};

}  // namespace gsi
