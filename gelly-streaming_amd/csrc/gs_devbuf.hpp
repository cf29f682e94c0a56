// gs_devbuf.hpp -- DevBuf<T>: the one owner of a dmalloc'ed device array.
//
// A DevBuf frees what it holds when it goes out of scope, so a handle struct made of them
// needs no pointer list in its destroy function and a function with temporaries needs no
// clean-up on its exit paths. That is all it does: which stream has to be waited for before a
// buffer may be freed, and how a buffer's size is chosen, differ from one scratch group to the
// next and stay with the callers (alloc / reset free at once).
//
// Only the HIP API header and standard headers are read here: a host compiler can build a
// stand-alone check of the type (tests/cpp/devbuf_sanitize.cpp).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

namespace gsi {

// Device memory of summaries and groups: hipMalloc / hipFree plus the per-device byte
// count gs_hbm_bytes reports (tables that grow inside a fold or combine included).
// Defined in gs_capi.cpp.
hipError_t dmalloc(void** p, size_t bytes);
hipError_t dfree(void* p);

template <typename T>
struct DevElem {
  static constexpr size_t bytes = sizeof(T);
};
template <>
struct DevElem<void> {  // DevBuf<void>: a count of bytes
  static constexpr size_t bytes = 1;
};

template <typename T>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_), n_(o.n_) {
    o.p_ = nullptr;
    o.n_ = 0;
  }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      reset();
      swap(o);
    }
    return *this;
  }
  ~DevBuf() { reset(); }

  void reset() {
    (void)dfree(p_);
    p_ = nullptr;
    n_ = 0;
  }
  // Frees what it holds, then allocates exactly `count` elements; empty on failure.
  hipError_t alloc(uint64_t count) {
    reset();
    void* p = nullptr;
    const hipError_t e = dmalloc(&p, (size_t)count * DevElem<T>::bytes);
    if (e != hipSuccess) return e;
    p_ = static_cast<T*>(p);
    n_ = count;
    return hipSuccess;
  }
  void swap(DevBuf& o) noexcept {
    T* p = p_;
    p_ = o.p_;
    o.p_ = p;
    const uint64_t n = n_;
    n_ = o.n_;
    o.n_ = n;
  }
  T* get() const { return p_; }
  operator T*() const { return p_; }
  uint64_t size() const { return n_; }  // elements

 private:
  T* p_ = nullptr;
  uint64_t n_ = 0;
};

}  // namespace gsi
