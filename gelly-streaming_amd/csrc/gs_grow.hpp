// gs_grow.hpp -- grow_group: the one way a handle grows a group of device buffers that share a
// capacity word.
//
// A group is a set of DevBufs sized from one count (scratch of a fold, staging of an export): all
// of them are reallocated together when a call needs more than they hold. Four things have to be
// right each time: the stream that may still use the old buffers is waited for before the first
// one is freed; the capacity word is zero while the group is half-built, so a failed growth
// leaves a group that the next call rebuilds whole; the capacity becomes the new count only when
// every buffer has it; and nothing happens at all while the group is large enough. How the new
// count follows from the need (the growth factor, a clamp) stays with the caller, as do checks
// that are not HIP errors.
//
// Only the HIP API header, standard headers and gs_devbuf.hpp are read here: a host compiler can
// build a stand-alone check (tests/cpp/grow_sanitize.cpp).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "gs_devbuf.hpp"

namespace gsi {

// Every buffer of the pack to `count` elements, in order; stops at the first failure.
inline hipError_t alloc_each(uint64_t) { return hipSuccess; }
template <class Buf, class... Rest>
hipError_t alloc_each(uint64_t count, Buf& first, Rest&... rest) {
  const hipError_t e = first.alloc(count);
  return e != hipSuccess ? e : alloc_each(count, rest...);
}

// Nothing while cap >= need. Otherwise: waits for `stream`, then cap = 0, alloc(new_cap) --
// which allocates every buffer of the group, each from new_cap by its own formula -- and
// cap = new_cap if that succeeded. A failing wait changes nothing.
template <class Alloc>
hipError_t grow_group(hipStream_t stream, uint64_t& cap, uint64_t need, uint64_t new_cap, Alloc alloc) {
  if (cap >= need) return hipSuccess;
  hipError_t e = hipStreamSynchronize(stream);
  if (e != hipSuccess) return e;
  cap = 0;
  if ((e = alloc(new_cap)) == hipSuccess) cap = new_cap;
  return e;
}

}  // namespace gsi
