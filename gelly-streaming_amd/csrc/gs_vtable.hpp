// gs_vtable.hpp -- VertexTable: the owner of the distinct streams' vertex table (gs_distinct.hpp:
// DistVSlot, launch_dist_vertices) and of the vertex list beside it, and the one way it grows.
// The distinct streams (gs_distinct.cpp), the weighted matching (gs_matching.cpp), which keeps
// one state record per rank next to the list, the degree streams (gs_degstream.cpp), which keep
// one degree per rank there, and the triangle streams (gs_tristream.cpp), which keep one 64-bit
// triangle counter per rank there, derive their handles from it. Host only.
#pragma once
#include "gs_distinct.hpp"
#include "gs_internal.hpp"

namespace gsi {

struct VertexTable {
  DevBuf<gs::DistVSlot> vtab;  // [vcap + 1]
  DevBuf<int64_t> vid;         // [dist_vid_cap(vcap)] vertices in rank order
  uint64_t vcap = 0;

  gs::DistVTable vtable() const { return gs::dist_vtable_of(vtab, vcap); }

  // A table of new_cap slots and its vertex list in place of the current ones, whose nv vertices
  // move over (a rank is the same before and after); the first table of a handle when there is
  // none. ctl: the DistCtl words the rebuild reports into. extra(rebuild) runs once the rebuild
  // is queued and before the one wait for `stream` that precedes the release of the old arrays:
  // what a handle keeps per rank is allocated, initialised and copied there (rebuild: there is an
  // old table). A failure, an allocation's or extra's, leaves the old table in place.
  template <class Extra>
  int grow(uint64_t new_cap, uint64_t nv, unsigned long long* ctl, hipStream_t stream, Extra extra) {
    DevBuf<gs::DistVSlot> tab;
    DevBuf<int64_t> ids;
    GS_HIP(tab.alloc(new_cap + 1));
    GS_HIP(ids.alloc(gs::dist_vid_cap(new_cap)));
    const gs::DistVTable to = gs::dist_vtable_of(tab, new_cap);
    const bool rebuild = vtab;
    GS_LAUNCH(gs::launch_dist_init(to, stream));
    if (rebuild) {
      GS_LAUNCH(gs::launch_dist_rebuild(vtable(), to, ctl, stream));
      if (nv) GS_HIP(hipMemcpyAsync(ids, vid, nv * 8, hipMemcpyDeviceToDevice, stream));
    }
    if (int rc = extra(rebuild)) return rc;
    if (rebuild) GS_HIP(hipStreamSynchronize(stream));  // before the old arrays are freed
    vtab.swap(tab);
    vid.swap(ids);
    vcap = new_cap;
    return GS_OK;
  }
};

}  // namespace gsi
