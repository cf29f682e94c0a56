// gs_vtable.hpp -- VertexTable: the owner of the distinct streams' vertex table (gs_distinct.hpp:
// DistVSlot, launch_dist_vertices), of the vertex list beside it and of the count of vertices in
// them; the one way it grows, the capacity check a fold makes before any device work and the
// growth decision that opens a fold. The distinct streams (gs_distinct.cpp), the weighted
// matching (gs_matching.cpp), which keeps one state record per rank next to the list, the degree
// streams (gs_degstream.cpp), which keep one degree per rank there, and the triangle streams
// (gs_tristream.cpp), which keep one 64-bit triangle counter per rank there, derive their handles
// from it. Host only.
#pragma once
#include <string>

#include "gs_distinct.hpp"
#include "gs_internal.hpp"

namespace gsi {

struct VertexTable {
  DevBuf<gs::DistVSlot> vtab;  // [vcap + 1]
  DevBuf<int64_t> vid;         // [dist_vid_cap(vcap)] vertices in rank order
  uint64_t vcap = 0;
  uint64_t nv = 0;  // ids in the table (host-known: a fold reads the count of its new ones)

  gs::DistVTable vtable() const { return gs::dist_vtable_of(vtab, vcap); }

  // What a fold of n edges, folded in pieces of at most `piece`, checks before any device work:
  // the worst case (two new vertices an edge) fits the rank range, and the table a piece may have
  // to grow to fits the slot range. what: the summary's name in the message.
  int fold_guard_vertices(uint64_t n, uint64_t piece, const char* what) const {
    if (nv + gs::dist_worst_vertices(n) > gs::kDistMaxVertices ||
        (gs::dist_must_grow(nv, gs::dist_worst_vertices(piece), vcap) &&
         gs::dist_slots_for(nv + gs::dist_worst_vertices(piece)) > gs::kDistMaxSlots))
      return fail(GS_ERR_CAPACITY, std::string(what) + " fold: the fold may pass 2^31 vertex table slots");
    return GS_OK;
  }

  // The top of a fold of n edges: grow_fn(slots) -- the handle's own growth, which ends in grow()
  // -- if the worst case of the fold would pass the table's load limit. Nothing grows after it.
  template <class Grow>
  int ensure_for(uint64_t n, Grow grow_fn) {
    if (!gs::dist_must_grow(nv, gs::dist_worst_vertices(n), vcap)) return GS_OK;
    return grow_fn(gs::dist_slots_for(nv + gs::dist_worst_vertices(n)));
  }

  // A table of new_cap slots and its vertex list in place of the current ones, whose nv vertices
  // move over (a rank is the same before and after); the first table of a handle when there is
  // none. ctl: the DistCtl words the rebuild reports into. extra(rebuild) runs once the rebuild
  // is queued and before the one wait for `stream` that precedes the release of the old arrays:
  // what a handle keeps per rank is allocated, initialised and copied there (rebuild: there is an
  // old table). A failure, an allocation's or extra's, leaves the old table in place.
  template <class Extra>
  int grow(uint64_t new_cap, unsigned long long* ctl, hipStream_t stream, Extra extra) {
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

  // grow() for a handle that keeps one T per rank, zero for a rank not yet given out: per_rank
  // becomes [dist_vid_cap(new_cap)], zero-filled, the nv old values moved over, inside the same wait.
  template <class T>
  int grow_ranked(uint64_t new_cap, unsigned long long* ctl, hipStream_t stream, DevBuf<T>& per_rank) {
    DevBuf<T> fresh;
    const uint64_t ranks = gs::dist_vid_cap(new_cap);
    const int rc = grow(new_cap, ctl, stream, [&](bool rebuild) -> int {
      GS_HIP(fresh.alloc(ranks));
      GS_HIP(hipMemsetAsync(fresh, 0, ranks * sizeof(T), stream));
      if (rebuild && nv) GS_HIP(hipMemcpyAsync(fresh, per_rank, nv * sizeof(T), hipMemcpyDeviceToDevice, stream));
      return GS_OK;
    });
    if (rc) return rc;
    per_rank.swap(fresh);
    return GS_OK;
  }
};

}  // namespace gsi
