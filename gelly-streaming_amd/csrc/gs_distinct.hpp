// gs_distinct.hpp -- host-side launchers of the distinct streams' kernels (gs_distinct_k.hip):
// the first-seen vertices and edges of an edge stream (SimpleEdgeStream.distinct / getVertices).
// Every launch is queued on the given stream; kernel boundaries carry all ordering between
// workgroups (no workgroup waits on another inside a launch).
//
// State. Two open-addressing tables of 16-byte slots, linear probing at
// load <= 1/2:
//   vertex slot { int64 id | uint32 rank | uint32 stamp }, initially { EMPTY, NONE, UINT32_MAX };
//               slot `cap`, one past the hashed range, is reserved for INT64_MIN
//   edge slot   { uint64 key | uint64 stamp }, key = rank(src) << 32 | rank(dst) (undirected:
//               smaller rank first), initially all ones
// and beside them vid[rank], the vertices in rank order, plus the scratch of the last fold: the
// slot index of every entry and edge, one flag byte per position, the tile counts, and the kept
// entry / edge indices. The arithmetic is gs_distinct_seq.hpp's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gs_distinct_seq.hpp"

namespace gs {

// Positions per workgroup of the flag and write kernels (gsamd.DISTINCT_TILE).
constexpr uint32_t DISTINCT_TILE = 2048;
constexpr uint32_t kDistBS = 256;                         // threads of every workgroup
constexpr uint32_t kDistPer = DISTINCT_TILE / kDistBS;    // consecutive positions per thread
static_assert(DISTINCT_TILE == kDistBS * kDistPer, "tile = threads x positions per thread");
static_assert(kDistPer == 8, "a thread's flags are the 8 bytes of one 64-bit word");

struct alignas(16) DistVSlot {
  int64_t id;
  uint32_t rank;
  uint32_t stamp;
};
struct alignas(16) DistESlot {
  unsigned long long key;
  unsigned long long stamp;
};
struct DistVTable {
  DistVSlot* tab;  // [cap + 1]
  uint32_t cap;    // hashed slots (a power of two); the reserved slot's index
  uint32_t mask;
  int shift;       // 64 - log2(cap)
};
// the view of a vertex table of `cap` hashed slots (a power of two) at tab[cap + 1]
inline DistVTable dist_vtable_of(DistVSlot* tab, uint64_t cap) {
  DistVTable t;
  t.tab = tab;
  t.cap = (uint32_t)cap;
  t.mask = (uint32_t)(cap - 1);
  t.shift = 64 - dist_log2(cap);
  return t;
}
struct DistETable {
  DistESlot* tab;  // [cap]
  uint32_t cap;
  uint32_t mask;
  int shift;
};

// control words (uint64) of a handle
enum DistCtl : int {
  DIST_NEW_V = 0,     // new vertices of the fold
  DIST_NEW_E = 1,     // new edges of the fold
  DIST_OVERFLOW = 2,  // a probe ran over a whole table, or an index was out of range
  DIST_PROBE = 3,     // the longest probe of the fold, in slots past home
  DIST_EXPORT = 4,    // append position of the edge export
  DIST_ATOMICS = 5,   // profiled folds only: occurrences that issued an atomic minimum
  DIST_CTL_WORDS = 8
};

// every slot of a vertex table (cap + 1) / an edge table (cap) to its initial value
void launch_dist_init(const DistVTable& vt, hipStream_t st);
void launch_dist_init(const DistETable& et, hipStream_t st);
// every occupied slot of `from` into the initialised, larger `to`, payload included
void launch_dist_rebuild(const DistVTable& from, const DistVTable& to, unsigned long long* ctl, hipStream_t st);
void launch_dist_rebuild(const DistETable& from, const DistETable& to, unsigned long long* ctl, hipStream_t st);

// Phases 1 and 2 of a fold of n edges (edge i = src[i * stride], dst[i * stride]): insert-or-find
// and stamp every entry, then flag, scan and write the new vertices: vid[v0 + k], entry[k], the
// slot's rank = v0 + k; ctl[DIST_NEW_V] = their number. vslot holds 2 n words, flags whole tiles
// of 2 n positions, tbase tiles + 1 words.
void launch_dist_vertices(const int64_t* src, const int64_t* dst, uint64_t n, uint64_t stride, const DistVTable& vt,
                          uint32_t* vslot, uint8_t* flags, uint32_t* tbase, uint64_t v0, int64_t* vid,
                          uint64_t vid_cap, uint32_t* entry, unsigned long long* ctl, hipStream_t st,
                          hipEvent_t mid = nullptr);
// Phases 3 and 4: key every edge by its endpoints' ranks, insert-or-find and stamp it, then flag,
// scan and write the kept edge indices ascending: index[k]; ctl[DIST_NEW_E] = their number.
// mid (both launchers, profiled folds): recorded between the probe kernel and the compaction, and
// the probe kernel then counts its atomics into ctl[DIST_ATOMICS].
void launch_dist_edges(uint64_t n, uint64_t folded, int mode, const DistVTable& vt, const uint32_t* vslot,
                       const DistETable& et, uint32_t* eslot, uint8_t* flags, uint32_t* tbase, uint32_t* index,
                       unsigned long long* ctl, hipStream_t st, hipEvent_t mid = nullptr);

// src[k], dst[k] (either may be null) of the last fold's kept edges k < ne, decoded from their slots
void launch_dist_new_edges(const uint32_t* index, uint64_t ne, const uint32_t* eslot, uint64_t n, const DistETable& et,
                           const int64_t* vid, uint64_t nv, int64_t* src, int64_t* dst, hipStream_t st);
// the occupied slots of the edge table appended to (stamp[], key[]) in any order, at most cap rows
void launch_dist_export(const DistETable& et, int64_t* stamp, unsigned long long* key, uint64_t cap,
                        unsigned long long* ctl, hipStream_t st);
// rows sorted by stamp: skey[i] = stamp ^ sign bit, pay[i] = its row in key[]; src / dst / first may be null
void launch_dist_decode(const unsigned long long* skey, const uint32_t* pay, const unsigned long long* key, uint64_t ne,
                        const int64_t* vid, uint64_t nv, int64_t* src, int64_t* dst, unsigned long long* first,
                        hipStream_t st);
// read-only probes
void launch_dist_rank(const DistVTable& vt, const int64_t* v, uint64_t n, int64_t* rank, uint8_t* found, hipStream_t st);
void launch_dist_contains(const DistVTable& vt, const DistETable& et, int mode, const int64_t* src, const int64_t* dst,
                          uint64_t n, uint8_t* found, hipStream_t st);

}  // namespace gs
