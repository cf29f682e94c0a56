// gs_distinct_seq.hpp -- everything of the distinct streams (gs_distinct_k.hip) that a host can
// walk: the stamp encodings, the keep predicates, the edge key packing of both modes, the home
// slots, the capacity and growth arithmetic and the tile / scan index arithmetic. Plain
// functions of their arguments with standard headers only: the header compiles with a host
// compiler too (tests/cpp/distinct_seq_sanitize.cpp walks the phases of a fold on the host,
// tables as arrays, against brute force under the address and UB sanitizers).
//
// Monotone stamps. Every occurrence of a key does insert-or-find and then a minimum of its own
// stamp into the slot; stamps only fall. In the NEXT launch an occurrence is the first one when
// the slot's stamp equals its own. A vertex stamp is entry + 1 of the current fold (32 bits,
// meaningful only while the slot has no rank: a vertex of an earlier fold is recognised by its
// rank); an edge stamp is arrival << 1 | swapped over the whole stream (64 bits), so an edge of
// an earlier fold is recognised by stamp >> 1 < folded.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GS_DIST_HD __host__ __device__ inline
#else
#define GS_DIST_HD inline
#endif

namespace gs {

// the values of include/gs_summary.h's gs_distinct_mode
enum DistinctMode : int { kDistDirected = 0, kDistUndirected = 1, kDistModes = 2 };

constexpr int64_t kDistEmptyId = -0x7FFFFFFFFFFFFFFFll - 1;  // INT64_MIN: its vertex lives in the reserved slot
constexpr uint32_t kDistNoRank = 0xFFFFFFFFu;
constexpr uint32_t kDistNoStamp = 0xFFFFFFFFu;
constexpr uint64_t kDistEmptyKey = ~0ull;   // no rank pair: ranks are <= 2^32 - 3
constexpr uint64_t kDistNoEdgeStamp = ~0ull;
// stored slot indices (4 bytes of scratch per entry / edge)
constexpr uint32_t kDistNoSlot = 0xFFFFFFFFu;   // the probe ran over the whole table (overflow)
constexpr uint32_t kDistOldEdge = 0xFFFFFFFEu;  // the edge was folded by an earlier fold: dropped
// limits
constexpr uint64_t kDistMaxFold = 0x7FFFFFFEull;      // edges per fold: entry + 1 fits 32 bits
constexpr uint64_t kDistMaxVertices = 0xFFFFFFFEull;  // ranks 0 .. 2^32 - 3
constexpr uint64_t kDistMinSlots = 1024;
constexpr uint64_t kDistMaxSlots = 1ull << 31;        // a stored slot index has 32 bits

// ---- entries: entry e of a fold is one endpoint of edge e >> 1, src (even) before dst (odd)
GS_DIST_HD uint64_t dist_entry_edge(uint64_t e) { return e >> 1; }
GS_DIST_HD bool dist_entry_is_dst(uint64_t e) { return (e & 1ull) != 0; }

// ---- vertex stamps
GS_DIST_HD uint32_t dist_vertex_stamp(uint64_t e) { return (uint32_t)(e + 1); }
// no atomic needed: the loaded slot shows a vertex of an earlier fold, or a stamp not above mine
GS_DIST_HD bool dist_vertex_skip(uint32_t rank, uint32_t stamp, uint32_t mine) {
  return rank != kDistNoRank || stamp <= mine;
}
// (next launch) entry e is the first occurrence of a new vertex
GS_DIST_HD bool dist_vertex_keep(uint32_t rank, uint32_t stamp, uint64_t e) {
  return rank == kDistNoRank && stamp == dist_vertex_stamp(e);
}

// ---- edge keys and stamps
// key = rank(src) << 32 | rank(dst); undirected: (smaller rank, larger rank), *swapped = the
// arrival had the larger rank first
GS_DIST_HD uint64_t dist_edge_key(uint32_t rs, uint32_t rd, int mode, bool* swapped) {
  const bool sw = mode == kDistUndirected && rs > rd;
  *swapped = sw;
  const uint32_t a = sw ? rd : rs, b = sw ? rs : rd;
  return ((uint64_t)a << 32) | (uint64_t)b;
}
// the ranks of the arrival's src and dst
GS_DIST_HD void dist_key_ranks(uint64_t key, bool swapped, uint32_t* rs, uint32_t* rd) {
  const uint32_t a = (uint32_t)(key >> 32), b = (uint32_t)key;
  *rs = swapped ? b : a;
  *rd = swapped ? a : b;
}
GS_DIST_HD uint64_t dist_edge_stamp(uint64_t arrival, bool swapped) { return (arrival << 1) | (swapped ? 1ull : 0ull); }
GS_DIST_HD uint64_t dist_stamp_arrival(uint64_t stamp) { return stamp >> 1; }
GS_DIST_HD bool dist_stamp_swapped(uint64_t stamp) { return (stamp & 1ull) != 0; }
// the slot's edge arrived in an earlier fold (kDistNoEdgeStamp >> 1 is above every arrival)
GS_DIST_HD bool dist_edge_old(uint64_t stamp, uint64_t folded) { return dist_stamp_arrival(stamp) < folded; }
GS_DIST_HD bool dist_edge_skip(uint64_t stamp, uint64_t mine) { return stamp <= mine; }
// (next launch) the occurrence of arrival number `arrival` is the first of its key
GS_DIST_HD bool dist_edge_keep(uint64_t stamp, uint64_t arrival) { return dist_stamp_arrival(stamp) == arrival; }

// ---- home slots of a table of 2^(64 - shift) slots
// vertices: as the main table's hash (gs_device.hpp hash_slot): ids that differ only in their
// low 3 bits share one 128-byte line of 8 slots
GS_DIST_HD uint32_t dist_vertex_home(int64_t id, int shift) {
  return ((uint32_t)((((uint64_t)id >> 3) * 0x9E3779B97F4A7C15ull) >> (shift + 3)) << 3) | (uint32_t)(id & 7);
}
// edges: a rank pair is two small numbers, so all its bits are mixed (splitmix64's finaliser)
GS_DIST_HD uint32_t dist_edge_home(uint64_t key, int shift) {
  uint64_t z = key + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (uint32_t)(z >> shift);
}

// ---- capacity and growth: open addressing, linear probing, load <= 1/2
GS_DIST_HD uint64_t dist_pow2_ceil(uint64_t x) {
  uint64_t p = 1;
  while (p < x) p <<= 1;
  return p;
}
GS_DIST_HD int dist_log2(uint64_t pow2) {
  int l = 0;
  while ((1ull << l) < pow2) ++l;
  return l;
}
// slots of a table that holds `count` keys at load <= 1/2 (min_slots: a power of two >= 16, the
// home slot of a vertex has 3 line bits; the host walk uses small tables)
GS_DIST_HD uint64_t dist_slots_for(uint64_t count, uint64_t min_slots = kDistMinSlots) {
  const uint64_t s = dist_pow2_ceil(2 * count);
  return s < min_slots ? min_slots : s;
}
// a fold of n edges adds at most 2 n vertices and n edges
GS_DIST_HD uint64_t dist_worst_vertices(uint64_t n) { return 2 * n; }
GS_DIST_HD uint64_t dist_worst_edges(uint64_t n) { return n; }
// decided before the fold from host-known totals
GS_DIST_HD bool dist_must_grow(uint64_t count, uint64_t worst, uint64_t cap) { return count + worst > cap / 2; }
// ranks a vertex table of cap slots can hand out (the vertex list beside it)
GS_DIST_HD uint64_t dist_vid_cap(uint64_t cap) { return cap / 2; }

// ---- tiles: positions 0 .. n - 1 cut into tiles of `tile`; the flag kernel strides over a tile
// (position k * bs + thread), the write kernel gives a thread `per` consecutive positions
GS_DIST_HD uint64_t dist_tiles(uint64_t n, uint32_t tile) { return (n + tile - 1) / tile; }
GS_DIST_HD uint64_t dist_tile_begin(uint64_t t, uint32_t tile) { return t * (uint64_t)tile; }
GS_DIST_HD uint64_t dist_flag_pos(uint64_t t, uint32_t tile, uint32_t bs, uint32_t k, uint32_t thread) {
  return dist_tile_begin(t, tile) + (uint64_t)k * bs + thread;
}
GS_DIST_HD uint64_t dist_write_first(uint64_t t, uint32_t tile, uint32_t per, uint32_t thread) {
  return dist_tile_begin(t, tile) + (uint64_t)thread * per;
}
// output row of a kept position: kept before its tile + kept before it inside the tile
GS_DIST_HD uint64_t dist_out_row(uint64_t tile_base, uint32_t before_in_tile) { return tile_base + before_in_tile; }

}  // namespace gs
