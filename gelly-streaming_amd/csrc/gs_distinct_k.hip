// gs_distinct_k.hip -- kernels of the distinct streams (gfx950).
//
//   k_dist_vinit / k_dist_einit     : a table's slots to their initial values
//   k_dist_vrebuild / k_dist_erebuild : every occupied slot of the old table into the new one
//   k_dist_vertices : phase 1. One entry per thread: insert-or-find of its id, a minimum of
//                     entry + 1 into the slot's stamp unless the loaded slot already shows a rank
//                     (a vertex of an earlier fold: the steady state issues no atomic) or a stamp
//                     that is not larger; the slot index goes to scratch
//   k_dist_flag<1>  : phase 2. One flag byte per entry (new: no rank, stamp == entry + 1), kept
//                     positions per tile
//   k_dist_vwrite   : the new vertices in entry order: vid[], entry[], the slot's rank; between
//                     a flag and a write kernel, the sort's launch_tile_scan turns the tile
//                     counts into tile bases and the total
//   k_dist_edges    : phase 3. One edge per thread: the two ranks through the stored slot
//                     indices, the key, insert-or-find, a minimum of arrival << 1 | swapped into
//                     the stamp; an edge of an earlier fold is dropped without an atomic
//   k_dist_flag<0>  : phase 4. One flag byte per edge (new: stamp >> 1 == its arrival)
//   k_dist_ewrite   : the kept edge indices ascending
//   k_dist_new_edges / k_dist_export / k_dist_decode : the emissions and the whole edge set
//   k_dist_rank / k_dist_contains   : read-only probes
// Encodings, predicates, key packing, home slots and tile arithmetic are gs_distinct_seq.hpp's;
// the tile count and the rank inside a tile are gs_scan.hpp's.
//
// Concurrency (gs_device.hpp's rules). Correctness never depends on a plain load being fresh: a
// key changes once, EMPTY -> k, by 64-bit CAS, and a stale EMPTY is settled by the CAS's
// return; a stamp only falls, by atomic minimum, so a stale stamp can only cause a superfluous
// atomic. Whether an occurrence is the first is read in the NEXT launch. Nobody waits.
//
// What bounds every loop and index:
//   * per-element kernels handle one element per thread, its index tested against the count;
//   * every probe loop runs at most cap iterations and raises ctl[DIST_OVERFLOW] instead of
//     running on; the stored slot index is then kDistNoSlot;
//   * a stored slot index is tested against its table's slot count, a rank against the vertex
//     list's fill, a sort payload against the row count, before any is used as an index;
//   * tile kernels handle kDistPer positions per thread, each tested against the count; a flag
//     word is read inside the flag array's whole tiles (the flag kernels wrote all of them);
//   * every output row is tested against the capacity of its array before the store.
// No workgroup waits on another. No kernel reads what another workgroup of the same launch
// writes, except through the atomics above (the write kernels set ranks that only later
// launches read).
#include "gs_distinct.hpp"
#include "gs_distinct_seq.hpp"
#include "gs_scan.hpp"
#include "gs_sort.hpp"

namespace gs {
namespace {

__device__ __forceinline__ void load_vslot(const DistVSlot* p, int64_t& id, uint32_t& rank, uint32_t& stamp) {
  const uint4 v = *reinterpret_cast<const uint4*>(p);  // one 16-byte load: key and payload together
  id = (int64_t)(((uint64_t)v.y << 32) | v.x);
  rank = v.z;
  stamp = v.w;
}

__device__ __forceinline__ void load_eslot(const DistESlot* p, unsigned long long& key, unsigned long long& stamp) {
  const uint4 v = *reinterpret_cast<const uint4*>(p);
  key = ((unsigned long long)v.y << 32) | v.x;
  stamp = ((unsigned long long)v.w << 32) | v.z;
}

__device__ __forceinline__ void raise_overflow(unsigned long long* ctl) { atomicOr(ctl + DIST_OVERFLOW, 1ull); }

// The longest probe: every lane of the wave calls this (wave-uniform control flow); one atomic
// per wave, issued only when one of its probes left its home slot.
__device__ __forceinline__ void note_probe(unsigned long long* ctl, uint32_t probes) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t y = __shfl_xor(probes, o, 64);
    probes = y > probes ? y : probes;
  }
  if ((threadIdx.x & 63u) == 0 && probes) atomicMax(ctl + DIST_PROBE, (unsigned long long)probes);
}

// Profiled folds: the wave's occurrences that issued an atomic minimum (every lane calls this).
__device__ __forceinline__ void note_atomics(unsigned long long* ctl, bool issued) {
  const unsigned long long m = __ballot(issued);
  if ((threadIdx.x & 63u) == 0 && m) atomicAdd(ctl + DIST_ATOMICS, (unsigned long long)__popcll(m));
}

// Insert-or-find of a vertex id: its slot, or kDistNoSlot. rank / stamp: what the load showed
// (no rank, no stamp for a slot claimed or met through the CAS: it is of this launch).
__device__ __forceinline__ uint32_t vertex_insert(const DistVTable& t, int64_t id, uint32_t& rank, uint32_t& stamp,
                                                  uint32_t& probes) {
  int64_t k;
  if (id == kDistEmptyId) {  // the reserved slot: always "found", its rank says whether it is a vertex
    load_vslot(t.tab + t.cap, k, rank, stamp);
    return t.cap;
  }
  uint32_t h = dist_vertex_home(id, t.shift) & t.mask;
  for (uint32_t p = 0; p <= t.mask; ++p) {
    load_vslot(t.tab + h, k, rank, stamp);
    if (k == id) {
      probes = p;
      return h;
    }
    if (k == kDistEmptyId) {
      const unsigned long long old = atomicCAS((unsigned long long*)&t.tab[h].id, (unsigned long long)kDistEmptyId,
                                               (unsigned long long)id);
      if (old == (unsigned long long)kDistEmptyId || (int64_t)old == id) {
        rank = kDistNoRank;
        stamp = kDistNoStamp;
        probes = p;
        return h;
      }
    }
    h = (h + 1) & t.mask;
  }
  return kDistNoSlot;
}

// Read-only: the slot of id, or kDistNoSlot; rank = its rank (kDistNoRank: not a vertex).
__device__ __forceinline__ uint32_t vertex_find(const DistVTable& t, int64_t id, uint32_t& rank) {
  int64_t k;
  uint32_t stamp;
  if (id == kDistEmptyId) {
    load_vslot(t.tab + t.cap, k, rank, stamp);
    return rank == kDistNoRank ? kDistNoSlot : t.cap;
  }
  uint32_t h = dist_vertex_home(id, t.shift) & t.mask;
  for (uint32_t p = 0; p <= t.mask; ++p) {
    load_vslot(t.tab + h, k, rank, stamp);
    if (k == id) return rank == kDistNoRank ? kDistNoSlot : h;
    if (k == kDistEmptyId) break;
    h = (h + 1) & t.mask;
  }
  rank = kDistNoRank;
  return kDistNoSlot;
}

constexpr uint32_t kDistInitPer = 4;  // slots per thread of the init kernels

__global__ __launch_bounds__(kDistBS) void k_dist_vinit(DistVSlot* tab, uint64_t slots) {
  const uint64_t s0 = ((uint64_t)blockIdx.x * kDistBS + threadIdx.x) * kDistInitPer;
  DistVSlot v;
  v.id = kDistEmptyId;
  v.rank = kDistNoRank;
  v.stamp = kDistNoStamp;
#pragma unroll
  for (uint32_t k = 0; k < kDistInitPer; ++k)
    if (s0 + k < slots) tab[s0 + k] = v;
}

__global__ __launch_bounds__(kDistBS) void k_dist_einit(DistESlot* tab, uint64_t slots) {
  const uint64_t s0 = ((uint64_t)blockIdx.x * kDistBS + threadIdx.x) * kDistInitPer;
  DistESlot v;
  v.key = kDistEmptyKey;
  v.stamp = kDistNoEdgeStamp;
#pragma unroll
  for (uint32_t k = 0; k < kDistInitPer; ++k)
    if (s0 + k < slots) tab[s0 + k] = v;
}

// All keys of the old table are distinct: a slot of the new one is claimed by CAS and its
// payload stored by the winner; no other thread reads it in this launch.
__global__ __launch_bounds__(kDistBS) void k_dist_vrebuild(DistVTable from, DistVTable to, unsigned long long* ctl) {
  const uint64_t s = (uint64_t)blockIdx.x * kDistBS + threadIdx.x;
  if (s > from.cap) return;
  int64_t id;
  uint32_t rank, stamp;
  load_vslot(from.tab + s, id, rank, stamp);
  if (s == from.cap) {  // the reserved slot
    to.tab[to.cap].rank = rank;
    to.tab[to.cap].stamp = stamp;
    return;
  }
  if (id == kDistEmptyId) return;
  uint32_t h = dist_vertex_home(id, to.shift) & to.mask;
  for (uint32_t p = 0; p <= to.mask; ++p) {
    const unsigned long long old = atomicCAS((unsigned long long*)&to.tab[h].id, (unsigned long long)kDistEmptyId,
                                             (unsigned long long)id);
    if (old == (unsigned long long)kDistEmptyId) {
      to.tab[h].rank = rank;
      to.tab[h].stamp = stamp;
      return;
    }
    h = (h + 1) & to.mask;
  }
  raise_overflow(ctl);
}

__global__ __launch_bounds__(kDistBS) void k_dist_erebuild(DistETable from, DistETable to, unsigned long long* ctl) {
  const uint64_t s = (uint64_t)blockIdx.x * kDistBS + threadIdx.x;
  if (s >= from.cap) return;
  unsigned long long key, stamp;
  load_eslot(from.tab + s, key, stamp);
  if (key == kDistEmptyKey) return;
  uint32_t h = dist_edge_home(key, to.shift) & to.mask;
  for (uint32_t p = 0; p <= to.mask; ++p) {
    const unsigned long long old = atomicCAS(&to.tab[h].key, (unsigned long long)kDistEmptyKey, key);
    if (old == kDistEmptyKey) {
      to.tab[h].stamp = stamp;
      return;
    }
    h = (h + 1) & to.mask;
  }
  raise_overflow(ctl);
}

// ---- phase 1
__global__ __launch_bounds__(kDistBS) void k_dist_vertices(const int64_t* __restrict__ src,
                                                           const int64_t* __restrict__ dst, uint64_t entries,
                                                           uint64_t stride, DistVTable t, uint32_t* __restrict__ vslot,
                                                           unsigned long long* __restrict__ ctl, int profile) {
  const uint64_t e = (uint64_t)blockIdx.x * kDistBS + threadIdx.x;
  uint32_t probes = 0;
  bool issued = false;
  if (e < entries) {
    const uint64_t i = dist_entry_edge(e);
    const int64_t id = dist_entry_is_dst(e) ? dst[i * stride] : src[i * stride];
    uint32_t rank, stamp;
    const uint32_t s = vertex_insert(t, id, rank, stamp, probes);
    if (s == kDistNoSlot) {
      raise_overflow(ctl);
    } else {
      const uint32_t mine = dist_vertex_stamp(e);
      if (!dist_vertex_skip(rank, stamp, mine)) {
        atomicMin(&t.tab[s].stamp, mine);
        issued = true;
      }
    }
    vslot[e] = s;
  }
  note_probe(ctl, probes);
  if (profile) note_atomics(ctl, issued);
}

// ---- phases 2 and 4: flags and tile counts
// VERT: position = entry, its slot in the vertex table; else position = edge, slot in the edge table
template <bool VERT>
__global__ __launch_bounds__(kDistBS) void k_dist_flag(const uint32_t* __restrict__ slot, uint64_t count,
                                                       uint64_t folded, const DistVSlot* __restrict__ vtab,
                                                       const DistESlot* __restrict__ etab, uint64_t slots,
                                                       uint8_t* __restrict__ flags, uint64_t flag_cap,
                                                       uint32_t* __restrict__ tcount) {
  __shared__ uint32_t total;
  uint32_t cnt = 0;
#pragma unroll
  for (uint32_t k = 0; k < kDistPer; ++k) {
    const uint64_t i = dist_flag_pos(blockIdx.x, DISTINCT_TILE, kDistBS, k, threadIdx.x);
    bool keep = false;
    if (i < count) {
      const uint32_t s = slot[i];
      if (s < slots) {
        if (VERT) {
          int64_t id;
          uint32_t rank, stamp;
          load_vslot(vtab + s, id, rank, stamp);
          keep = dist_vertex_keep(rank, stamp, i);
        } else {
          unsigned long long key, stamp;
          load_eslot(etab + s, key, stamp);
          keep = dist_edge_keep(stamp, folded + i);
        }
      }
    }
    if (i < flag_cap) flags[i] = keep ? 1 : 0;
    cnt += keep ? 1u : 0u;
  }
  block_count_to<kDistBS>(cnt, &total, tcount + blockIdx.x);
}

__global__ __launch_bounds__(kDistBS) void k_dist_vwrite(const uint8_t* __restrict__ flags,
                                                         const uint32_t* __restrict__ tbase,
                                                         const int64_t* __restrict__ src,
                                                         const int64_t* __restrict__ dst, uint64_t entries,
                                                         uint64_t stride, const uint32_t* __restrict__ vslot,
                                                         DistVTable t, uint64_t v0, int64_t* __restrict__ vid,
                                                         uint64_t vid_cap, uint32_t* __restrict__ entry) {
  __shared__ uint32_t wsum[kDistBS / 64];
  const uint64_t i0 = dist_write_first(blockIdx.x, DISTINCT_TILE, kDistPer, threadIdx.x);
  const uint64_t fw = *reinterpret_cast<const uint64_t*>(flags + i0);  // inside the whole tiles
  uint64_t row = dist_out_row(tbase[blockIdx.x], block_excl_scan<kDistBS>((uint32_t)__popcll(fw), wsum));
#pragma unroll
  for (uint32_t k = 0; k < kDistPer; ++k) {
    if ((fw >> (8 * k)) & 1ull) {
      const uint64_t e = i0 + k;
      if (e < entries && row < entries && v0 + row < vid_cap) {
        const uint32_t s = vslot[e];
        if (s <= t.cap) {
          const uint64_t i = dist_entry_edge(e);
          vid[v0 + row] = dist_entry_is_dst(e) ? dst[i * stride] : src[i * stride];
          entry[row] = (uint32_t)e;
          t.tab[s].rank = (uint32_t)(v0 + row);
        }
      }
      ++row;
    }
  }
}

__global__ __launch_bounds__(kDistBS) void k_dist_ewrite(const uint8_t* __restrict__ flags,
                                                         const uint32_t* __restrict__ tbase, uint64_t n,
                                                         uint32_t* __restrict__ index) {
  __shared__ uint32_t wsum[kDistBS / 64];
  const uint64_t i0 = dist_write_first(blockIdx.x, DISTINCT_TILE, kDistPer, threadIdx.x);
  const uint64_t fw = *reinterpret_cast<const uint64_t*>(flags + i0);
  uint64_t row = dist_out_row(tbase[blockIdx.x], block_excl_scan<kDistBS>((uint32_t)__popcll(fw), wsum));
#pragma unroll
  for (uint32_t k = 0; k < kDistPer; ++k) {
    if ((fw >> (8 * k)) & 1ull) {
      if (i0 + k < n && row < n) index[row] = (uint32_t)(i0 + k);
      ++row;
    }
  }
}

// ---- phase 3
__global__ __launch_bounds__(kDistBS) void k_dist_edges(uint64_t n, uint64_t folded, int mode, DistVTable vt,
                                                        const uint32_t* __restrict__ vslot, DistETable et,
                                                        uint32_t* __restrict__ eslot,
                                                        unsigned long long* __restrict__ ctl, int profile) {
  const uint64_t i = (uint64_t)blockIdx.x * kDistBS + threadIdx.x;
  uint32_t probes = 0;
  bool issued = false;
  if (i < n) {
    uint32_t out = kDistNoSlot;
    const uint32_t su = vslot[2 * i], sv = vslot[2 * i + 1];
    uint32_t ru = kDistNoRank, rv = kDistNoRank;
    if (su <= vt.cap && sv <= vt.cap) {  // both ranks are settled: phase 2 wrote them in an earlier launch
      ru = vt.tab[su].rank;
      rv = vt.tab[sv].rank;
    }
    if (ru != kDistNoRank && rv != kDistNoRank) {
      bool swapped;
      const unsigned long long key = dist_edge_key(ru, rv, mode, &swapped);
      const unsigned long long mine = dist_edge_stamp(folded + i, swapped);
      uint32_t h = dist_edge_home(key, et.shift) & et.mask;
      for (uint32_t p = 0; p <= et.mask; ++p) {
        unsigned long long k, stamp;
        load_eslot(et.tab + h, k, stamp);
        if (k == key) {
          if (dist_edge_old(stamp, folded)) {
            out = kDistOldEdge;  // no atomic
          } else {
            if (!dist_edge_skip(stamp, mine)) {
              atomicMin(&et.tab[h].stamp, mine);
              issued = true;
            }
            out = h;
          }
          probes = p;
          break;
        }
        if (k == kDistEmptyKey) {
          const unsigned long long old = atomicCAS(&et.tab[h].key, (unsigned long long)kDistEmptyKey, key);
          if (old == kDistEmptyKey || old == key) {  // claimed, or met a claim of this launch
            atomicMin(&et.tab[h].stamp, mine);
            issued = true;
            out = h;
            probes = p;
            break;
          }
        }
        h = (h + 1) & et.mask;
      }
    }
    if (out == kDistNoSlot) raise_overflow(ctl);
    eslot[i] = out;
  }
  note_probe(ctl, probes);
  if (profile) note_atomics(ctl, issued);
}

// ---- emissions, export, probes
__device__ __forceinline__ void decode_edge(unsigned long long key, unsigned long long stamp, const int64_t* vid,
                                            uint64_t nv, int64_t* src, int64_t* dst, uint64_t row) {
  uint32_t rs, rd;
  dist_key_ranks(key, dist_stamp_swapped(stamp), &rs, &rd);
  if (rs >= nv || rd >= nv) return;
  if (src) src[row] = vid[rs];
  if (dst) dst[row] = vid[rd];
}

__global__ __launch_bounds__(kDistBS) void k_dist_new_edges(const uint32_t* __restrict__ index, uint64_t ne,
                                                            const uint32_t* __restrict__ eslot, uint64_t n,
                                                            DistETable et, const int64_t* __restrict__ vid,
                                                            uint64_t nv, int64_t* __restrict__ src,
                                                            int64_t* __restrict__ dst) {
  const uint64_t k = (uint64_t)blockIdx.x * kDistBS + threadIdx.x;
  if (k >= ne) return;
  const uint32_t i = index[k];
  if (i >= n) return;
  const uint32_t s = eslot[i];
  if (s >= et.cap) return;
  unsigned long long key, stamp;
  load_eslot(et.tab + s, key, stamp);
  decode_edge(key, stamp, vid, nv, src, dst, k);
}

// wave-aggregated append: one atomic per wave for its occupied slots
__global__ __launch_bounds__(kDistBS) void k_dist_export(DistETable et, int64_t* __restrict__ stamp_out,
                                                         unsigned long long* __restrict__ key_out, uint64_t cap,
                                                         unsigned long long* __restrict__ ctl) {
  const uint64_t s = (uint64_t)blockIdx.x * kDistBS + threadIdx.x;
  unsigned long long key = kDistEmptyKey, stamp = kDistNoEdgeStamp;
  if (s < et.cap) load_eslot(et.tab + s, key, stamp);
  const bool has = key != kDistEmptyKey;
  const unsigned long long m = __ballot(has);
  if (!m) return;  // wave-uniform
  const int lane = (int)(threadIdx.x & 63u);
  const int leader = __ffsll((long long)m) - 1;
  unsigned long long base = 0;
  if (lane == leader) base = atomicAdd(ctl + DIST_EXPORT, (unsigned long long)__popcll(m));
  base = __shfl(base, leader, 64);
  if (!has) return;
  const uint64_t row = base + (uint64_t)__popcll(m & ((1ull << lane) - 1ull));
  if (row < cap) {
    stamp_out[row] = (int64_t)stamp;
    key_out[row] = key;
  }
}

__global__ __launch_bounds__(kDistBS) void k_dist_decode(const unsigned long long* __restrict__ skey,
                                                         const uint32_t* __restrict__ pay,
                                                         const unsigned long long* __restrict__ key, uint64_t ne,
                                                         const int64_t* __restrict__ vid, uint64_t nv,
                                                         int64_t* __restrict__ src, int64_t* __restrict__ dst,
                                                         unsigned long long* __restrict__ first) {
  const uint64_t i = (uint64_t)blockIdx.x * kDistBS + threadIdx.x;
  if (i >= ne) return;
  const uint32_t p = pay[i];
  if (p >= ne) return;
  const unsigned long long stamp = skey[i] ^ kSortSignBit;
  decode_edge(key[p], stamp, vid, nv, src, dst, i);
  if (first) first[i] = dist_stamp_arrival(stamp);
}

__global__ __launch_bounds__(kDistBS) void k_dist_rank(DistVTable vt, const int64_t* __restrict__ v, uint64_t n,
                                                       int64_t* __restrict__ rank, uint8_t* __restrict__ found) {
  const uint64_t i = (uint64_t)blockIdx.x * kDistBS + threadIdx.x;
  if (i >= n) return;
  uint32_t r;
  const bool hit = vertex_find(vt, v[i], r) != kDistNoSlot;
  rank[i] = hit ? (int64_t)r : -1;
  if (found) found[i] = hit ? 1 : 0;
}

__global__ __launch_bounds__(kDistBS) void k_dist_contains(DistVTable vt, DistETable et, int mode,
                                                           const int64_t* __restrict__ src,
                                                           const int64_t* __restrict__ dst, uint64_t n,
                                                           uint8_t* __restrict__ found) {
  const uint64_t i = (uint64_t)blockIdx.x * kDistBS + threadIdx.x;
  if (i >= n) return;
  uint32_t ru, rv;
  bool hit = false;
  if (vertex_find(vt, src[i], ru) != kDistNoSlot && vertex_find(vt, dst[i], rv) != kDistNoSlot) {
    bool swapped;
    const unsigned long long key = dist_edge_key(ru, rv, mode, &swapped);
    uint32_t h = dist_edge_home(key, et.shift) & et.mask;
    for (uint32_t p = 0; p <= et.mask; ++p) {
      unsigned long long k, stamp;
      load_eslot(et.tab + h, k, stamp);
      if (k == key) {
        hit = true;
        break;
      }
      if (k == kDistEmptyKey) break;
      h = (h + 1) & et.mask;
    }
  }
  found[i] = hit ? 1 : 0;
}

uint32_t blocks_of(uint64_t n) { return (uint32_t)((n + kDistBS - 1) / kDistBS); }

}  // namespace

void launch_dist_init(const DistVTable& vt, hipStream_t st) {
  const uint64_t slots = (uint64_t)vt.cap + 1;
  hipLaunchKernelGGL(k_dist_vinit, dim3(blocks_of((slots + kDistInitPer - 1) / kDistInitPer)), dim3(kDistBS), 0, st,
                     vt.tab, slots);
}

void launch_dist_init(const DistETable& et, hipStream_t st) {
  const uint64_t slots = et.cap;
  hipLaunchKernelGGL(k_dist_einit, dim3(blocks_of((slots + kDistInitPer - 1) / kDistInitPer)), dim3(kDistBS), 0, st,
                     et.tab, slots);
}

void launch_dist_rebuild(const DistVTable& from, const DistVTable& to, unsigned long long* ctl, hipStream_t st) {
  hipLaunchKernelGGL(k_dist_vrebuild, dim3(blocks_of((uint64_t)from.cap + 1)), dim3(kDistBS), 0, st, from, to, ctl);
}

void launch_dist_rebuild(const DistETable& from, const DistETable& to, unsigned long long* ctl, hipStream_t st) {
  hipLaunchKernelGGL(k_dist_erebuild, dim3(blocks_of(from.cap)), dim3(kDistBS), 0, st, from, to, ctl);
}

void launch_dist_vertices(const int64_t* src, const int64_t* dst, uint64_t n, uint64_t stride, const DistVTable& vt,
                          uint32_t* vslot, uint8_t* flags, uint32_t* tbase, uint64_t v0, int64_t* vid,
                          uint64_t vid_cap, uint32_t* entry, unsigned long long* ctl, hipStream_t st,
                          hipEvent_t mid) {
  const uint64_t entries = 2 * n;
  const uint64_t nt = dist_tiles(entries, DISTINCT_TILE);
  hipLaunchKernelGGL(k_dist_vertices, dim3(blocks_of(entries)), dim3(kDistBS), 0, st, src, dst, entries, stride, vt,
                     vslot, ctl, mid ? 1 : 0);
  if (mid) (void)hipEventRecord(mid, st);
  hipLaunchKernelGGL(k_dist_flag<true>, dim3((uint32_t)nt), dim3(kDistBS), 0, st, (const uint32_t*)vslot, entries,
                     (uint64_t)0, (const DistVSlot*)vt.tab, (const DistESlot*)nullptr, (uint64_t)vt.cap + 1, flags,
                     nt * DISTINCT_TILE, tbase);
  launch_tile_scan(tbase, nt, ctl + DIST_NEW_V, st);
  hipLaunchKernelGGL(k_dist_vwrite, dim3((uint32_t)nt), dim3(kDistBS), 0, st, (const uint8_t*)flags,
                     (const uint32_t*)tbase, src, dst, entries, stride, (const uint32_t*)vslot, vt, v0, vid, vid_cap,
                     entry);
}

void launch_dist_edges(uint64_t n, uint64_t folded, int mode, const DistVTable& vt, const uint32_t* vslot,
                       const DistETable& et, uint32_t* eslot, uint8_t* flags, uint32_t* tbase, uint32_t* index,
                       unsigned long long* ctl, hipStream_t st, hipEvent_t mid) {
  const uint64_t nt = dist_tiles(n, DISTINCT_TILE);
  hipLaunchKernelGGL(k_dist_edges, dim3(blocks_of(n)), dim3(kDistBS), 0, st, n, folded, mode, vt, vslot, et, eslot,
                     ctl, mid ? 1 : 0);
  if (mid) (void)hipEventRecord(mid, st);
  hipLaunchKernelGGL(k_dist_flag<false>, dim3((uint32_t)nt), dim3(kDistBS), 0, st, (const uint32_t*)eslot, n, folded,
                     (const DistVSlot*)nullptr, (const DistESlot*)et.tab, (uint64_t)et.cap, flags, nt * DISTINCT_TILE,
                     tbase);
  launch_tile_scan(tbase, nt, ctl + DIST_NEW_E, st);
  hipLaunchKernelGGL(k_dist_ewrite, dim3((uint32_t)nt), dim3(kDistBS), 0, st, (const uint8_t*)flags,
                     (const uint32_t*)tbase, n, index);
}

void launch_dist_new_edges(const uint32_t* index, uint64_t ne, const uint32_t* eslot, uint64_t n, const DistETable& et,
                           const int64_t* vid, uint64_t nv, int64_t* src, int64_t* dst, hipStream_t st) {
  hipLaunchKernelGGL(k_dist_new_edges, dim3(blocks_of(ne)), dim3(kDistBS), 0, st, index, ne, eslot, n, et, vid, nv, src,
                     dst);
}

void launch_dist_export(const DistETable& et, int64_t* stamp, unsigned long long* key, uint64_t cap,
                        unsigned long long* ctl, hipStream_t st) {
  hipLaunchKernelGGL(k_dist_export, dim3(blocks_of(et.cap)), dim3(kDistBS), 0, st, et, stamp, key, cap, ctl);
}

void launch_dist_decode(const unsigned long long* skey, const uint32_t* pay, const unsigned long long* key, uint64_t ne,
                        const int64_t* vid, uint64_t nv, int64_t* src, int64_t* dst, unsigned long long* first,
                        hipStream_t st) {
  hipLaunchKernelGGL(k_dist_decode, dim3(blocks_of(ne)), dim3(kDistBS), 0, st, skey, pay, key, ne, vid, nv, src, dst,
                     first);
}

void launch_dist_rank(const DistVTable& vt, const int64_t* v, uint64_t n, int64_t* rank, uint8_t* found,
                      hipStream_t st) {
  hipLaunchKernelGGL(k_dist_rank, dim3(blocks_of(n)), dim3(kDistBS), 0, st, vt, v, n, rank, found);
}

void launch_dist_contains(const DistVTable& vt, const DistETable& et, int mode, const int64_t* src, const int64_t* dst,
                          uint64_t n, uint8_t* found, hipStream_t st) {
  hipLaunchKernelGGL(k_dist_contains, dim3(blocks_of(n)), dim3(kDistBS), 0, st, vt, et, mode, src, dst, n, found);
}

}  // namespace gs
