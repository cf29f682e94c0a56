// The distinct streams' arithmetic (csrc/gs_distinct_seq.hpp) on the host, against brute force,
// built with -fsanitize=address,undefined (tests/test_distinct_seq.py). The program walks a fold
// the way gs_distinct_k.hip does -- tables as arrays; phase 1: insert-or-find and a minimum of the
// stamp for every entry, in every order of a small permutation set (the result must not depend
// on the schedule), with the loaded payload fresh or stale; phase 2: flags over whole tiles, tile
// counts, their exclusive scan, the write by threads of P consecutive positions; phases 3 and 4:
// the same over rank pairs -- with every decision (stamp, skip, keep, key, home slot, growth,
// tile and row) taken by the header's functions, and checks that every output row is written
// exactly once, inside its array, with the right value.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <set>
#include <utility>
#include <vector>

#include "gs_distinct_seq.hpp"

using namespace gs;

static long checks = 0;

#define REQUIRE(cond)                                                       \
  do {                                                                      \
    ++checks;                                                               \
    if (!(cond)) {                                                          \
      std::printf("FAILED %s (line %d)\n", #cond, __LINE__);                \
      std::exit(1);                                                         \
    }                                                                       \
  } while (0)

template <typename V>
static auto& at(V& v, uint64_t i) {
  REQUIRE(i < v.size());
  return v[i];
}

struct VSlot {
  int64_t id;
  uint32_t rank, stamp;
};
struct ESlot {
  uint64_t key, stamp;
};

constexpr uint64_t kWalkMinSlots = 16;

// ---- the device state, as arrays
struct Walk {
  int mode;
  uint64_t min_slots;
  std::vector<VSlot> vtab;  // [vcap + 1]
  std::vector<ESlot> etab;  // [ecap]
  std::vector<int64_t> vid;
  uint64_t vcap = 0, ecap = 0, nv = 0, ne = 0, folded = 0;
  int v_rebuilds = 0, e_rebuilds = 0;
  uint64_t atomics = 0;
  // the last fold's scratch, kept like the handle's (and spared the allocator)
  std::vector<uint32_t> vslot, eslot, tbase, writes, row_writes;
  std::vector<uint8_t> keep, flags;

  explicit Walk(int m, uint64_t min_s = kWalkMinSlots) : mode(m), min_slots(min_s) {
    set_vertices(dist_slots_for(0, min_slots));
    set_edges(dist_slots_for(0, min_slots));
  }
  int vshift() const { return 64 - dist_log2(vcap); }
  int eshift() const { return 64 - dist_log2(ecap); }

  static std::vector<VSlot> vinit(uint64_t cap) { return std::vector<VSlot>(cap + 1, VSlot{kDistEmptyId, kDistNoRank, kDistNoStamp}); }
  static std::vector<ESlot> einit(uint64_t cap) { return std::vector<ESlot>(cap, ESlot{kDistEmptyKey, kDistNoEdgeStamp}); }

  // k_dist_vrebuild: every occupied slot into the new table, payload included
  void set_vertices(uint64_t cap) {
    REQUIRE(cap >= 16 && (cap & (cap - 1)) == 0 && cap <= kDistMaxSlots);
    std::vector<VSlot> to = vinit(cap);
    const int shift = 64 - dist_log2(cap);
    if (vcap) {
      for (uint64_t s = 0; s <= vcap; ++s) {
        const VSlot o = at(vtab, s);
        if (s == vcap) {
          at(to, cap).rank = o.rank;
          at(to, cap).stamp = o.stamp;
          continue;
        }
        if (o.id == kDistEmptyId) continue;
        uint64_t h = dist_vertex_home(o.id, shift) & (cap - 1);
        bool placed = false;
        for (uint64_t p = 0; p < cap && !placed; ++p) {
          if (at(to, h).id == kDistEmptyId) {
            at(to, h) = o;
            placed = true;
          }
          h = (h + 1) & (cap - 1);
        }
        REQUIRE(placed);
      }
      ++v_rebuilds;
    }
    vtab.swap(to);
    vcap = cap;
    vid.resize(dist_vid_cap(cap), 0);
  }
  void set_edges(uint64_t cap) {
    REQUIRE(cap >= 16 && (cap & (cap - 1)) == 0 && cap <= kDistMaxSlots);
    std::vector<ESlot> to = einit(cap);
    const int shift = 64 - dist_log2(cap);
    if (ecap) {
      for (uint64_t s = 0; s < ecap; ++s) {
        const ESlot o = at(etab, s);
        if (o.key == kDistEmptyKey) continue;
        uint64_t h = dist_edge_home(o.key, shift) & (cap - 1);
        bool placed = false;
        for (uint64_t p = 0; p < cap && !placed; ++p) {
          if (at(to, h).key == kDistEmptyKey) {
            at(to, h) = o;
            placed = true;
          }
          h = (h + 1) & (cap - 1);
        }
        REQUIRE(placed);
      }
      ++e_rebuilds;
    }
    etab.swap(to);
    ecap = cap;
  }

  // vertex_insert of the kernels: the slot, or kDistNoSlot
  uint32_t vertex_insert(int64_t id) {
    if (id == kDistEmptyId) return (uint32_t)vcap;
    uint64_t h = dist_vertex_home(id, vshift()) & (vcap - 1);
    for (uint64_t p = 0; p < vcap; ++p) {
      VSlot& s = at(vtab, h);
      if (s.id == id) return (uint32_t)h;
      if (s.id == kDistEmptyId) {
        s.id = id;  // (the CAS)
        return (uint32_t)h;
      }
      h = (h + 1) & (vcap - 1);
    }
    return kDistNoSlot;
  }
};

struct FoldOut {
  std::vector<int64_t> new_v;
  std::vector<uint32_t> new_v_entry, new_e_index;
};

// flags over whole tiles, tile counts, exclusive scan: the positions a flag kernel of tile T,
// BS threads and P positions per thread visits; every position of the whole tiles exactly once
static void flag_and_scan(uint64_t count, uint32_t T, uint32_t P, const std::vector<uint8_t>& keep,
                          std::vector<uint8_t>* flags, std::vector<uint32_t>* tb, std::vector<uint32_t>* wr) {
  std::vector<uint32_t>&tbase = *tb, &writes = *wr;
  const uint32_t BS = T / P;
  REQUIRE(BS * P == T);
  const uint64_t nt = dist_tiles(count, T);
  REQUIRE(nt * T >= count && (nt == 0 || (nt - 1) * T < count));
  flags->assign(nt * T, 0xCC);
  writes.assign(nt * T, 0);
  tbase.assign(nt + 1, 0);
  for (uint64_t t = 0; t < nt; ++t) {
    uint32_t total = 0;
    for (uint32_t thread = 0; thread < BS; ++thread)
      for (uint32_t k = 0; k < P; ++k) {
        const uint64_t i = dist_flag_pos(t, T, BS, k, thread);
        const bool kp = i < count && keep[i];
        at(*flags, i) = kp ? 1 : 0;
        ++at(writes, i);
        total += kp ? 1u : 0u;
      }
    tbase[t] = total;
  }
  for (uint32_t w : writes) REQUIRE(w == 1);
  uint32_t carry = 0;
  for (uint64_t t = 0; t < nt; ++t) {
    const uint32_t x = tbase[t];
    tbase[t] = carry;
    carry += x;
  }
  tbase[nt] = carry;
}

// the write kernels' walk: calls emit(position, row) for every kept position, rows ascending
template <typename F>
static void write_walk(uint64_t count, uint32_t T, uint32_t P, const std::vector<uint8_t>& flags,
                       const std::vector<uint32_t>& tbase, F emit) {
  const uint32_t BS = T / P;
  const uint64_t nt = dist_tiles(count, T);
  for (uint64_t t = 0; t < nt; ++t) {
    uint32_t before = 0;  // kept before the thread inside the tile (the wave scan + the waves before)
    for (uint32_t thread = 0; thread < BS; ++thread) {
      const uint64_t i0 = dist_write_first(t, T, P, thread);
      uint64_t row = dist_out_row(at(tbase, t), before);
      for (uint32_t k = 0; k < P; ++k) {
        REQUIRE(i0 + k < flags.size());  // a flag is read inside the whole tiles
        const uint8_t f = flags[i0 + k];
        REQUIRE(f == 0 || f == 1);
        if (f) {
          if (i0 + k < count) emit(i0 + k, row);
          ++row;
          ++before;
        }
      }
    }
  }
}

// One fold, walked as the kernels walk it. order_v / order_e: the order in which entries / edges
// take their turn in phases 1 and 3; stale: the loaded payload of a slot is what it was when the
// launch began (a plain load need not be fresh)
static FoldOut walk_fold(Walk& w, const std::vector<int64_t>& src, const std::vector<int64_t>& dst, uint32_t T,
                         uint32_t P, const std::vector<uint32_t>& order_v, const std::vector<uint32_t>& order_e,
                         bool stale) {
  FoldOut out;
  const uint64_t n = src.size(), entries = 2 * n;
  REQUIRE(n <= kDistMaxFold);
  if (n == 0) return out;
  // growth, decided before the fold from the totals
  if (dist_must_grow(w.nv, dist_worst_vertices(n), w.vcap))
    w.set_vertices(dist_slots_for(w.nv + dist_worst_vertices(n), w.min_slots));
  if (dist_must_grow(w.ne, dist_worst_edges(n), w.ecap)) w.set_edges(dist_slots_for(w.ne + dist_worst_edges(n), w.min_slots));
  REQUIRE(w.nv + dist_worst_vertices(n) <= w.vcap / 2 && w.ne + dist_worst_edges(n) <= w.ecap / 2);
  REQUIRE(w.nv + dist_worst_vertices(n) <= dist_vid_cap(w.vcap));

  // phase 1
  std::vector<uint32_t>&vslot = w.vslot, &eslot = w.eslot, &tbase = w.tbase, &row_writes = w.row_writes;
  std::vector<uint8_t>&keep = w.keep, &flags = w.flags;
  vslot.assign(entries, kDistNoSlot);
  REQUIRE(order_v.size() == entries);
  for (uint32_t e : order_v) {
    const int64_t id = dist_entry_is_dst(e) ? at(dst, dist_entry_edge(e)) : at(src, dist_entry_edge(e));
    const uint32_t s = w.vertex_insert(id);
    REQUIRE(s != kDistNoSlot);
    // What a stale load shows is the slot as the launch found it: a rank (ranks are written by
    // phase 2, never during this launch), or neither rank nor stamp.
    VSlot seen = at(w.vtab, s);
    if (stale && seen.rank == kDistNoRank) seen.stamp = kDistNoStamp;
    const uint32_t mine = dist_vertex_stamp(e);
    REQUIRE(mine != kDistNoStamp);
    if (!dist_vertex_skip(seen.rank, seen.stamp, mine)) {
      VSlot& slot = at(w.vtab, s);
      slot.stamp = std::min(slot.stamp, mine);  // (the atomic minimum)
      ++w.atomics;
    }
    at(vslot, e) = s;
  }
  // phase 2
  keep.assign(entries, 0);
  for (uint64_t e = 0; e < entries; ++e) {
    const VSlot& s = at(w.vtab, at(vslot, e));
    keep[e] = dist_vertex_keep(s.rank, s.stamp, e) ? 1 : 0;
  }
  flag_and_scan(entries, T, P, keep, &flags, &tbase, &w.writes);
  const uint64_t new_v = tbase.back();
  REQUIRE(new_v <= entries);
  out.new_v.assign(new_v, 0);
  out.new_v_entry.assign(new_v, 0);
  row_writes.assign(new_v, 0);
  const uint64_t v0 = w.nv;
  write_walk(entries, T, P, flags, tbase, [&](uint64_t e, uint64_t row) {
    REQUIRE(v0 + row < dist_vid_cap(w.vcap) && v0 + row <= kDistMaxVertices - 1);
    const int64_t id = dist_entry_is_dst(e) ? at(dst, dist_entry_edge(e)) : at(src, dist_entry_edge(e));
    at(w.vid, v0 + row) = id;
    at(out.new_v, row) = id;
    at(out.new_v_entry, row) = (uint32_t)e;
    ++at(row_writes, row);
    VSlot& slot = at(w.vtab, at(vslot, e));
    REQUIRE(slot.rank == kDistNoRank);  // a rank is written once
    slot.rank = (uint32_t)(v0 + row);
  });
  for (uint32_t c : row_writes) REQUIRE(c == 1);
  w.nv += new_v;

  // phase 3
  eslot.assign(n, kDistNoSlot);
  REQUIRE(order_e.size() == n);
  for (uint32_t i : order_e) {
    const uint32_t ru = at(w.vtab, at(vslot, 2 * (uint64_t)i)).rank, rv = at(w.vtab, at(vslot, 2 * (uint64_t)i + 1)).rank;
    REQUIRE(ru != kDistNoRank && rv != kDistNoRank && ru < w.nv && rv < w.nv);  // settled by phase 2
    bool swapped = false;
    const uint64_t key = dist_edge_key(ru, rv, w.mode, &swapped);
    REQUIRE(key != kDistEmptyKey);
    uint32_t rs = 0, rd = 0;
    dist_key_ranks(key, swapped, &rs, &rd);
    REQUIRE(rs == ru && rd == rv);
    const uint64_t mine = dist_edge_stamp(w.folded + i, swapped);
    REQUIRE(dist_stamp_arrival(mine) == w.folded + i && dist_stamp_swapped(mine) == swapped);
    uint64_t h = dist_edge_home(key, w.eshift()) & (w.ecap - 1);
    uint32_t got = kDistNoSlot;
    for (uint64_t p = 0; p < w.ecap; ++p) {
      ESlot& s = at(w.etab, h);
      if (s.key == kDistEmptyKey) s.key = key;  // (the CAS)
      if (s.key == key) {
        // a stale load shows the slot as the launch found it: an edge of an earlier fold (its
        // stamp is below every stamp of this fold, so it never changes), or an empty slot
        ESlot seen = s;
        if (stale && !dist_edge_old(s.stamp, w.folded)) seen = ESlot{kDistEmptyKey, kDistNoEdgeStamp};
        if (seen.key == key && dist_edge_old(seen.stamp, w.folded)) {
          got = kDistOldEdge;
        } else {
          if (seen.key != key || !dist_edge_skip(seen.stamp, mine)) {
            s.stamp = std::min(s.stamp, mine);
            ++w.atomics;
          }
          got = (uint32_t)h;
        }
        break;
      }
      h = (h + 1) & (w.ecap - 1);
    }
    REQUIRE(got != kDistNoSlot);
    at(eslot, i) = got;
  }
  // phase 4
  keep.assign(n, 0);  // (the flag bytes and tile counts are shared by both compactions)
  for (uint64_t i = 0; i < n; ++i) {
    const uint32_t s = at(eslot, i);
    if (s == kDistOldEdge) continue;
    keep[i] = dist_edge_keep(at(w.etab, s).stamp, w.folded + i) ? 1 : 0;
  }
  flag_and_scan(n, T, P, keep, &flags, &tbase, &w.writes);
  const uint64_t new_e = tbase.back();
  REQUIRE(new_e <= n);
  out.new_e_index.assign(new_e, 0);
  row_writes.assign(new_e, 0);
  write_walk(n, T, P, flags, tbase, [&](uint64_t i, uint64_t row) {
    at(out.new_e_index, row) = (uint32_t)i;
    ++at(row_writes, row);
  });
  for (uint32_t c : row_writes) REQUIRE(c == 1);
  w.ne += new_e;
  w.folded += n;
  return out;
}

// the edge export: the occupied slots sorted by stamp, decoded through the vertex list
static void walk_edges(Walk& w, std::vector<int64_t>* src, std::vector<int64_t>* dst, std::vector<uint64_t>* first) {
  std::vector<std::pair<uint64_t, uint64_t>> rows;  // (stamp, key)
  for (const ESlot& s : w.etab)
    if (s.key != kDistEmptyKey) rows.emplace_back(s.stamp, s.key);
  REQUIRE(rows.size() == w.ne);
  std::sort(rows.begin(), rows.end());
  for (const auto& r : rows) {
    uint32_t rs = 0, rd = 0;
    dist_key_ranks(r.second, dist_stamp_swapped(r.first), &rs, &rd);
    REQUIRE(rs < w.nv && rd < w.nv);
    src->push_back(at(w.vid, rs));
    dst->push_back(at(w.vid, rd));
    first->push_back(dist_stamp_arrival(r.first));
  }
}

// ---- the truth: sets
struct Brute {
  int mode;
  std::set<int64_t> vs;
  std::set<std::pair<int64_t, int64_t>> es;
  std::vector<int64_t> vlist, esrc, edst;
  std::vector<uint64_t> efirst;
  uint64_t folded = 0;
  explicit Brute(int m) : mode(m) {}
  FoldOut fold(const std::vector<int64_t>& src, const std::vector<int64_t>& dst) {
    FoldOut o;
    for (size_t i = 0; i < src.size(); ++i) {
      const int64_t ends[2] = {src[i], dst[i]};
      for (int k = 0; k < 2; ++k)
        if (vs.insert(ends[k]).second) {
          o.new_v.push_back(ends[k]);
          o.new_v_entry.push_back((uint32_t)(2 * i + k));
          vlist.push_back(ends[k]);
        }
      std::pair<int64_t, int64_t> key(src[i], dst[i]);
      if (mode == kDistUndirected && key.first > key.second) std::swap(key.first, key.second);
      if (es.insert(key).second) {
        o.new_e_index.push_back((uint32_t)i);
        esrc.push_back(src[i]);
        edst.push_back(dst[i]);
        efirst.push_back(folded + i);
      }
    }
    folded += src.size();
    return o;
  }
};

// the permutation set of the atomic steps: arrival order, its reverse, odd positions before even
// ones, a random shuffle
static std::vector<uint32_t> order_of(uint32_t n, int which, std::mt19937_64& rng) {
  std::vector<uint32_t> r;
  r.reserve(n);
  switch (which & 3) {
    case 0:
      for (uint32_t i = 0; i < n; ++i) r.push_back(i);
      break;
    case 1:
      for (uint32_t i = n; i > 0; --i) r.push_back(i - 1);
      break;
    case 2:
      for (uint32_t i = 1; i < n; i += 2) r.push_back(i);
      for (uint32_t i = 0; i < n; i += 2) r.push_back(i);
      break;
    default:
      for (uint32_t i = 0; i < n; ++i) r.push_back(i);
      std::shuffle(r.begin(), r.end(), rng);
  }
  return r;
}

static void compare(const FoldOut& got, const FoldOut& want) {
  REQUIRE(got.new_v == want.new_v);
  REQUIRE(got.new_v_entry == want.new_v_entry);
  REQUIRE(got.new_e_index == want.new_e_index);
}

static void compare_state(Walk& w, const Brute& b) {
  REQUIRE(w.nv == b.vlist.size() && w.ne == b.esrc.size() && w.folded == b.folded);
  for (uint64_t k = 0; k < w.nv; ++k) REQUIRE(at(w.vid, k) == b.vlist[k]);
  std::vector<int64_t> s, d;
  std::vector<uint64_t> f;
  walk_edges(w, &s, &d, &f);
  REQUIRE(s == b.esrc && d == b.edst && f == b.efirst);
}

// A stream cut into folds at `cuts`, every fold in order `which` of the permutation set,
// continuing the state of w and b
static void run_folds(Walk& w, Brute& b, const std::vector<int64_t>& src, const std::vector<int64_t>& dst,
                      const std::vector<size_t>& cuts, uint32_t T, uint32_t P, int which, bool stale,
                      std::mt19937_64& rng) {
  size_t at0 = 0;
  std::vector<size_t> ends = cuts;
  ends.push_back(src.size());
  for (size_t end : ends) {
    REQUIRE(end >= at0 && end <= src.size());
    const std::vector<int64_t> s(src.begin() + at0, src.begin() + end), d(dst.begin() + at0, dst.begin() + end);
    const uint32_t n = (uint32_t)s.size();
    const FoldOut got = walk_fold(w, s, d, T, P, order_of(2 * n, which, rng), order_of(n, which, rng), stale);
    compare(got, b.fold(s, d));
    at0 = end;
  }
}

// the same from an empty state, which is compared as a whole at the end
static void run_stream(int mode, const std::vector<int64_t>& src, const std::vector<int64_t>& dst,
                       const std::vector<size_t>& cuts, uint32_t T, uint32_t P, int which, bool stale,
                       std::mt19937_64& rng, int* v_rebuilds = nullptr) {
  Walk w(mode);
  Brute b(mode);
  run_folds(w, b, src, dst, cuts, T, P, which, stale, rng);
  compare_state(w, b);
  if (v_rebuilds) *v_rebuilds = w.v_rebuilds;
}

int main() {
  std::mt19937_64 rng(0xD157C7ull);
  const int64_t I64MIN = kDistEmptyId, I64MAX = 0x7FFFFFFFFFFFFFFFll;

  // encodings
  REQUIRE(dist_vertex_stamp(0) == 1 && dist_vertex_stamp(2 * kDistMaxFold - 1) == 0xFFFFFFFCu);
  REQUIRE(!dist_edge_old(kDistNoEdgeStamp, ~0ull >> 2));
  REQUIRE(dist_edge_old(dist_edge_stamp(4, true), 5) && !dist_edge_old(dist_edge_stamp(5, false), 5));
  REQUIRE(dist_slots_for(0) == kDistMinSlots && dist_slots_for(513) == 2048 && dist_slots_for(512) == 1024);
  REQUIRE(dist_must_grow(0, 513, 1024) && !dist_must_grow(0, 512, 1024));
  {
    bool sw = false;
    REQUIRE(dist_edge_key(5, 3, kDistDirected, &sw) == ((5ull << 32) | 3) && !sw);
    REQUIRE(dist_edge_key(5, 3, kDistUndirected, &sw) == ((3ull << 32) | 5) && sw);
    REQUIRE(dist_edge_key(0xFFFFFFFDu, 0xFFFFFFFDu, kDistUndirected, &sw) != kDistEmptyKey && !sw);
  }
  for (int logcap = 4; logcap <= 31; ++logcap)
    for (int64_t id : {int64_t(0), int64_t(1), int64_t(-1), I64MAX, I64MIN + 1, int64_t(123456789)}) {
      REQUIRE(dist_vertex_home(id, 64 - logcap) < (1ull << logcap));
      REQUIRE(dist_edge_home((uint64_t)id, 64 - logcap) < (1ull << logcap));
    }

  for (int mode = 0; mode < kDistModes; ++mode)
    for (int stale = 0; stale < 2; ++stale)
      for (int which = 0; which < 4; ++which) {
        // the empty fold, one edge, a loop
        run_stream(mode, {}, {}, {}, 8, 2, which, stale, rng);
        run_stream(mode, {}, {}, {0, 0}, 8, 2, which, stale, rng);
        run_stream(mode, {7}, {9}, {}, 8, 2, which, stale, rng);
        run_stream(mode, {7}, {7}, {}, 8, 2, which, stale, rng);
        run_stream(mode, {7, 7}, {7, 7}, {1}, 8, 2, which, stale, rng);
        // (u, v) then (v, u); ids INT64_MIN / INT64_MAX
        run_stream(mode, {1, 2, 1}, {2, 1, 2}, {}, 8, 2, which, stale, rng);
        run_stream(mode, {I64MIN, I64MAX, -1, I64MIN, 0}, {I64MAX, I64MIN, 0, I64MIN, -1}, {2}, 8, 2, which, stale, rng);
        // all-equal and all-distinct tiles, around the tile size
        for (uint32_t n : {7u, 8u, 9u, 17u}) {
          std::vector<int64_t> eq_s(n, 3), eq_d(n, 4), ds(n), dd(n);
          for (uint32_t i = 0; i < n; ++i) {
            ds[i] = 100 + 2 * i;
            dd[i] = 101 + 2 * i;
          }
          run_stream(mode, eq_s, eq_d, {}, 8, 2, which, stale, rng);
          run_stream(mode, ds, dd, {}, 8, 2, which, stale, rng);
          run_stream(mode, ds, dd, {n / 2}, 8, 4, which, stale, rng);
        }
        // a first occurrence on a tile's last position (edge 7 of tile 0; entry 7 = dst of edge 3)
        {
          std::vector<int64_t> s(16, 1), d(16, 1);
          s[7] = 1, d[7] = 2;
          run_stream(mode, s, d, {}, 8, 2, which, stale, rng);
          std::vector<int64_t> s2(8, 1), d2(8, 1);
          d2[3] = 5;
          run_stream(mode, s2, d2, {}, 8, 2, which, stale, rng);
        }
        // a rebuild between folds: 40 fresh vertices per fold pass the walk's smallest tables
        {
          std::vector<int64_t> s, d;
          for (int i = 0; i < 60; ++i) {
            s.push_back(1000 + i);
            d.push_back(i % 3 ? 2000 + i : 1000 + i / 2);
          }
          int rebuilds = 0;
          run_stream(mode, s, d, {5, 20, 20, 45}, 8, 2, which, stale, rng, &rebuilds);
          REQUIRE(rebuilds >= 2);
        }
      }

  // every pattern of 6 edges over 3 ids, both modes; cut, order and staleness vary with the
  // pattern. 729 patterns share one state, each over three ids of its own (the tables grow and
  // their clusters differ from pattern to pattern); the state is compared as a whole after each batch.
  for (int mode = 0; mode < kDistModes; ++mode) {
    long patterns = 0;
    Walk w(mode);
    Brute b(mode);
    for (uint32_t code = 0; code < 531441u; ++code) {  // 9^6
      const int64_t base = (int64_t)(code % 729u) * 3;
      std::vector<int64_t> s(6), d(6);
      uint32_t c = code;
      for (int i = 0; i < 6; ++i) {
        s[i] = base + (c % 9) / 3;
        d[i] = base + (c % 9) % 3;
        c /= 9;
      }
      std::vector<size_t> cuts;
      if (code % 7) cuts.push_back(code % 7 - 1);
      run_folds(w, b, s, d, cuts, 4, 2, (int)(code % 4), (code / 4) % 2 != 0, rng);
      ++patterns;
      if (code % 729u == 728u) {
        compare_state(w, b);
        w = Walk(mode);
        b = Brute(mode);
      }
    }
    REQUIRE(patterns == 531441);
  }

  // 10^4 random folds cut at random points over tiles of 8, duplicate-heavy and wide ids
  for (int mode = 0; mode < kDistModes; ++mode) {
    Walk w(mode);
    Brute b(mode);
    for (int f = 0; f < 10000; ++f) {
      if (f % 500 == 0) {  // a fresh handle: the tables grow again from the smallest
        compare_state(w, b);
        w = Walk(mode);
        b = Brute(mode);
      }
      const uint32_t n = (uint32_t)(rng() % 41);
      const int64_t range = f % 3 ? 12 : 400;
      std::vector<int64_t> s(n), d(n);
      for (uint32_t i = 0; i < n; ++i) {
        s[i] = f % 5 == 4 ? (int64_t)rng() : (int64_t)(rng() % range);
        d[i] = f % 5 == 4 ? (int64_t)rng() : (int64_t)(rng() % range);
      }
      const FoldOut got = walk_fold(w, s, d, 8, f % 2 ? 2 : 4, order_of(2 * n, f, rng), order_of(n, f / 4, rng),
                                    (f / 16) % 2 != 0);
      compare(got, b.fold(s, d));
    }
    compare_state(w, b);
    REQUIRE(w.v_rebuilds > 0 && w.e_rebuilds > 0);
  }

  // the steady state issues no atomic: a second pass over the same stream
  {
    Walk w(kDistDirected);
    std::vector<int64_t> s, d;
    for (int i = 0; i < 100; ++i) {
      s.push_back(i % 17);
      d.push_back(i % 13);
    }
    walk_fold(w, s, d, 8, 2, order_of(200, 3, rng), order_of(100, 3, rng), false);
    const uint64_t before = w.atomics;
    REQUIRE(before > 0);
    const FoldOut again = walk_fold(w, s, d, 8, 2, order_of(200, 1, rng), order_of(100, 2, rng), false);
    REQUIRE(w.atomics == before && again.new_v.empty() && again.new_e_index.empty());
  }

  // the kernels' own tile shape: tiles of 2048, 8 positions per thread
  for (int mode = 0; mode < kDistModes; ++mode)
    for (uint32_t n : {2047u, 2048u, 2049u, 4097u}) {
      std::vector<int64_t> s(n), d(n);
      for (uint32_t i = 0; i < n; ++i) {
        s[i] = (int64_t)(rng() % 3000);
        d[i] = (int64_t)(rng() % 3000);
      }
      s[n - 1] = 70000, d[n - 1] = 70001;  // a first occurrence on the last position
      Walk w(mode, kDistMinSlots);
      Brute b(mode);
      compare(walk_fold(w, s, d, 2048, 8, order_of(2 * n, 3, rng), order_of(n, 1, rng), true), b.fold(s, d));
      compare(walk_fold(w, s, d, 2048, 8, order_of(2 * n, 2, rng), order_of(n, 3, rng), false), b.fold(s, d));
      compare_state(w, b);
    }

  std::printf("all checks passed (%ld)\n", checks);
  return 0;
}
