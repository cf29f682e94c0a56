// gs_degree.hpp -- host-side launchers of the degree summary's kernels (gs_degree_k.hip):
// the tiled degree fold with on-chip combining, the batched find, the table export and the
// small tails of the sorted export and of the degree distribution. Every launch is queued
// on the given stream; kernel boundaries carry all ordering between workgroups (no
// workgroup waits on another inside a launch).
//
// The counter of a vertex lives in the 32-bit link word of its slot (gs_device.hpp):
//   degree(slot s) = (int32)(link - (s << 1))   mod 2^32
// so the table's initial value (every slot its own root, link = s << 1) reads as zero and
// init, reset-by-list and the vertex list work unchanged. The fold only ever touches link
// with memory-side atomic adds; it never reads a counter.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gs_device.hpp"

namespace gs {

constexpr uint32_t kDegreeBS = 256;    // threads of a k_degree_fold workgroup
constexpr uint32_t kDegreeItems = 8;   // edges per thread
// Edges per workgroup (gsamd.DEGREE_TILE): the tile whose endpoint occurrences are summed
// per id in LDS before any global atomic.
constexpr uint32_t DEGREE_TILE = 2048;
static_assert(DEGREE_TILE == kDegreeBS * kDegreeItems, "tile = threads x edges per thread");
constexpr uint32_t kDegreeLdsLog2 = 10;  // LDS hash slots of the product kernel (1024: 12 KiB)
constexpr uint32_t kDegreeLdsProbes = 4; // bounded linear probe of the LDS hash; then the id goes to global

// Kernel variants (the product is 0; the others are the measured alternatives of
// tools/degree_bench.py, selected through the private test knob GS_TESTING_DEGREE_VARIANT).
enum DegreeVariant : int {
  kDegreeProduct = 0,     // tile 2048, 1024 LDS slots
  kDegreeNoCombine = 1,   // tile 2048, every occurrence is its own global atomic
  kDegreeLds4096 = 2,     // tile 2048, 4096 LDS slots
  kDegreeTile1024 = 3,    // tile 1024, 2048 LDS slots
  kDegreeLds2048 = 4,     // tile 2048, 2048 LDS slots
  kDegreeProbeOnly = 5,   // DIAGNOSTIC: the product kernel without its counter adds (counts stay 0):
                          //   what the probes, inserts and the LDS phase cost without the atomics
  kDegreeVariants = 6
};

enum DegreeDir : int { kDegreeAll = 0, kDegreeIn = 1, kDegreeOut = 2 };

// One k_degree_fold launch. Edge form (wt == nullptr): element i is src[i * stride],
// dst[i * stride]; del (optional) one byte per edge, bit 0 = deletion; dir says which
// endpoints are collected. Row form (wt != nullptr): element i adds wt[i] (may be <= 0) to
// vertex src[i] and inserts it whatever the weight (combine, table rebuild, deserialize).
struct DegreeLaunch {
  const int64_t* src = nullptr;
  const int64_t* dst = nullptr;
  const uint8_t* del = nullptr;
  const int64_t* wt = nullptr;
  uint32_t n = 0;
  uint32_t stride = 1;
  int dir = kDegreeAll;
  uint32_t shard0 = 0;
};

// edges per workgroup of a variant, and workgroups of a launch of n elements
uint32_t degree_tile(int variant);
uint32_t degree_blocks(uint32_t n, int variant);
void launch_degree_fold(const Table& t, const DegreeLaunch& f, int variant, hipStream_t st);

// degree[i] = count of v[i] when it is > 0, else 0; found[i] (optional) = that test
void launch_degree_find(const Table& t, const int64_t* v, uint64_t n, int64_t* degree, uint8_t* found,
                        hipStream_t st);
// Table scan: every entry (all) or every entry with a count > 0 appended to (ov, od),
// unordered; *count (zero before) = rows found, of which the first cap_out are written.
void launch_degree_export(const Table& t, int64_t* ov, int64_t* od, uint64_t cap_out, unsigned long long* count,
                          bool all, hipStream_t st);
// ov[i] = v[pay[i]], od[i] = d[pay[i]] (pay == nullptr: the identity)
void launch_degree_gather(const uint32_t* pay, const int64_t* v, const int64_t* d, uint64_t n, int64_t* ov,
                          int64_t* od, hipStream_t st);
// *out (zero before) += positions i of the sorted keys with i == 0 or key[i] != key[i - 1]
void launch_degree_heads(const unsigned long long* key, uint64_t n, unsigned long long* out, hipStream_t st);
// degree[i] = comp[i], count[i] = off[i + 1] - off[i] for i < nd
void launch_degree_runs(const int64_t* comp, const unsigned long long* off, uint64_t nd, int64_t* degree,
                        int64_t* count, hipStream_t st);

}  // namespace gs
