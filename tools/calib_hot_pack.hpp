// calib_hot_pack.hpp -- the 32-B bucket of five quotiented ids that tools/calib_hot.hip prices as
// variant K5 against the library's 16-B bucket of two keys (profiles/hot_ways_calib.txt: not
// faster at the same 1 MiB, so the library keeps two keys per bucket). Sizes, packing, matching.
//
// A bucket is 32 B, 32-B aligned: four 64-bit words, read with two 16-B loads. The bucket of a
// key is the top q bits of m = key * kHotMul (an odd multiplier: a bijection on 64 bits).
//   index of 2^L ids, L >= 16 (q = L - 3 >= 13), "packed": five places of 51 bits. A place holds
//     the low 51 bits of m; the bucket number gives the top q >= 13 bits, so position plus stored
//     bits cover all 64 and a match is exact. Places 0-3 are the low 51 bits of the four words,
//     place 4 is spread over their top 13 bits (13 + 13 + 13 + 12; the last bit stays 0). Stored
//     bits 0 mean an empty place: a key whose low 51 product bits are 0 is never held and never
//     hits (INT64_MIN among them: its product is 2^63).
//   L <= 15 (q = max(0, L - 3) <= 12), "wide": four places of 64 bits that hold the key itself,
//     kHotEmptyKey (INT64_MIN, never a key of the table proper) for an empty place. Only
//     min(4, 2^L) of them are used.
// At every L the index holds at most 2^L ids.
#ifndef CALIB_HOT_PACK_HPP_
#define CALIB_HOT_PACK_HPP_
#include <stdint.h>

#if defined(__HIPCC__)
#define GS_HOT_HD __host__ __device__ inline
#else
#define GS_HOT_HD inline
#endif

namespace gs {

constexpr uint64_t kHotMul = 0xD6E8FEB86659FD93ull;
constexpr uint64_t hot_mul_inverse() {
  uint64_t x = kHotMul;  // correct to 3 bits; every Newton step doubles them
  for (int i = 0; i < 6; ++i) x *= 2 - kHotMul * x;
  return x;
}
constexpr uint64_t kHotMulInv = hot_mul_inverse();
static_assert(kHotMul * kHotMulInv == 1, "kHotMulInv");
constexpr int kHotPackedLog2 = 16;  // the smallest packed index
constexpr int kHotStoredBits = 51;
constexpr uint64_t kHotStoredMask = (1ull << kHotStoredBits) - 1;
constexpr int kHotPieceBits = 64 - kHotStoredBits;  // 13: a word's share of place 4
constexpr uint64_t kHotPieceMask = (1ull << kHotPieceBits) - 1;
constexpr int kHotMaxPlaces = 5;
constexpr int64_t kHotEmptyKey = INT64_MIN;

struct alignas(32) HotBucket {
  uint64_t w[4];
};

GS_HOT_HD bool hot_packed(int log2_ids) { return log2_ids >= kHotPackedLog2; }
GS_HOT_HD int hot_bucket_log2(int log2_ids) { return log2_ids > 3 ? log2_ids - 3 : 0; }
GS_HOT_HD uint64_t hot_buckets(int log2_ids) { return 1ull << hot_bucket_log2(log2_ids); }
// places of a bucket that are used
GS_HOT_HD int hot_places(int log2_ids) {
  return hot_packed(log2_ids) ? kHotMaxPlaces : (log2_ids >= 2 ? 4 : 2);
}
GS_HOT_HD uint64_t hot_capacity(int log2_ids) { return hot_buckets(log2_ids) * (uint64_t)hot_places(log2_ids); }

GS_HOT_HD uint64_t hot_product(int64_t key) { return (uint64_t)key * kHotMul; }
// the bucket of a product among 2^q (q <= 32; q == 0: the one bucket)
GS_HOT_HD uint32_t hot_bucket_of(uint64_t m, int q) { return (uint32_t)((m >> 32) >> (32 - q)); }
GS_HOT_HD uint64_t hot_stored(uint64_t m) { return m & kHotStoredMask; }
// what a place holds for a key: its stored bits (packed) or the key (wide)
GS_HOT_HD uint64_t hot_value(int64_t key, bool packed) { return packed ? hot_stored(hot_product(key)) : (uint64_t)key; }
GS_HOT_HD uint64_t hot_empty_value(bool packed) { return packed ? 0ull : (uint64_t)kHotEmptyKey; }

GS_HOT_HD void hot_clear(HotBucket& b, bool packed) {
  for (int i = 0; i < 4; ++i) b.w[i] = hot_empty_value(packed);
}
GS_HOT_HD uint64_t hot_get(const HotBucket& b, int place, bool packed) {
  if (!packed) return b.w[place];
  if (place < 4) return b.w[place] & kHotStoredMask;
  return ((b.w[0] >> kHotStoredBits) | ((b.w[1] >> kHotStoredBits) << kHotPieceBits) |
          ((b.w[2] >> kHotStoredBits) << (2 * kHotPieceBits)) | ((b.w[3] >> kHotStoredBits) << (3 * kHotPieceBits))) &
         kHotStoredMask;
}
// v: hot_value of the key (packed: at most 51 bits)
GS_HOT_HD void hot_set(HotBucket& b, int place, bool packed, uint64_t v) {
  if (!packed) {
    b.w[place] = v;
  } else if (place < 4) {
    b.w[place] = (b.w[place] & ~kHotStoredMask) | (v & kHotStoredMask);
  } else {
    for (int i = 0; i < 4; ++i)
      b.w[i] = (b.w[i] & kHotStoredMask) | (((v >> (i * kHotPieceBits)) & kHotPieceMask) << kHotStoredBits);
    b.w[3] &= ~(1ull << 63);  // bit 51 of place 4 does not exist
  }
}
GS_HOT_HD bool hot_held(const HotBucket& b, int place, bool packed) {
  return hot_get(b, place, packed) != hot_empty_value(packed);
}
// the key a held place of bucket p (of 2^q) stands for
GS_HOT_HD int64_t hot_key_at(const HotBucket& b, int place, bool packed, uint32_t p, int q) {
  if (!packed) return (int64_t)b.w[place];
  const uint64_t top = (uint64_t)(p >> (q - kHotPieceBits)) << kHotStoredBits;  // the product's top 13 bits
  return (int64_t)((top | hot_get(b, place, true)) * kHotMulInv);
}

// true when bucket b, the bucket of key (m = hot_product(key)), holds it
GS_HOT_HD bool hot_match(const HotBucket& b, bool packed, int64_t key, uint64_t m) {
  if (packed) {
    const uint64_t s = m & kHotStoredMask;
    // place 4 piecewise: each word's top 13 bits against the matching piece of s (the piece of
    // w[3] has 12 bits and a 0 above them, as has s)
    const bool p4 = ((b.w[0] >> kHotStoredBits) == (s & kHotPieceMask)) &
                    ((b.w[1] >> kHotStoredBits) == ((s >> kHotPieceBits) & kHotPieceMask)) &
                    ((b.w[2] >> kHotStoredBits) == ((s >> (2 * kHotPieceBits)) & kHotPieceMask)) &
                    ((b.w[3] >> kHotStoredBits) == (s >> (3 * kHotPieceBits)));
    const bool p03 = (((b.w[0] ^ s) & kHotStoredMask) == 0) | (((b.w[1] ^ s) & kHotStoredMask) == 0) |
                     (((b.w[2] ^ s) & kHotStoredMask) == 0) | (((b.w[3] ^ s) & kHotStoredMask) == 0);
    return (p03 | p4) & (s != 0);  // (no short circuit: the loads stay together)
  }
  const uint64_t k = (uint64_t)key;
  return ((b.w[0] == k) | (b.w[1] == k) | (b.w[2] == k) | (b.w[3] == k)) & (key != kHotEmptyKey);
}

}  // namespace gs

#endif  // CALIB_HOT_PACK_HPP_
