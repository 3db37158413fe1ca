// -m vanity: does a hash160 lie in one of a few ranges of 160-bit numbers?  The reference answers with a bloom over
// the leading bytes all its ranges share and a linear memcmp scan behind it (keyhunt.cpp:5775-5801); here the question
// is answered exactly, by a bucket bitmap and a binary search.  Host and device share this code (KHB_HD) so
// tests/native checks it on the CPU.
//
// Table (khb_load_vanity): R sorted, disjoint, closed intervals [lo_i, hi_i] of 160-bit big-endian numbers, each bound
// as five 32-bit words, word 0 the most significant (lo[5i .. 5i+4], hi[5i .. 5i+4]), and a bucket bitmap of 2^16
// bits (kVanityBitmapWords words, 8 KiB): bit b is set iff some interval holds a value whose first two bytes are b.
// A hash tests its bucket's bit first; only on a set bit it searches lo[] for the last lo_i <= h and tests h <= hi_i.
//
// Deliberate deviation from the reference: its addvanity (keyhunt.cpp:5837-5958) pairs the j-th '1'-padded lower bound
// with the j-th 'z'-padded upper bound, which loses or empties ranges when the two lists differ in length (for "1Q"
// the 34-character addresses are never matched).  The intervals loaded here are exact per address length
// (host/vanity_host.hpp builds them), and a hit is confirmed on the host by the printed address itself.
//
// Byte conventions: hash160_* leaves five words whose little-endian bytes are the hash bytes (bloom_check20's order),
// so the number's k-th word is bswap32(h[k]) and its first two bytes are the low half of h[0].
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "fe.hpp"
#include "bloom_probe.hpp"

namespace khb {

constexpr uint32_t kVanityBitmapWords = (1u << 16) / 32;   // 2,048 words = 8 KiB

// a <= b for 160-bit numbers of five words, word 0 the most significant
KHB_HD bool vanity_le(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b) {
#pragma unroll
  for (int k = 0; k < 5; ++k)
    if (a[k] != b[k]) return a[k] < b[k];
  return true;
}

// The bucket (first two bytes as a number) of a hash in hash160_*'s word order.
KHB_HD uint32_t vanity_bucket(const uint32_t h[5]) { return ((h[0] & 0xFFu) << 8) | ((h[0] >> 8) & 0xFFu); }

// w (five words, word 0 the most significant) lies in one of the n intervals.
KHB_HD bool vanity_search(const uint32_t* __restrict__ lo, const uint32_t* __restrict__ hi, uint32_t n,
                          const uint32_t w[5]) {
  uint32_t a = 0, b = n;                 // a = the number of intervals with lo_i <= w once a == b
  while (a < b) {
    const uint32_t m = a + (b - a) / 2;  // m < n
    if (vanity_le(lo + 5 * (size_t)m, w)) a = m + 1;
    else b = m;
  }
  return a != 0 && vanity_le(w, hi + 5 * (size_t)(a - 1));
}

// The match stage of the vanity kernels: h in hash160_*'s word order.  bitmap may be LDS or global memory.
KHB_HD bool vanity_match(const uint32_t* __restrict__ bitmap, const uint32_t* __restrict__ lo,
                         const uint32_t* __restrict__ hi, uint32_t n, const uint32_t h[5]) {
  const uint32_t b = vanity_bucket(h);
  if (!((bitmap[b >> 5] >> (b & 31u)) & 1u)) return false;
  uint32_t w[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) w[k] = bswap32(h[k]);
  return vanity_search(lo, hi, n, w);
}

// The bucket bitmap of n intervals (lo_i <= hi_i): every bucket from lo_i's to hi_i's.
static inline void vanity_build_bitmap(uint32_t bitmap[kVanityBitmapWords], const uint32_t* lo, const uint32_t* hi,
                                       uint32_t n) {
  for (uint32_t i = 0; i < kVanityBitmapWords; ++i) bitmap[i] = 0;
  for (uint32_t i = 0; i < n; ++i)
    for (uint32_t b = lo[5 * (size_t)i] >> 16; b <= hi[5 * (size_t)i] >> 16; ++b) bitmap[b >> 5] |= 1u << (b & 31u);
}

}  // namespace khb
