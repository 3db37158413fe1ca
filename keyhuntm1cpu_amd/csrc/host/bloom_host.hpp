// Host bloom filter: libbloom v2 semantics used by keyhunt (bloom/bloom.h:26-45,
// bloom/bloom.cpp:93-162) for the two key shapes keyhunt hashes: 32-byte x-coordinates (-m bsgs)
// and 20-byte hash160 values (-m address / -m rmd160).
#pragma once
#include <math.h>
#include <stdint.h>
#include <vector>

#include "../device/bloom_probe.hpp"

namespace khb {

struct BloomFilter {
  uint64_t entries = 0, bits = 0, bytes = 0;
  uint8_t hashes = 0;
  long double error = 0;
  double bpe = 0;
  bool ready = false;
  std::vector<uint8_t> bf;

  // bloom_init2: bits = entries * (-ln(err) / ln(2)^2) in long double, hashes = ceil(ln2 * bpe).
  // alloc = false keeps the geometry only (bf stays empty: the bits live on a device, Tables::resident).
  // Inline: the front end prints a filter's size (cli.cpp) without linking the library.
  int init2(uint64_t n_entries, long double err, bool alloc = true);
  // bloom_check / bloom_add on Get32Bytes(x) (keyhunt.cpp:3945-3946, 4515-4560).
  bool check32(const uint8_t x[32]) const;
  void add32_atomic(const uint8_t x[32]);     // thread-safe byte OR: same bits as mutex + bloom_add
  // bloom_check / bloom_add on a 20-byte hash160 (keyhunt.cpp:6341-6350, 2793-2800)
  bool check20(const uint8_t h[20]) const;
  void add20(const uint8_t h[20]);
  BloomGeom geom() const;
};

inline int BloomFilter::init2(uint64_t n_entries, long double err, bool alloc) {
  *this = BloomFilter();
  if (n_entries < 1000 || err <= 0 || err >= 1) return 1;
  entries = n_entries;
  error = err;
  const long double num = -logl(error);
  const long double denom = 0.480453013918201;   // ln(2)^2 as the reference spells it
  bpe = (double)(num / denom);
  const long double allbits = (long double)entries * bpe;
  bits = (uint64_t)allbits;
  bytes = bits / 8 + ((bits % 8) ? 1 : 0);
  hashes = (uint8_t)ceil(0.693147180559945 * bpe);
  if (alloc) bf.assign(bytes, 0);
  ready = true;
  return 0;
}

void words_of_bytes32(uint64_t w[4], const uint8_t x[32]);

}  // namespace khb
