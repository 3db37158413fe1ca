// Host-side run of device/vanity.hpp (compiled for the CPU, with the address and undefined-behaviour sanitizers by
// tests/test_native_vanity.py): reads a table and probe values from the file named on the command line,
//   u32 n, n x lo (20 bytes big-endian), n x hi, u32 m, m x value (20 bytes),
// builds the bucket bitmap with vanity_build_bitmap and checks it and vanity_match against a linear scan of its own
// (memcmp on the bytes, every bucket tested against every interval).  Prints one line of m characters, '1' for a value
// inside an interval by vanity_match; exits 1 on any disagreement with the linear scan.  Test infrastructure.
#include "../../keyhuntm1cpu_amd/csrc/device/vanity.hpp"
#include <cstdio>
#include <cstring>
#include <vector>
using namespace khb;

static uint32_t be32(const uint8_t* p) {
  return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t n = 0, m = 0;
  if (fread(&n, 4, 1, f) != 1 || n == 0) return 2;
  std::vector<uint8_t> lo(20 * (size_t)n), hi(20 * (size_t)n);
  if (fread(lo.data(), 20, n, f) != n || fread(hi.data(), 20, n, f) != n || fread(&m, 4, 1, f) != 1) return 2;
  std::vector<uint8_t> v(20 * (size_t)m);
  if (m && fread(v.data(), 20, m, f) != m) return 2;
  fclose(f);
  // exactly-sized heap arrays: a read past either end is the sanitizer's to report
  std::vector<uint32_t> wlo(5 * (size_t)n), whi(5 * (size_t)n), bitmap(kVanityBitmapWords);
  for (size_t k = 0; k < 5 * (size_t)n; ++k) {
    wlo[k] = be32(lo.data() + 4 * k);
    whi[k] = be32(hi.data() + 4 * k);
  }
  vanity_build_bitmap(bitmap.data(), wlo.data(), whi.data(), n);
  int bad = 0;
  for (uint32_t b = 0; b < 65536; ++b) {
    bool any = false;             // some interval holds a value whose first two bytes are b
    for (uint32_t i = 0; i < n && !any; ++i) {
      const uint32_t b0 = ((uint32_t)lo[20 * (size_t)i] << 8) | lo[20 * (size_t)i + 1];
      const uint32_t b1 = ((uint32_t)hi[20 * (size_t)i] << 8) | hi[20 * (size_t)i + 1];
      any = b0 <= b && b <= b1;
    }
    if ((((bitmap[b >> 5] >> (b & 31)) & 1u) != 0) != any) {
      if (!bad++) fprintf(stderr, "bitmap bit %04x: %d, linear scan %d\n", b, !any, any);
    }
  }
  std::vector<char> line(m + 1, 0);
  for (uint32_t j = 0; j < m; ++j) {
    const uint8_t* p = v.data() + 20 * (size_t)j;
    uint32_t h[5];                // hash160_*'s word order: the little-endian bytes of the words are the value's bytes
    memcpy(h, p, 20);
    const bool got = vanity_match(bitmap.data(), wlo.data(), whi.data(), n, h);
    bool want = false;
    for (uint32_t i = 0; i < n && !want; ++i)
      want = memcmp(lo.data() + 20 * (size_t)i, p, 20) <= 0 && memcmp(p, hi.data() + 20 * (size_t)i, 20) <= 0;
    if (got != want && !bad++) fprintf(stderr, "value %u: vanity_match %d, linear scan %d\n", j, got, want);
    line[j] = got ? '1' : '0';
  }
  printf("%s\n", line.data());
  return bad ? 1 : 0;
}
