// Host-side run of device/keccak.hpp (compiled for the CPU): reads points x || y (64 bytes each) from the file named
// on the command line and prints one 40-hex address per point.  tests/test_native_keccak.py compares the lines with
// the tests' own Keccak (tests/eth_ref.py).  Test infrastructure.
#include "../../keyhuntm1cpu_amd/csrc/device/keccak.hpp"
#include <cstdio>
using namespace khb;

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint8_t b[64];
  while (fread(b, 1, 64, f) == 64) {
    Fe x, y;
    fe_from_be(x, b);
    fe_from_be(y, b + 32);
    uint32_t h[5];
    eth_address(h, x, y);
    for (int k = 0; k < 5; ++k)
      for (int s = 0; s < 4; ++s) printf("%02x", (unsigned)((h[k] >> (8 * s)) & 0xffu));
    printf("\n");
  }
  fclose(f);
  return 0;
}
