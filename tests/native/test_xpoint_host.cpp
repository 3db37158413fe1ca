// Host-side run of device/xpoint.hpp (compiled for the CPU): reads x values (32 bytes big-endian each) from the file
// named on the command line and prints the 20 bytes x_be20 gives for each as one 40-hex line.
// tests/test_xpoint_host.py compares the lines with the first 20 bytes of x.  Test infrastructure.
#include "../../keyhuntm1cpu_amd/csrc/device/xpoint.hpp"
#include <cstdio>
using namespace khb;

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint8_t b[32];
  while (fread(b, 1, 32, f) == 32) {
    Fe x;
    fe_from_be(x, b);
    uint32_t h[5];
    x_be20(h, x);
    for (int k = 0; k < 5; ++k)
      for (int s = 0; s < 4; ++s) printf("%02x", (unsigned)((h[k] >> (8 * s)) & 0xffu));
    printf("\n");
  }
  fclose(f);
  return 0;
}
