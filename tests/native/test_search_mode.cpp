// device/scan_modes.hpp on the host: the decoder of khb_addr_submit's `search` and the traits of the kernel modes,
// printed for tests/test_native_search_mode.py to compare with its literal tables.
//   s <search> invalid
//   s <search> <family> <forms> <endo> <vanity> <kernel mode> <encode_search of the fields>
//   m <mode> <the fourteen predicates in the order below, waves_per_simd as its Occupancy>
#include <stdio.h>

#include "../../keyhuntm1cpu_amd/csrc/device/scan_modes.hpp"

using namespace khbk;

int main() {
  for (int search = -2; search < 128; ++search) {
    SearchMode sm;
    if (!decode_search(search, sm)) {
      printf("s %d invalid\n", search);
      continue;
    }
    printf("s %d %d %d %d %d %d %d\n", search, (int)sm.family, sm.forms, (int)sm.endo, (int)sm.vanity, scan_mode_of(sm),
           encode_search(sm));
  }
  for (int m = 0; m < kModeCount; ++m)
    printf("m %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", m, (int)is_gated(m), gate_stages(m), (int)is_scan(m),
           (int)is_vanity(m), (int)is_endo(m), (int)is_xpoint(m), (int)is_addr(m), (int)addr_compressed(m),
           (int)addr_uncompressed(m), (int)needs_y(m), (int)is_dump(m), (int)is_batched(m), (int)is_xy(m),
           (int)traits(m).occ);
  return 0;
}
