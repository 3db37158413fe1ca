// k_giant_scan instances for -m vanity (the walk and hash160s of -m address, with or without -e, matched against the
// interval table of device/vanity.hpp instead of the target bloom; keyhunt.cpp:3105-3540), in a translation unit of
// their own beside the address kernels (k_addr.hip, k_addr_e.hip).
#include "scan_kernels.hpp"

namespace khbk {

void launch_vanity(int mode, uint32_t blocks, hipStream_t stream, const ScanArgs& A) {
  switch (mode) {
    case kVanU: hipLaunchKernelGGL(k_giant_scan<kVanU>, dim3(blocks), dim3(kBlock), 0, stream, A); break;
    case kVanC: hipLaunchKernelGGL(k_giant_scan<kVanC>, dim3(blocks), dim3(kBlock), 0, stream, A); break;
    case kVanB: hipLaunchKernelGGL(k_giant_scan<kVanB>, dim3(blocks), dim3(kBlock), 0, stream, A); break;
    case kVanUE: hipLaunchKernelGGL(k_giant_scan<kVanUE>, dim3(blocks), dim3(kBlock), 0, stream, A); break;
    case kVanCE: hipLaunchKernelGGL(k_giant_scan<kVanCE>, dim3(blocks), dim3(kBlock), 0, stream, A); break;
    case kVanBE: hipLaunchKernelGGL(k_giant_scan<kVanBE>, dim3(blocks), dim3(kBlock), 0, stream, A); break;
    default: break;
  }
}

}  // namespace khbk
