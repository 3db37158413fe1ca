// k_giant_scan instances for -m vanity (the walk and hash160s of -m address, with or without -e, matched against the
// interval table of device/vanity.hpp instead of the target bloom; keyhunt.cpp:3105-3540), in a translation unit of
// their own beside the address kernels (k_addr.hip, k_addr_e.hip).
#include "scan_kernels.hpp"

namespace khbk { static const ScanInstances<kVanBE, kVanCE, kVanUE, kVanB, kVanC, kVanU> instances; }
