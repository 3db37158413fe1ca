// k_giant_scan instance for -m address -c eth (one Keccak-f[1600] per point, device/keccak.hpp; keyhunt.cpp:2776-2780),
// in a translation unit of its own beside the BTC address kernels (k_addr.hip, k_addr_e.hip).
#include "scan_kernels.hpp"

namespace khbk { static const ScanInstances<kAddrEth> instances; }
