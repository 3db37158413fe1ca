// k_giant_scan instances for -m xpoint (the first 20 bytes of every walked x probed in the target bloom, with -e also
// those of beta*x and beta^2*x; keyhunt.cpp:3005-3062, device/xpoint.hpp), in a translation unit of their own beside
// the address kernels (k_addr.hip, k_addr_e.hip, k_addr_eth.hip).
#include "scan_kernels.hpp"

namespace khbk { static const ScanInstances<kAddrXE, kAddrX> instances; }
