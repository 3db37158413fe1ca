// k_giant_scan instances for -m address / -m rmd160 (uncompress, compress, both) and the x||y dump (scan_kernels.hpp).
#include "scan_kernels.hpp"

namespace khbk { static const ScanInstances<kAddrDump, kAddrB, kAddrC, kAddrU> instances; }
