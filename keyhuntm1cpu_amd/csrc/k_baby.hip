// k_giant_scan instance for the baby-step table build (kBaby, khb_build_baby; scan_kernels.hpp).
#include "scan_kernels.hpp"

namespace khbk { static const ScanInstances<kBaby> instances; }
