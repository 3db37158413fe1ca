// k_giant_scan instances for -m bsgs: the scan (ungated, gated, gated with the stage-1 fold, and with the stage-0 filter in front of it) and the
// x dump (kDump) of the same walk for parity tests.
#include "scan_kernels.hpp"

namespace khbk { static const ScanInstances<kDump, kScanG2, kScanG1, kScanG, kScan> instances; }
