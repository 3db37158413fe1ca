// k_giant_scan instances for -m address / -m rmd160 with -e (endomorphism: the hashes of beta*x and beta^2*x and,
// for uncompressed keys, of the negated points; keyhunt.cpp:2646-2763), in a translation unit of their own so that
// `make -j` compiles them beside the plain address kernels (k_addr.hip).
#include "scan_kernels.hpp"

namespace khbk { static const ScanInstances<kAddrBE, kAddrCE, kAddrUE> instances; }
