// -m address / -m rmd160: what the x,y walk does with each point (hash160 or, with -c eth, the ETH address + the
// target bloom, or the x||y dump).
#pragma once
#include "scan_args.hpp"
#include "hash160.hpp"
#include "keccak.hpp"

namespace khbk {

// -m address handling of one point (keyhunt.cpp:2716-2937, BTC, no endomorphism): hash160 of
// the compressed key for both prefixes from x alone (covers +k and -k, keyhunt.cpp:2719-2733) and/or
// of the uncompressed key, each probed in the single target bloom; hits go to the host, which runs
// searchbinary and the key recovery.  x and y are canonical.
template <int MODE>
__device__ __forceinline__ void addr_point(const ScanArgs& A, const Fe& x, const Fe& y, uint32_t job, uint32_t j,
                                           uint32_t t) {
  static_assert(is_addr(MODE), "addr_point: an -m address mode");
  if constexpr (MODE == kAddrDump) {
    uint8_t* o = A.xdump + ((uint64_t)(j - A.group_begin) * KHB_GROUP + t) * 64;
    fe_to_be(o, x);
    fe_to_be(o + 32, y);
  } else if constexpr (MODE == kAddrEth) {
    // -c eth (keyhunt.cpp:2776-2780, 2989-3002): one Keccak-f[1600] per point; the address words are already in
    // bloom_check20's byte order
    uint32_t h[5];
    eth_address(h, x, y);
    if (bloom_check20(A.bloom, A.geom, h)) emit_ahit(A, job, j, t, KHB_ADDR_KIND_ETH);
  } else {
    uint32_t h[5];
    if constexpr (is_endo(MODE)) {
      // -e (keyhunt.cpp:2646-2763): lambda*P = (beta*x, y) and lambda^2*P = (beta^2*x, y) (keyhunt.cpp:582-585).
      // Compressed: the 02 and 03 hashes of x, beta*x, beta^2*x (kinds 0|e<<2, 1|e<<2); uncompressed: (x_e, y) and
      // (x_e, p - y), the negated point (kinds 2|e<<2, 3|e<<2).  Every x_e is canonical before it is hashed.
      // beta (keyhunt.cpp:584); beta^2*x is computed as beta*(beta*x), the same canonical value as the reference's
      // ModMulK1(x, beta2) (beta2 = beta^2 mod p, keyhunt.cpp:585), with one constant and no indexed table
      const Fe kBeta = {{0x719501eeu, 0xc1396c28u, 0x12f58995u, 0x9cf04975u, 0xac3434e9u, 0x6e64479eu, 0x657c0710u,
                         0x7ae96a2bu}};
      Fe ny;
      if constexpr (addr_uncompressed(MODE)) {
        fm_sub(ny, fe_p(), y);                     // y != 0 on the curve: p - y is canonical
        fm_canon(ny, ny);
      }
      Fe xe = x;
#pragma unroll 1
      for (uint32_t e = 0; e < 3; ++e) {
        if (e) {
          fm_mul(xe, xe, kBeta);
          fm_canon(xe, xe);
        }
        if constexpr (addr_compressed(MODE)) {
#pragma unroll 1
          for (uint32_t pre = 2; pre <= 3; ++pre) {
            hash160_compressed(h, pre, xe);
            if (bloom_check20(A.bloom, A.geom, h)) emit_ahit(A, job, j, t, (pre - 2) | (e << 2));
          }
        }
        if constexpr (addr_uncompressed(MODE)) {
          // one copy of the two-block hash in the loop body (unrolled twice it spilled ~700 VGPRs)
#pragma unroll 1
          for (uint32_t neg = 0; neg < 2; ++neg) {
            Fe yy;
#pragma unroll
            for (int k = 0; k < 8; ++k) yy.v[k] = neg ? ny.v[k] : y.v[k];
            hash160_uncompressed(h, xe, yy);
            if (bloom_check20(A.bloom, A.geom, h)) emit_ahit(A, job, j, t, (2u + neg) | (e << 2));
          }
        }
      }
    } else {
      if constexpr (MODE == kAddrC || MODE == kAddrB) {
#pragma unroll 1
        for (uint32_t pre = 2; pre <= 3; ++pre) {
          hash160_compressed(h, pre, x);
          if (bloom_check20(A.bloom, A.geom, h)) emit_ahit(A, job, j, t, pre - 2);
        }
      }
      if constexpr (MODE == kAddrU || MODE == kAddrB) {
        hash160_uncompressed(h, x, y);
        if (bloom_check20(A.bloom, A.geom, h)) emit_ahit(A, job, j, t, 2);
      }
    }
  }
}

}  // namespace khbk
