// -m address / -m rmd160 / -m xpoint: what the walk does with each point (hash160, with -c eth the ETH address, or
// for -m xpoint the first 20 bytes of x, + the target bloom; or the x||y dump).
#pragma once
#include "scan_args.hpp"
#include "hash160.hpp"
#include "keccak.hpp"
#include "xpoint.hpp"
#include "vanity.hpp"

namespace khbk {

// The vanity kernels' copy of the bucket bitmap in LDS (8 KiB per block; only kernels that reach it allocate it).
__device__ __forceinline__ uint32_t* vanity_lds() {
  __shared__ uint32_t s_bitmap[kVanityBitmapWords];
  return s_bitmap;
}

// Kernel entry of a vanity instance: every block copies the bitmap in once (the grid is persistent), one barrier.
__device__ __forceinline__ void vanity_load_bitmap(const uint32_t* __restrict__ bitmap) {
  uint32_t* s = vanity_lds();
  for (uint32_t i = threadIdx.x; i < kVanityBitmapWords; i += blockDim.x) s[i] = bitmap[i];
  __syncthreads();
}

// The last step of a BTC address mode: is the hash160 h a candidate?  The -m address modes probe the target bloom;
// the -m vanity modes test the interval table (device/vanity.hpp), its bitmap in LDS.
template <int MODE>
__device__ __forceinline__ bool addr_match(const ScanArgs& A, const uint32_t h[5]) {
  if constexpr (is_vanity(MODE))
    return vanity_match(vanity_lds(), A.van_lo, A.van_hi, A.van_n, h);
  else
    return bloom_check20(A.bloom, A.geom, h);
}

// beta (keyhunt.cpp:584): lambda*P = (beta*x, y).  beta^2*x is computed as beta*(beta*x), the same canonical value as
// the reference's ModMulK1(x, beta2) (beta2 = beta^2 mod p, keyhunt.cpp:585), with one constant and no indexed table.
__device__ __forceinline__ Fe fe_beta() {
  return Fe{{0x719501eeu, 0xc1396c28u, 0x12f58995u, 0x9cf04975u, 0xac3434e9u, 0x6e64479eu, 0x657c0710u, 0x7ae96a2bu}};
}

// x, beta*x and beta^2*x of one point (-m xpoint -e).
__device__ __forceinline__ void xpoint_endo(const ScanArgs& A, const Fe& x, uint32_t t, uint32_t job, uint32_t j) {
  const Fe kBeta = fe_beta();
  Fe xe = x;
#pragma unroll 1
  for (uint32_t e = 0; e < 3; ++e) {
    if (e) {
      fm_mul(xe, xe, kBeta);
      fm_canon(xe, xe);
    }
    uint32_t h[5];
    x_be20(h, xe);
    if (bloom_check20(A.bloom, A.geom, h)) emit_ahit(A, job, j, t, KHB_ADDR_KIND_X | (e << 2));
  }
}

// -m xpoint handling of a walk step's two points (keyhunt.cpp:3005-3062): the first 20 bytes of each canonical x
// probed in the target bloom (kind KHB_ADDR_KIND_X), with -e also those of beta*x and beta^2*x, each canonical before
// it is serialised (kind KHB_ADDR_KIND_X | e << 2; keyhunt.cpp:3013-3043).  Without -e both serialisations stand
// before either bloom load is issued.  TWO = false: x1 alone.
template <int MODE, bool TWO>
__device__ __forceinline__ void xpoint_probe(const ScanArgs& A, const Fe& x1, uint32_t t1, const Fe& x2, uint32_t t2,
                                             uint32_t job, uint32_t j) {
  static_assert(is_xpoint(MODE), "xpoint_probe: kAddrX or kAddrXE");
  uint32_t h1[5], h2[5];
  if constexpr (MODE == kAddrX) {
    x_be20(h1, x1);
    if constexpr (TWO) x_be20(h2, x2);
    const bool b1 = bloom_check20(A.bloom, A.geom, h1);
    const bool b2 = TWO && bloom_check20(A.bloom, A.geom, h2);
    if (b1) emit_ahit(A, job, j, t1, KHB_ADDR_KIND_X);
    if (b2) emit_ahit(A, job, j, t2, KHB_ADDR_KIND_X);
  } else {
    // one point after the other
    xpoint_endo(A, x1, t1, job, j);
    if constexpr (TWO) xpoint_endo(A, x2, t2, job, j);
  }
}

// -m address handling of one point (keyhunt.cpp:2716-2937, BTC, no endomorphism): hash160 of
// the compressed key for both prefixes from x alone (covers +k and -k, keyhunt.cpp:2719-2733) and/or
// of the uncompressed key, each probed in the single target bloom (-m vanity: tested against the interval table,
// addr_match); hits go to the host, which runs searchbinary and the key recovery.  x and y are canonical.
template <int MODE>
__device__ __forceinline__ void addr_point(const ScanArgs& A, const Fe& x, const Fe& y, uint32_t job, uint32_t j,
                                           uint32_t t) {
  static_assert(is_addr(MODE), "addr_point: an -m address mode");
  if constexpr (MODE == kAddrDump) {
    uint8_t* o = A.xdump + ((uint64_t)(j - A.group_begin) * KHB_GROUP + t) * 64;
    fe_to_be(o, x);
    fe_to_be(o + 32, y);
  } else if constexpr (is_xpoint(MODE)) {
    xpoint_probe<MODE, false>(A, x, t, x, t, job, j);   // y is not read
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
      const Fe kBeta = fe_beta();
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
            if (addr_match<MODE>(A, h)) emit_ahit(A, job, j, t, (pre - 2) | (e << 2));
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
            if (addr_match<MODE>(A, h)) emit_ahit(A, job, j, t, (2u + neg) | (e << 2));
          }
        }
      }
    } else {
      if constexpr (addr_compressed(MODE)) {
#pragma unroll 1
        for (uint32_t pre = 2; pre <= 3; ++pre) {
          hash160_compressed(h, pre, x);
          if (addr_match<MODE>(A, h)) emit_ahit(A, job, j, t, pre - 2);
        }
      }
      if constexpr (addr_uncompressed(MODE)) {
        hash160_uncompressed(h, x, y);
        if (addr_match<MODE>(A, h)) emit_ahit(A, job, j, t, 2);
      }
    }
  }
}

}  // namespace khbk
