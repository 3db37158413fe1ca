// Ethereum address of a secp256k1 public key for keyhunt's -m address -c eth (generate_binaddress_eth,
// keyhunt.cpp:4783-4789): Keccak-256 of x || y (64 bytes, each coordinate big-endian), bytes 12..31 of the digest.
// Keccak as submitted to the SHA-3 competition (pad byte 0x01, not FIPS 202's 0x06; sha3/sha3.c:229), rate 136,
// so the 64-byte message is one block and the address one Keccak-f[1600]:
//   lanes 0..7 : the message (lanes are little-endian 64-bit words of the byte stream)
//   lane 8     : 0x01, the first pad byte (byte 64)
//   lane 16    : 0x80 << 56, the last pad byte (byte 135)
//   others     : zero
// The permutation is restated from the Keccak reference (Bertoni, Daemen, Peeters, Van Assche, 2011, §1.2); host and
// device share this code (KHB_HD) so tests/native checks it on the CPU.
//
// gfx950 has a 32-bit VALU, so a lane is a register pair {lo, hi}.  A rotation is two v_alignbit_b32 (the halves
// swapped first for 32 or more), chi one v_bitop3_b32 per half, a column parity two xor3 per half; pi only renames
// registers.  One round is 20 (parities) + 20 (theta's D) + 50 (A ^ D) + 48 (rho) + 50 (chi) + 1..2 (iota) = ~190
// VALU.  KHB_KECCAK_ROLLED=1 (the product) keeps one copy of the round in a loop with the round constants in a
// table; =0 unrolls the 24 rounds, which folds round 0's 16 constant lanes and computes only the three lanes the
// address reads in round 23 (4,424 VALU per hash against 55 + 24 x 204 = 4,951 rolled, whose loop also copies the
// renamed lanes back) but puts three 4.4 k-instruction copies of the hash into the walk (one per point_xy call) and
// took 2-5 % more kernel time, with spills at 4 waves per SIMD (DESIGN.md §2b has both forms measured).
//
// Byte conventions: Fe limbs are little-endian words (v[7] most significant), so Get32Bytes(x) is the word stream
// x.v[7] ... x.v[0] big-endian and lane 0 = {lo = bswap32(x.v[7]), hi = bswap32(x.v[6])}.  The 20 address bytes are
// returned as five words whose little-endian bytes are the address bytes, the convention of hash160.hpp's outputs
// and of bloom_check20.
#pragma once
#include <stdint.h>
#include "fe.hpp"
#include "hash160.hpp"

#ifndef KHB_KECCAK_ROLLED
#define KHB_KECCAK_ROLLED 1
#endif

namespace khb {

// (a:b) >> s, low word: (b >> s) | (a << (32 - s)), 0 < s < 32
KHB_HD uint32_t funnel_r(uint32_t a, uint32_t b, int s) {
#ifdef __HIP_DEVICE_COMPILE__
  return __builtin_amdgcn_alignbit(a, b, (uint32_t)s);
#else
  return (b >> s) | (a << (32 - s));
#endif
}

// {rl, rh} = {l, h} rotated left by n, 0 <= n < 64
KHB_HD void rotl64(uint32_t& rl, uint32_t& rh, uint32_t l, uint32_t h, int n) {
  if (n >= 32) {
    const uint32_t t = l;
    l = h;
    h = t;
    n -= 32;
  }
  if (n == 0) {
    rl = l;
    rh = h;
  } else {
    rl = funnel_r(l, h, 32 - n);
    rh = funnel_r(h, l, 32 - n);
  }
}

// One round of Keccak-f[1600] on lanes A[x + 5y] = {lo, hi}: theta, rho and pi into B, chi, iota.
KHB_HD void keccak_round(uint32_t lo[25], uint32_t hi[25], uint32_t rc_lo, uint32_t rc_hi) {
  const uint8_t kRho[25] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};
  uint32_t cl[5], ch[5], dl[5], dh[5], bl[25], bh[25];
#pragma unroll
  for (int x = 0; x < 5; ++x) {
    cl[x] = xor3(xor3(lo[x], lo[x + 5], lo[x + 10]), lo[x + 15], lo[x + 20]);
    ch[x] = xor3(xor3(hi[x], hi[x + 5], hi[x + 10]), hi[x + 15], hi[x + 20]);
  }
#pragma unroll
  for (int x = 0; x < 5; ++x) {
    uint32_t rl, rh;
    rotl64(rl, rh, cl[(x + 1) % 5], ch[(x + 1) % 5], 1);
    dl[x] = cl[(x + 4) % 5] ^ rl;
    dh[x] = ch[(x + 4) % 5] ^ rh;
  }
#pragma unroll
  for (int i = 0; i < 25; ++i) {
    const int x = i % 5, y = i / 5, j = y + 5 * ((2 * x + 3 * y) % 5);
    rotl64(bl[j], bh[j], lo[i] ^ dl[x], hi[i] ^ dh[x], kRho[i]);
  }
#pragma unroll
  for (int y = 0; y < 25; y += 5) {
#pragma unroll
    for (int x = 0; x < 5; ++x) {
      lo[y + x] = chi3(bl[y + x], bl[y + (x + 1) % 5], bl[y + (x + 2) % 5]);
      hi[y + x] = chi3(bh[y + x], bh[y + (x + 1) % 5], bh[y + (x + 2) % 5]);
    }
  }
  lo[0] ^= rc_lo;
  hi[0] ^= rc_hi;
}

#define KHB_KECCAK_RC                                                                                          \
  {0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808Aull, 0x8000000080008000ull,                   \
   0x000000000000808Bull, 0x0000000080000001ull, 0x8000000080008081ull, 0x8000000000008009ull,                   \
   0x000000000000008Aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000Aull,                   \
   0x000000008000808Bull, 0x800000000000008Bull, 0x8000000000008089ull, 0x8000000000008003ull,                   \
   0x8000000000008002ull, 0x8000000000000080ull, 0x000000000000800Aull, 0x800000008000000Aull,                   \
   0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull}

KHB_HD void keccak_f1600(uint32_t lo[25], uint32_t hi[25]) {
  const uint64_t RC[24] = KHB_KECCAK_RC;
#if KHB_KECCAK_ROLLED
#pragma unroll 1
#else
#pragma unroll
#endif
  for (int r = 0; r < 24; ++r) keccak_round(lo, hi, (uint32_t)RC[r], (uint32_t)(RC[r] >> 32));
}

// The 20 address bytes of the public key (x, y), canonical: digest bytes 12..31 = the high half of lane 1 and
// lanes 2 and 3.
KHB_HD void eth_address(uint32_t h[5], const Fe& x, const Fe& y) {
  uint32_t lo[25], hi[25];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    lo[k] = bswap32(x.v[7 - 2 * k]);
    hi[k] = bswap32(x.v[6 - 2 * k]);
    lo[4 + k] = bswap32(y.v[7 - 2 * k]);
    hi[4 + k] = bswap32(y.v[6 - 2 * k]);
  }
#pragma unroll
  for (int k = 8; k < 25; ++k) lo[k] = hi[k] = 0;
  lo[8] = 0x01u;
  hi[16] = 0x80000000u;
  keccak_f1600(lo, hi);
  h[0] = hi[1];
  h[1] = lo[2];
  h[2] = hi[2];
  h[3] = lo[3];
  h[4] = hi[3];
}

}  // namespace khb
