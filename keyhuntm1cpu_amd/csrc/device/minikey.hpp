// -m minikeys (thread_process_minikeys, keyhunt.cpp:2338-2505): the candidate counter, the two fixed SHA-256 message
// shapes and the fixed-base multiplication k*G.  Host and device share this code (KHB_HD) so tests/native checks it on
// the CPU.
//
// Candidate: 'S' followed by 21 characters of a 58-character alphabet.  The 21 digits d[0..20], d[0] the most
// significant, form a counter in [0, 58^21) (124 bits); character j + 1 of the string is alphabet[d[j]].
//   valid   iff byte 0 of SHA-256(minikey || '?') is 0x00 (23 bytes, one block; keyhunt.cpp:2448-2453)
//   key     =   SHA-256(minikey) read big-endian (22 bytes, one block; keyhunt.cpp:2457-2461)
// Message words (big-endian, as sha256_block takes them): w[0] = 'S' c1 c2 c3, w[k] = c(4k) .. c(4k+3) for k = 1..4,
//   22 bytes: w[5] = c20 << 24 | c21 << 16 | 0x8000,            w[15] = 0xB0 (176 bits)
//   23 bytes: w[5] = c20 << 24 | c21 << 16 | '?' << 8 | 0x80,   w[15] = 0xB8 (184 bits)
// and w[6..14] = 0.  Inside a run of 58^2 consecutive candidates only w[5] and, every 58th step, its top byte change.
//
// k*G: windows of w bits (4, 8 or 16) over a table of affine points tab[j * (2^w - 1) + d - 1] = d * 2^(w j) * G,
// j < 256 / w, d in 1..2^w - 1 (64 x 15, 32 x 255 or 16 x 65,535 points of 64 bytes: 60 KiB, 510 KiB, 64 MiB), summed
// from the lowest window up in Jacobian coordinates with mixed additions and made affine by one inversion.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "confirm.hpp"
#include "fe.hpp"
#include "hash160.hpp"

namespace khb {

constexpr int kMiniDigits = 21;
constexpr uint32_t kMiniBase = 58;

// d += off over the 21 base-58 digits, d[0] the most significant.  False when the sum is 58^21 or more: there is no
// wrap in a search (the digits then hold the sum mod 58^21).
KHB_HD bool mini_add(uint8_t d[kMiniDigits], uint64_t off) {
  uint64_t c = off;
#pragma unroll
  for (int i = kMiniDigits - 1; i >= 0; --i) {
    uint64_t q = c / kMiniBase;                       // q + 1 cannot overflow: q <= 2^64 / 58
    uint32_t s = (uint32_t)(c - q * kMiniBase) + d[i];
    if (s >= kMiniBase) {
      s -= kMiniBase;
      q += 1;
    }
    d[i] = (uint8_t)s;
    c = q;
  }
  return c == 0;
}

// The next candidate's digits above d[from]: d[from], d[from - 1], ... += 1 with carry.  False on the carry out of d[0].
KHB_HD bool mini_carry(uint8_t d[kMiniDigits], int from) {
  bool c = true;
#pragma unroll
  for (int i = kMiniDigits - 1; i >= 0; --i) {
    if (i > from) continue;
    const uint32_t s = d[i] + (c ? 1u : 0u);
    c = s >= kMiniBase;
    d[i] = (uint8_t)(c ? 0u : s);
  }
  return !c;
}

// w[0..4]: the message words every shape shares (characters 0..19).  alphabet may be LDS or global memory.
KHB_HD void mini_pack_head(uint32_t w[5], const uint8_t* __restrict__ alphabet, const uint8_t d[kMiniDigits]) {
  w[0] = ((uint32_t)'S' << 24) | ((uint32_t)alphabet[d[0]] << 16) | ((uint32_t)alphabet[d[1]] << 8) | alphabet[d[2]];
#pragma unroll
  for (int k = 1; k < 5; ++k)
    w[k] = ((uint32_t)alphabet[d[4 * k - 1]] << 24) | ((uint32_t)alphabet[d[4 * k]] << 16) |
           ((uint32_t)alphabet[d[4 * k + 1]] << 8) | alphabet[d[4 * k + 2]];
}

// w[5] of the two shapes from characters 20 and 21.
KHB_HD uint32_t mini_w5_key(uint32_t c20, uint32_t c21) { return (c20 << 24) | (c21 << 16) | 0x8000u; }
KHB_HD uint32_t mini_w5_check(uint32_t c20, uint32_t c21) { return (c20 << 24) | (c21 << 16) | ((uint32_t)'?' << 8) | 0x80u; }

// The 16 message words of a candidate: check = the 23-byte shape (minikey || '?'), else the 22-byte shape.
KHB_HD void mini_pack(uint32_t w[16], const uint8_t* __restrict__ alphabet, const uint8_t d[kMiniDigits], bool check) {
  mini_pack_head(w, alphabet, d);
  const uint32_t c20 = alphabet[d[19]], c21 = alphabet[d[20]];
  w[5] = check ? mini_w5_check(c20, c21) : mini_w5_key(c20, c21);
#pragma unroll
  for (int k = 6; k < 15; ++k) w[k] = 0;
  w[15] = check ? 0xB8u : 0xB0u;
}

// SHA-256 state of the padded head words w[0..4] and w5 (w[6..14] = 0, w[15] = bits).
KHB_HD void mini_sha(uint32_t s[8], const uint32_t head[5], uint32_t w5, uint32_t bits) {
  uint32_t w[16];
#pragma unroll
  for (int k = 0; k < 5; ++k) w[k] = head[k];
  w[5] = w5;
#pragma unroll
  for (int k = 6; k < 15; ++k) w[k] = 0;
  w[15] = bits;
  sha256_init(s);
  sha256_block(s, w);
}

// What the candidates with the same first 20 characters share in the typo check's SHA-256: the state after the five
// rounds that read w[0..4], and the schedule words W16..W19, which w[5] does not reach (W20 is the first it does).
// The filter keeps this across a run of up to 58^2 candidates, so a candidate costs rounds 5..63 and W20..W63.
struct MiniPre {
  uint32_t st[8];
  uint32_t w16[4];
  uint32_t w4;
};

KHB_HD void mini_sha_round(uint32_t& a, uint32_t& b, uint32_t& c, uint32_t& d, uint32_t& e, uint32_t& f, uint32_t& g,
                           uint32_t& h, uint32_t k, uint32_t wi) {
  const uint32_t S1 = xor3(ror32(e, 6), ror32(e, 11), ror32(e, 25));
  const uint32_t ch = bitop3<0xCAu>(e, f, g);
  const uint32_t t1 = h + S1 + ch + k + wi;
  const uint32_t S0 = xor3(ror32(a, 2), ror32(a, 13), ror32(a, 22));
  const uint32_t maj = bitop3<0xE8u>(a, b, c);
  const uint32_t t2 = S0 + maj;
  h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
}
KHB_HD uint32_t mini_sig0(uint32_t x) { return xor3(ror32(x, 7), ror32(x, 18), x >> 3); }
KHB_HD uint32_t mini_sig1(uint32_t x) { return xor3(ror32(x, 17), ror32(x, 19), x >> 10); }

// bits: the message's w[15] (0xB8 for the typo check's 23 bytes); w[6..14] are zero.
KHB_HD void mini_pre(MiniPre& P, const uint32_t head[5], uint32_t bits) {
  const uint32_t K[64] = KHB_SHA_K;
  sha256_init(P.st);
  uint32_t a = P.st[0], b = P.st[1], c = P.st[2], d = P.st[3], e = P.st[4], f = P.st[5], g = P.st[6], h = P.st[7];
#pragma unroll
  for (int i = 0; i < 5; ++i) mini_sha_round(a, b, c, d, e, f, g, h, K[i], head[i]);
  P.st[0] = a; P.st[1] = b; P.st[2] = c; P.st[3] = d; P.st[4] = e; P.st[5] = f; P.st[6] = g; P.st[7] = h;
  P.w16[0] = head[0] + mini_sig0(head[1]);                           // + w[9] + sig1(w[14]), both zero
  P.w16[1] = head[1] + mini_sig0(head[2]) + mini_sig1(bits);         // + w[10]
  P.w16[2] = head[2] + mini_sig0(head[3]) + mini_sig1(P.w16[0]);     // + w[11]
  P.w16[3] = head[3] + mini_sig0(head[4]) + mini_sig1(P.w16[1]);     // + w[12]
  P.w4 = head[4];
}

// Word 0 of SHA-256 of the message whose first 20 bytes made P, with w[5] = w5: the typo check tests its top byte.
KHB_HD uint32_t mini_sha_word0(const MiniPre& P, uint32_t w5, uint32_t bits) {
  const uint32_t K[64] = KHB_SHA_K;
  uint32_t w[16];                  // the schedule ring as round 20 finds it: W16..W19 in place of w[0..3]
#pragma unroll
  for (int k = 0; k < 4; ++k) w[k] = P.w16[k];
  w[4] = P.w4;
  w[5] = w5;
#pragma unroll
  for (int k = 6; k < 15; ++k) w[k] = 0;
  w[15] = bits;
  uint32_t a = P.st[0], b = P.st[1], c = P.st[2], d = P.st[3], e = P.st[4], f = P.st[5], g = P.st[6], h = P.st[7];
#pragma unroll
  for (int i = 5; i < 64; ++i) {
    uint32_t wi;
    if (i < 20) {
      wi = w[i & 15];              // w[5..15] as packed, then the four precomputed words
    } else {
      wi = w[i & 15] = w[i & 15] + mini_sig0(w[(i - 15) & 15]) + w[(i - 7) & 15] + mini_sig1(w[(i - 2) & 15]);
    }
    mini_sha_round(a, b, c, d, e, f, g, h, K[i], wi);
  }
  return 0x6a09e667u + a;
}

// The typo check of the candidate with digits d.
KHB_HD bool mini_valid(const uint8_t* __restrict__ alphabet, const uint8_t d[kMiniDigits]) {
  uint32_t w[16], s[8];
  mini_pack(w, alphabet, d, true);
  sha256_init(s);
  sha256_block(s, w);
  return (s[0] >> 24) == 0;
}

// The private key of the candidate with digits d: the digest's word 0 is the scalar's most significant word.
KHB_HD void mini_key(U8& k, const uint8_t* __restrict__ alphabet, const uint8_t d[kMiniDigits]) {
  uint32_t w[16], s[8];
  mini_pack(w, alphabet, d, false);
  sha256_init(s);
  sha256_block(s, w);
#pragma unroll
  for (int i = 0; i < 8; ++i) k.v[7 - i] = s[i];
}

// 0 < k < n, n the group order: a key outside has no public key (a "bad key").
KHB_HD bool mini_scalar_ok(const U8& k) {
  const uint32_t n[8] = {0xD0364141u, 0xBFD25E8Cu, 0xAF48A03Bu, 0xBAAEDCE6u, 0xFFFFFFFEu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
  uint32_t any = 0;
  int64_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    any |= k.v[i];
    c = (int64_t)k.v[i] - (int64_t)n[i] + (c >> 32);
  }
  return any != 0 && c < 0;     // the borrow out of k - n
}

// acc += q (q affine, never the point at infinity), acc at infinity iff inf.  The sum is computed by the one mixed
// addition formula whatever inf says and (q, z = 1) is selected over it afterwards, so the lanes of a wave do not part
// on it.  There is no doubling path and none to the point at infinity: mini_mul_g's operands never need one.
KHB_HD void mini_madd(JPt& acc, const CPt& q) {
  Fe z1z1, u2, s2, h, rr, hh, hhh, v, x3, y3, z3, t;
  fe_sqr(z1z1, acc.z);
  fe_mul(u2, q.x, z1z1);
  fe_mul(s2, q.y, acc.z);
  fe_mul(s2, s2, z1z1);
  fe_sub(h, u2, acc.x);
  fe_sub(rr, s2, acc.y);
  fe_sqr(hh, h);
  fe_mul(hhh, h, hh);
  fe_mul(v, acc.x, hh);
  fe_sqr(x3, rr);
  fe_sub(x3, x3, hhh);
  fe_sub(x3, x3, v);
  fe_sub(x3, x3, v);
  fe_sub(t, v, x3);
  fe_mul(y3, rr, t);
  fe_mul(t, acc.y, hhh);
  fe_sub(y3, y3, t);
  fe_mul(z3, acc.z, h);
  const bool inf = acc.inf;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    acc.x.v[i] = inf ? q.x.v[i] : x3.v[i];
    acc.y.v[i] = inf ? q.y.v[i] : y3.v[i];
    acc.z.v[i] = inf ? (i == 0 ? 1u : 0u) : z3.v[i];
  }
  acc.inf = false;
}

// r = k*G for 0 < k < n over the window table `tab` of width wbits (4, 8 or 16); a zero window is skipped.
// Before window j the sum is (k mod 2^(w j))*G and the point added is d*2^(w j)*G with
//   k mod 2^(w j) < 2^(w j) <= d*2^(w j) < n,
// so the two scalars differ and an addition never meets its own point (no doubling).  Their sum is at most k, so it
// is n -- the addition meets its negative -- only for k = n itself: callers test mini_scalar_ok and never use the
// result of a bad key (what this returns for one is unspecified, and no memory outside the table is read for it).
KHB_HD void mini_mul_g(CPt& r, const U8& k, const CPt* __restrict__ tab, uint32_t wbits) {
  JPt acc;
  acc.x = Fe{};
  acc.y = Fe{};
  acc.z = Fe{};
  acc.inf = true;
  U8 s = k;
  const uint32_t mask = (1u << wbits) - 1u, nwin = 256u / wbits;
#pragma unroll 1
  for (uint32_t j = 0; j < nwin; ++j) {
    const uint32_t d = s.v[0] & mask;
#pragma unroll
    for (int i = 0; i < 7; ++i) s.v[i] = (s.v[i] >> wbits) | (s.v[i + 1] << (32u - wbits));
    s.v[7] >>= wbits;
    if (d) {
      const CPt q = tab[(size_t)j * mask + d - 1];
      mini_madd(acc, q);
    }
  }
  if (acc.inf) {                 // k = 0: a bad key
    r.x = Fe{};
    r.y = Fe{};
    return;
  }
  Fe zi, zi2, zi3;
  fe_inv(zi, acc.z);
  fe_sqr(zi2, zi);
  fe_mul(zi3, zi2, zi);
  fe_mul(r.x, acc.x, zi2);
  fe_mul(r.y, acc.y, zi3);
}

// Points of a table of width wbits.
KHB_HD size_t mini_table_points(uint32_t wbits) { return (size_t)(256u / wbits) * ((1u << wbits) - 1u); }

}  // namespace khb
