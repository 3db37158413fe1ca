// gfx950 fast path for the secp256k1 field: 8 x 32-bit limbs, hand-placed carry chains.
//
// Why: the scan kernel is VALU-issue-bound (profiles/r01_pmc.txt).  The portable fe.hpp compiles
// to 390 VALU instructions per multiply — 216 of them v_mov_b32 materialising zero-extended
// 64-bit addends.  Here each 32x32 partial product is one v_mad_u64_u32 whose carry-out (VCC)
// is absorbed by one VOP2 v_addc_co_u32 (product scanning), and add/sub are single carry chains.
// How the file came to this form, and what was tried and left out: DESIGN.md §2a (field arithmetic), §5.
//
// Value contract (checked by tests/test_gpu_scan.py::test_field_ops and every x-dump test):
//   * fm_mul / fm_sqr / fm_sqr_add return a value < 2^256 congruent to the result mod p, not necessarily
//     < p ("lazy").  The lazy value is a function of the operands alone: the same for every lane whether
//     or not its wave took a rare branch (tests/field_model.py defines it on integers;
//     tests/test_gpu_field_directed.py compares it in raw mode).
//   * fm_add_lazy(a, b) takes a < p, b < 2^256 and returns a lazy value.
//   * fm_sub(a, b) is correct for a < 2^256 and b < p; its result is < 2^256 (< p if it borrowed).
//   * fm_add(a, b) needs a, b < p and returns a canonical value.
//   * fm_canon brings any value < 2^256 into [0, p).  Values that are hashed, compared or used as a
//     subtrahend (x-coordinates, centres) are canonicalised, so every observable equals the
//     reference's canonical Int (IntMod.cpp) bit for bit.
//
// Hazard rules.  hipcc pads its own carry chains (seen in its ISA for __builtin_addc) but nothing inside
// an asm string (cdna_hip_programming.md §5.7 item 2), so the pads are written out:
//   * KHB_NOP (`s_nop 0`): a VALU that writes VCC (v_add_co / v_sub_co / v_mad_u64_u32 carry-out) needs one
//     wait state before a VALU reads that VCC as carry-in.  Every carry consumer is preceded by it.
//   * `s_nop 1` ahead of a VALU read (v_cndmask's select mask) of an SGPR pair that a VALU wrote:
//     fm_mask_bit and fm_fix_R.  Scalar reads of such a pair (s_or_b64, s_cmp) are interlocked: no pad.
//
// Rare carries.  A carry or borrow that is set with probability 2^-22 or less per call (each function
// gives its own figure) is not propagated on the common path.  The instruction that produces it, in its
// VOP3 form (v_addc / v_subb / v_mad_u64_u32; carry-in still VCC), writes it as a lane mask to an SGPR
// pair instead of VCC; a function's masks are ORed and tested on the scalar unit (fm_any_mask), and one
// wave-uniform branch, taken when some lane needs it, turns each mask into a per-lane 0/1 (fm_mask_bit)
// and does the full propagation: a no-op for lanes whose bit is 0.  Against "v_addc c, vcc, 0, 0, vcc" +
// a v_cmp for a ballot that is two half-rate VALU instructions less per call.  The hardware writes 0 to
// the mask bits of lanes that are inactive at the write, so a lane that sits out cannot raise the branch;
// a stale bit could only send the wave through a body that leaves that lane alone (it is still inactive
// there) and adds 0 in every other lane.
#pragma once
#include <stdint.h>
#include <utility>

#include "fe.hpp"

namespace khb {

#define FM_DEV __device__ __forceinline__

// The one wait state between a VCC (carry) write and its VALU reader.  (A timing-only build without it
// was 1.1 % faster, profiles/r01_nonop_ab.txt; the pads stay as the hazard rule asks.)
#define KHB_NOP "s_nop 0\n\t"
#if KHB_RARE_FORCE    // test builds: always take the rare branch (its full propagation is a no-op at c = 0)
FM_DEV bool fm_any(uint32_t) { return true; }
FM_DEV bool fm_any_mask(uint64_t) { return true; }
#else
FM_DEV bool fm_any(uint32_t c) { return __builtin_expect(__ballot(c != 0) != 0, 0); }
FM_DEV bool fm_any_mask(uint64_t m) { return __builtin_expect(m != 0, 0); }
#endif
// The lane's bit of a carry mask as 0/1; only inside a rare branch.
FM_DEV uint32_t fm_mask_bit(uint64_t m) {
  uint32_t c;
  asm("s_nop 1\n\t"
      "v_cndmask_b32_e64 %0, 0, 1, %1" : "=v"(c) : "s"(m));
  return c;
}

// r[k..7] += c (c in {0, 1} per lane), carry-out returned.
template <int K>
FM_DEV uint32_t fm_propagate(uint32_t* r, uint32_t c) {
  uint32_t co = c;
#pragma unroll
  for (int i = K; i < 8; ++i) {
    const uint64_t t = (uint64_t)r[i] + co;
    r[i] = (uint32_t)t;
    co = (uint32_t)(t >> 32);
  }
  return co;
}

// acc += a*b ; c2 += carry-out
FM_DEV void fm_madc(uint64_t& acc, uint32_t& c2, uint32_t a, uint32_t b) {
  asm("v_mad_u64_u32 %0, vcc, %2, %3, %0\n\t"
      KHB_NOP
      "v_addc_co_u32_e32 %1, vcc, 0, %1, vcc"
      : "+v"(acc), "+v"(c2)
      : "v"(a), "v"(b)
      : "vcc");
}

// ---- 512-bit products with forward-carried columns -------------------------------------------
// Column K (sum of a_i*b_{K-i}) accumulates in one 64-bit pair S whose two halves weigh 2^(32K) and
// 2^(32K+32); the carries out of S (weight 2^(32K+64)) are counted in cw.  The next column's pair starts as
//   {lo = hi(S), hi = cw}
// which is exactly what column K hands on: both words weigh in column K+1 what the halves of its own pair
// weigh.  So the column's first mad adds the carried word for nothing, t[K] = lo(S) with no fold chain
// behind the columns, and two pairs are live at a time instead of fifteen.  Column 14 (one product, or
// none in the squaring's cross sum) leaves t[14], t[15] as its two halves: the whole product is < 2^512.
//
// The first product of a column is a mad without a carry count.  A product is at most (2^32 - 1)^2 =
// 2^64 - 2^33 + 1, so that is exact while the seed is <= 2^33 - 2: always when the column before holds one
// or two products (then what it hands on, floor(total / 2^32), stays below that), not always when it holds
// three or more (cw >= 2, or cw = 1 under a full high word): columns 3..13 of a product, 6..10 of the cross
// sum (FmCol::masked works the bound out).  It takes a first product within 2^35 of 2^64 (~2^-29 per column
// for random limbs; certain for all-ones operands).  Those columns' first mad writes its carry-out to an
// SGPR pair of its own (VOP3 always names a scalar destination: no instruction more) and the rare branch
// adds the dropped carries back: the one out of column K weighs 2^(32(K+2)), and since everything after
// the drop was computed exactly from the smaller count, t falls short of the product by exactly those
// bits (fm_fix_cols, one chain).

// acc += a*b; cw = carry-out (first carry of a column: no zero-initialisation needed)
FM_DEV void fm_madc_first(uint64_t& acc, uint32_t& cw, uint32_t a, uint32_t b) {
  asm("v_mad_u64_u32 %0, vcc, %2, %3, %0\n\t"
      KHB_NOP
      "v_addc_co_u32_e32 %1, vcc, 0, %4, vcc"
      : "+v"(acc), "=v"(cw)
      : "v"(a), "v"(b), "v"(0u)
      : "vcc");
}

// acc += a*b; co = lane mask of the carry-out (a column's first product on a seed that can reach 2^33 - 1)
FM_DEV void fm_mad_seed(uint64_t& acc, uint64_t& co, uint32_t a, uint32_t b) {
  asm("v_mad_u64_u32 %0, %1, %2, %3, %0" : "+v"(acc), "=s"(co) : "v"(a), "v"(b));
}

// The products of a column after its first: cw receives their carries.
template <int LO, int HI, int K>
FM_DEV void fm_col_rest(uint64_t& A, uint32_t& cw, const uint32_t* a, const uint32_t* b) {
  if constexpr (HI > LO) {
    fm_madc_first(A, cw, a[LO + 1], b[K - LO - 1]);
#pragma unroll
    for (int i = LO + 2; i <= HI; ++i) fm_madc(A, cw, a[i], b[K - i]);
  }
}

// The pair column K+1 starts from: the high word of column K's pair and its carry count.
FM_DEV uint64_t fm_col_next(uint64_t S, uint32_t cw) { return ((uint64_t)cw << 32) | (uint32_t)(S >> 32); }

// The shape of column K: the products a_i b_{K-i}, lo <= i <= hi, of a*b, or (SQ) of the cross sum
// sum_{i<j} a_i a_j 2^(32(i+j)), whose pairs are i < K-i with b = a.
template <int K, bool SQ>
struct FmCol {
  static constexpr int count(int k) {           // products in column k
    const int l = k > 7 ? k - 7 : 0, h = SQ ? (k - 1) / 2 : (k < 7 ? k : 7);
    return k < (SQ ? 1 : 0) || h < l ? 0 : h - l + 1;
  }
  // The first product can overflow its seed: the most column k-1 hands on, floor(total / 2^32) with every
  // product at its maximum, plus one such product passes 2^64 (tests/field_columns.py unsafe_columns).
  static constexpr bool unsafe(int k) {
    constexpr uint64_t pmax = 0xFFFFFFFE00000001ull;   // (2^32 - 1)^2
    unsigned __int128 v = 0;
    for (int j = 0; j < k; ++j) v = (count(j) * (unsigned __int128)pmax + v) >> 32;
    return count(k) && v + pmax > ~0ull;
  }
  static constexpr int first_unsafe(int k) { return unsafe(k) ? k : first_unsafe(k + 1); }
  static constexpr int lo = K > 7 ? K - 7 : 0, hi = SQ ? (K - 1) / 2 : (K < 7 ? K : 7);
  static constexpr int n = count(K), first_masked = first_unsafe(0);
  static constexpr bool masked = unsafe(K);
};
static_assert(!FmCol<2, false>::masked && FmCol<3, false>::masked && FmCol<13, false>::masked &&
              !FmCol<14, false>::masked, "fm_mul512x: m[0..10] are columns 3..13");
static_assert(!FmCol<5, true>::masked && FmCol<6, true>::masked && FmCol<10, true>::masked &&
              !FmCol<11, true>::masked, "fm_sqr512x: m[0..4] are columns 6..10");

// Column K on top of column K-1: the seed, the products, t[K].  A column of one product hands on its high
// word alone (its cw is not written).  m[K - first_masked] receives a masked column's first carry-out.
template <int K, bool SQ>
FM_DEV void fm_col(uint32_t* t, uint64_t& S, uint32_t& cw, uint64_t* m, const uint32_t* a, const uint32_t* b) {
  using C = FmCol<K, SQ>;
  if constexpr (FmCol<K - 1, SQ>::n >= 2) S = fm_col_next(S, cw); else S >>= 32;
  if constexpr (C::masked) fm_mad_seed(S, m[K - C::first_masked], a[C::lo], b[K - C::lo]);
  else S += (uint64_t)a[C::lo] * b[K - C::lo];
  fm_col_rest<C::lo, C::hi, K>(S, cw, a, b);
  t[K] = (uint32_t)S;
}

template <bool SQ, int K0, int... I>   // columns K0 + I, in order
FM_DEV void fm_cols(uint32_t* t, uint64_t& S, uint32_t& cw, uint64_t* m, const uint32_t* a, const uint32_t* b,
                    std::integer_sequence<int, I...>) {
  (fm_col<K0 + I, SQ>(t, S, cw, m, a, b), ...);
}

// w[0..W-1] += sum_i bit_i 2^(32i), bit_i the lane's bit of mask m[i] (i < N): w[0] is the word two above
// the first masked column.  Nothing leaves w[W-1]: with the bits in, the words are those of the product.
// (The reduction's fm_fix_R is the same thing written as one asm chain, and stays that: as
// fm_fix_cols<8, 8> on a 10-word R it costs k_giant_scan<0, 7, 8, 9> 256 bytes of scratch against 160-168.)
template <int N, int W>
FM_DEV void fm_fix_cols(uint32_t* w, const uint64_t* m) {
  uint32_t c = 0;
#pragma unroll
  for (int i = 0; i < W; ++i) {
    uint64_t s = (uint64_t)w[i] + c;
    if (i < N) s += fm_mask_bit(m[i]);
    w[i] = (uint32_t)s;
    c = (uint32_t)(s >> 32);
  }
}

FM_DEV void fm_mul512x(uint32_t t[16], const uint32_t* a, const uint32_t* b) {
  uint64_t S = (uint64_t)a[0] * b[0];
  uint64_t m[11];                     // first-product carry-outs of columns 3..13
  uint32_t cw;
  t[0] = (uint32_t)S;
  fm_cols<false, 1>(t, S, cw, m, a, b, std::make_integer_sequence<int, 14>{});   // columns 1..14
  t[15] = (uint32_t)(S >> 32);
  if (fm_any_mask(m[0] | m[1] | m[2] | m[3] | m[4] | m[5] | m[6] | m[7] | m[8] | m[9] | m[10]))
    fm_fix_cols<11, 11>(t + 5, m);
}

// a^2 = 2*cross + diag: 36 products instead of 64.
FM_DEV void fm_sqr512x(uint32_t t[16], const uint32_t* a) {
  // Cross sum c, columns carried forward as in fm_mul512x.  Only columns 3..11 hold two or more cross
  // products and count carries; columns 1, 2, 12, 13 hold one and column 14 none (7,7 is diagonal), so c[14]
  // is column 13's high word and c[15] = 0: the cross sum is < 2^481, with the dropped carries back in too.
  uint32_t c[16];
  uint64_t S = (uint64_t)a[0] * a[1];
  uint64_t m[5];                      // first-product carry-outs of columns 6..10
  uint32_t cw;
  c[0] = 0u;
  c[1] = (uint32_t)S;
  fm_cols<true, 2>(c, S, cw, m, a, a, std::make_integer_sequence<int, 12>{});    // columns 2..13
  c[14] = (uint32_t)(S >> 32);
  c[15] = 0u;
  if (fm_any_mask(m[0] | m[1] | m[2] | m[3] | m[4])) fm_fix_cols<5, 7>(c + 8, m);
  uint64_t D[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) D[i] = (uint64_t)a[i] * a[i];
  // t = D + 2c: the doubled cross sum by one funnel shift per word (v_alignbit_b32, no carry flag:
  // (c_k << 1) | (c_k-1 >> 31); c[0] = 0, and 2c < 2^512 since a^2 < 2^512), then one carry chain
  // instead of adding c twice.
  uint32_t c2[16];
  c2[0] = 0u;
  c2[1] = c[1] << 1;
#pragma unroll
  for (int k = 2; k < 16; ++k) c2[k] = __builtin_amdgcn_alignbit(c[k], c[k - 1], 31);
  uint32_t u[16];
  u[0] = (uint32_t)D[0];
  asm("v_add_co_u32_e32 %0, vcc, %15, %30\n\t"
      KHB_NOP
      "v_addc_co_u32_e32 %1, vcc, %16, %31, vcc\n\t"
      KHB_NOP
      "v_addc_co_u32_e32 %2, vcc, %17, %32, vcc\n\t"
      KHB_NOP
      "v_addc_co_u32_e32 %3, vcc, %18, %33, vcc\n\t"
      KHB_NOP
      "v_addc_co_u32_e32 %4, vcc, %19, %34, vcc\n\t"
      KHB_NOP
      "v_addc_co_u32_e32 %5, vcc, %20, %35, vcc\n\t"
      KHB_NOP
      "v_addc_co_u32_e32 %6, vcc, %21, %36, vcc\n\t"
      KHB_NOP
      "v_addc_co_u32_e32 %7, vcc, %22, %37, vcc\n\t"
      KHB_NOP
      "v_addc_co_u32_e32 %8, vcc, %23, %38, vcc\n\t"
      KHB_NOP
      "v_addc_co_u32_e32 %9, vcc, %24, %39, vcc\n\t"
      KHB_NOP
      "v_addc_co_u32_e32 %10, vcc, %25, %40, vcc\n\t"
      KHB_NOP
      "v_addc_co_u32_e32 %11, vcc, %26, %41, vcc\n\t"
      KHB_NOP
      "v_addc_co_u32_e32 %12, vcc, %27, %42, vcc\n\t"
      KHB_NOP
      "v_addc_co_u32_e32 %13, vcc, %28, %43, vcc\n\t"
      KHB_NOP
      "v_addc_co_u32_e32 %14, vcc, %29, %44, vcc"
      : "=&v"(u[1]), "=&v"(u[2]), "=&v"(u[3]), "=&v"(u[4]), "=&v"(u[5]), "=&v"(u[6]), "=&v"(u[7]), "=&v"(u[8]),
        "=&v"(u[9]), "=&v"(u[10]), "=&v"(u[11]), "=&v"(u[12]), "=&v"(u[13]), "=&v"(u[14]), "=&v"(u[15])
      : "v"((uint32_t)(D[0] >> 32)), "v"((uint32_t)D[1]), "v"((uint32_t)(D[1] >> 32)),
        "v"((uint32_t)D[2]), "v"((uint32_t)(D[2] >> 32)), "v"((uint32_t)D[3]), "v"((uint32_t)(D[3] >> 32)),
        "v"((uint32_t)D[4]), "v"((uint32_t)(D[4] >> 32)), "v"((uint32_t)D[5]), "v"((uint32_t)(D[5] >> 32)),
        "v"((uint32_t)D[6]), "v"((uint32_t)(D[6] >> 32)), "v"((uint32_t)D[7]), "v"((uint32_t)(D[7] >> 32)),
        "v"(c2[1]), "v"(c2[2]), "v"(c2[3]), "v"(c2[4]), "v"(c2[5]), "v"(c2[6]), "v"(c2[7]), "v"(c2[8]),
        "v"(c2[9]), "v"(c2[10]), "v"(c2[11]), "v"(c2[12]), "v"(c2[13]), "v"(c2[14]), "v"(c2[15])
      : "vcc");
#pragma unroll
  for (int i = 0; i < 16; ++i) t[i] = u[i];
}

// ---- reduction mod p: 2^256 = 2^32 + 977 applied limb by limb ---------------------------------
// With L, H the halves of the 512-bit product (Lw = L, or L + w for fm_reduce_add, with its carry
// Lw8), the value to fold is  S = Lw + Lw8 2^256 + (H << 32) + 977 H.  Per limb that is
//   V_i = 977 H_i + (H_i : Lw_i)                                     (sum_i V_i 2^(32i) + Lw8 2^256 == S)
// one v_mad_u64_u32 whose 64-bit addend is the register pair {lo = Lw_i, hi = H_i}: no carry chain
// for Lw + (H << 32) and no zero-extended addend.  V_i < 2^64 + 977 2^32, so the mad carries out
// when H_i >= ~2^32 - 978 (2^-22 per limb for random limbs, certain for operands near p): each mad has
// a mask of its own (ov_i).  The chain R = sum_i lo64(V_i) 2^(32i) + Lw8 2^256 runs on the truncated
// V_i, and the rare branch adds the dropped carries back: the one out of V_i weighs 2^(32(i+2)), a 0/1
// addend of R's word i+2 (fm_fix_R, one chain over words 2..9).  After it R is S as 10 words.  The second
// fold adds top (2^32 + 977), top = R9:R8, to R[7..0].  R9 and the two carries out of the folded limbs are
// masks too, tested together with the ov_i: the common path has no R9 register and folds R8 alone in one
// mad (fm_reduce_V); the rare branch holds the fold in its general form (fm_fold2).

// d = a*k + c (c a 64-bit register pair); co = lane mask of the carry-out.  k comes from an SGPR (VOP3
// takes no literal on gfx9; one scalar source per instruction is the constant-bus limit).
FM_DEV void fm_mad_co(uint64_t& d, uint64_t& co, uint32_t a, uint32_t k, uint64_t c) {
  asm("v_mad_u64_u32 %0, %1, %2, %3, %4" : "=v"(d), "=s"(co) : "v"(a), "s"(k), "v"(c));
}

// V = 977*h + (h : lw); ov = lane mask of the carry-out.
FM_DEV void fm_madv(uint64_t& V, uint64_t& ov, uint32_t h, uint32_t lw, uint32_t k977) {
  fm_mad_co(V, ov, h, k977, ((uint64_t)h << 32) | lw);
}

// R8:R[7..0] = sum_i V_i 2^(32i) + T8 2^256 (mod 2^288): one carry chain.  The carry out of R8 -- R9, the
// tenth word -- is not materialised: the add that produces R8 writes it to the lane mask m9 (VOP3 form).
// R[1] overwrites the high word of V_0, so that R[1]:R[0] stays the register pair the second fold's mad
// takes as its addend.
FM_DEV void fm_chain_R(uint32_t R[8], uint32_t& R8, uint64_t& m9, const uint64_t V[8], uint32_t T8) {
  R[0] = (uint32_t)V[0];
  R[1] = (uint32_t)(V[0] >> 32);
  asm("v_add_co_u32_e32 %0, vcc, %9, %0\n\t"
      KHB_NOP
      "v_addc_co_u32_e32 %1, vcc, %10, %11, vcc\n\t"
      KHB_NOP
      "v_addc_co_u32_e32 %2, vcc, %12, %13, vcc\n\t"
      KHB_NOP
      "v_addc_co_u32_e32 %3, vcc, %14, %15, vcc\n\t"
      KHB_NOP
      "v_addc_co_u32_e32 %4, vcc, %16, %17, vcc\n\t"
      KHB_NOP
      "v_addc_co_u32_e32 %5, vcc, %18, %19, vcc\n\t"
      KHB_NOP
      "v_addc_co_u32_e32 %6, vcc, %20, %21, vcc\n\t"
      KHB_NOP
      "v_addc_co_u32_e64 %7, %8, %22, %23, vcc"
      : "+v"(R[1]), "=&v"(R[2]), "=&v"(R[3]), "=&v"(R[4]), "=&v"(R[5]), "=&v"(R[6]), "=&v"(R[7]),
        "=&v"(R8), "=s"(m9)
      : "v"((uint32_t)V[1]),
        "v"((uint32_t)V[2]), "v"((uint32_t)(V[1] >> 32)),
        "v"((uint32_t)V[3]), "v"((uint32_t)(V[2] >> 32)),
        "v"((uint32_t)V[4]), "v"((uint32_t)(V[3] >> 32)),
        "v"((uint32_t)V[5]), "v"((uint32_t)(V[4] >> 32)),
        "v"((uint32_t)V[6]), "v"((uint32_t)(V[5] >> 32)),
        "v"((uint32_t)V[7]), "v"((uint32_t)(V[6] >> 32)),
        "v"(T8), "v"((uint32_t)(V[7] >> 32))
      : "vcc");
}

// R9:R8:R[7..2] += sum_i ov_i 2^(32i) with ov_i the lane's bit of mask ov[i] (the carry out of V_i):
// eight v_cndmask reading the SGPR masks, one carry chain.  S < 2^290, so nothing leaves R9.  The
// masks were written by VALU (the mads) a whole R chain earlier; the leading pad keeps the distance
// whatever is scheduled in between.
FM_DEV void fm_fix_R(uint32_t R[8], uint32_t& R8, uint32_t& R9, const uint64_t ov[8]) {
  uint32_t c[8];
  asm("s_nop 1\n\t"
      "v_cndmask_b32_e64 %8, 0, 1, %16\n\t"
      "v_cndmask_b32_e64 %9, 0, 1, %17\n\t"
      "v_cndmask_b32_e64 %10, 0, 1, %18\n\t"
      "v_cndmask_b32_e64 %11, 0, 1, %19\n\t"
      "v_cndmask_b32_e64 %12, 0, 1, %20\n\t"
      "v_cndmask_b32_e64 %13, 0, 1, %21\n\t"
      "v_cndmask_b32_e64 %14, 0, 1, %22\n\t"
      "v_cndmask_b32_e64 %15, 0, 1, %23\n\t"
      "v_add_co_u32_e32 %0, vcc, %0, %8\n\t"
      KHB_NOP
      "v_addc_co_u32_e32 %1, vcc, %1, %9, vcc\n\t"
      KHB_NOP
      "v_addc_co_u32_e32 %2, vcc, %2, %10, vcc\n\t"
      KHB_NOP
      "v_addc_co_u32_e32 %3, vcc, %3, %11, vcc\n\t"
      KHB_NOP
      "v_addc_co_u32_e32 %4, vcc, %4, %12, vcc\n\t"
      KHB_NOP
      "v_addc_co_u32_e32 %5, vcc, %5, %13, vcc\n\t"
      KHB_NOP
      "v_addc_co_u32_e32 %6, vcc, %6, %14, vcc\n\t"
      KHB_NOP
      "v_addc_co_u32_e32 %7, vcc, %7, %15, vcc"
      : "+v"(R[2]), "+v"(R[3]), "+v"(R[4]), "+v"(R[5]), "+v"(R[6]), "+v"(R[7]), "+v"(R8), "+v"(R9),
        "=&v"(c[0]), "=&v"(c[1]), "=&v"(c[2]), "=&v"(c[3]), "=&v"(c[4]), "=&v"(c[5]), "=&v"(c[6]), "=&v"(c[7])
      : "s"(ov[0]), "s"(ov[1]), "s"(ov[2]), "s"(ov[3]), "s"(ov[4]), "s"(ov[5]), "s"(ov[6]), "s"(ov[7])
      : "vcc");
}

// The second fold in its general form: R[7..0] += top (2^32 + 977) for top = R9:R8 < 3 * 2^32, carries
// and the wrap past 2^256 included.  Only reached through fm_reduce_V's rare branch.
FM_DEV void fm_fold2(uint32_t R[8], uint32_t R8, uint32_t R9) {
  // add top*977 at limb 0 and top*2^32 at limb 1
  const uint64_t u = (uint64_t)R8 * 977u + (uint64_t)(R9 * 977u) * 0x100000000ull;   // < 2^44
  const uint64_t w = (uint64_t)(uint32_t)(u >> 32) + R8;                              // limb-1 addend
  const uint32_t w2 = (uint32_t)(w >> 32) + R9;                                       // limb-2 addend (<= 3)
  uint32_t c;
  // limbs 0..2 take the addends; the carry into limb 3 (probability ~2^-30) is propagated, and
  // a wrap past 2^256 (~2^-212) folded, only in the rare branch.
  uint32_t c3;
  asm("v_add_co_u32_e32 %0, vcc, %0, %4\n\t"
      KHB_NOP
      "v_addc_co_u32_e32 %1, vcc, %1, %5, vcc\n\t"
      KHB_NOP
      "v_addc_co_u32_e32 %2, vcc, %2, %6, vcc\n\t"
      KHB_NOP
      "v_addc_co_u32_e32 %3, vcc, 0, %7, vcc"
      : "+v"(R[0]), "+v"(R[1]), "+v"(R[2]), "=&v"(c3)
      : "v"((uint32_t)u), "v"((uint32_t)w), "v"(w2), "v"(0u)
      : "vcc");
  if (fm_any(c3)) {
    c = fm_propagate<3>(R, c3);
    const uint32_t k0 = c * 977u;
    uint64_t t = (uint64_t)R[0] + k0;
    R[0] = (uint32_t)t;
    t = (uint64_t)R[1] + c + (t >> 32);
    R[1] = (uint32_t)t;
    fm_propagate<2>(R, (uint32_t)(t >> 32));
  }
}

// Lw + Lw8 2^256 + H (2^32 + 977) -> a value < 2^256 congruent to it (lazy).
FM_DEV void fm_reduce_V(Fe& r, const uint32_t* Lw, uint32_t Lw8, const uint32_t* H) {
  uint64_t V[8], ov[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) fm_madv(V[i], ov[i], H[i], Lw[i], 977u);
  uint32_t R[8], R8;
  uint64_t m9;                        // lane mask of R9 (0/1 before the carry fix)
  fm_chain_R(R, R8, m9, V, Lw8);
  // Second fold, common form (R9 = 0, no V carry): R + R8 (2^32 + 977) over limbs 0..2 is
  //   m = R8*977 + (R1:R0)   one mad on the register pair, carry-out o (R1:R0 >= 2^64 - 977 R8: ~2^-22)
  //   R0' = lo(m), R1' = hi(m) + R8, R2' = R2 + carry, with the carry out of R2' in the mask c2m
  // written to registers of their own.  It is the general fold's value unless o is set (the mad dropped
  // 2^64); c2m is the general fold's c3.  One wave-uniform branch on every mask then redoes the fold in
  // its general form from the untouched R0, R1, R2, R8, for all lanes of the wave: a lane the common
  // form was right for gets the same three words again.
  const uint64_t r01 = ((uint64_t)R[1] << 32) | R[0];
  uint64_t m, o, c2m;
  uint32_t n1, n2;
  fm_mad_co(m, o, R8, 977u, r01);
  n1 = (uint32_t)(m >> 32);           // R1' takes the place of hi(m): R1':R0' stays a pair, no copy
  asm("v_add_co_u32_e32 %0, vcc, %3, %0\n\t"
      KHB_NOP
      "v_addc_co_u32_e64 %1, %2, 0, %4, vcc"
      : "+v"(n1), "=&v"(n2), "=s"(c2m)
      : "v"(R8), "v"(R[2])
      : "vcc");
  const uint64_t anyov = ov[0] | ov[1] | ov[2] | ov[3] | ov[4] | ov[5] | ov[6] | ov[7];
  r.v[0] = (uint32_t)m;
  r.v[1] = n1;
  r.v[2] = n2;
#pragma unroll
  for (int i = 3; i < 8; ++i) r.v[i] = R[i];
  if (fm_any_mask(anyov | m9 | o | c2m)) {
    uint32_t R9 = fm_mask_bit(m9);    // top = R9:R8 < 3 * 2^32 once the carries are in
    if (fm_any_mask(anyov)) fm_fix_R(R, R8, R9, ov);
    fm_fold2(R, R8, R9);
#pragma unroll
    for (int i = 0; i < 8; ++i) r.v[i] = R[i];
  }
}

// Reduce t (512 bits) mod p to a value < 2^256 (lazy).
FM_DEV void fm_reduce(Fe& r, const uint32_t t[16]) { fm_reduce_V(r, t, 0u, t + 8); }

// s = a + b mod 2^256 as one carry chain; the carry out of limb 7 (0/1) is returned.
FM_DEV uint32_t fm_add8(uint32_t s[8], const uint32_t* a, const uint32_t* b) {
  uint32_t c;
  asm("v_add_co_u32_e32 %0, vcc, %9, %17\n\t"
      KHB_NOP
      "v_addc_co_u32_e32 %1, vcc, %10, %18, vcc\n\t"
      KHB_NOP
      "v_addc_co_u32_e32 %2, vcc, %11, %19, vcc\n\t"
      KHB_NOP
      "v_addc_co_u32_e32 %3, vcc, %12, %20, vcc\n\t"
      KHB_NOP
      "v_addc_co_u32_e32 %4, vcc, %13, %21, vcc\n\t"
      KHB_NOP
      "v_addc_co_u32_e32 %5, vcc, %14, %22, vcc\n\t"
      KHB_NOP
      "v_addc_co_u32_e32 %6, vcc, %15, %23, vcc\n\t"
      KHB_NOP
      "v_addc_co_u32_e32 %7, vcc, %16, %24, vcc\n\t"
      KHB_NOP
      "v_addc_co_u32_e32 %8, vcc, 0, %25, vcc"
      : "=&v"(s[0]), "=&v"(s[1]), "=&v"(s[2]), "=&v"(s[3]), "=&v"(s[4]), "=&v"(s[5]), "=&v"(s[6]), "=&v"(s[7]),
        "=&v"(c)
      : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "v"(a[4]), "v"(a[5]), "v"(a[6]), "v"(a[7]),
        "v"(b[0]), "v"(b[1]), "v"(b[2]), "v"(b[3]), "v"(b[4]), "v"(b[5]), "v"(b[6]), "v"(b[7]),
        "v"(0u)
      : "vcc");
  return c;
}

// (t + w) mod p, lazy (< 2^256), for t a 512-bit product and any w < 2^256: the addend rides in
// one carry chain U = L + w ahead of the V mads, so a following modular add/sub (x = s^2 - u)
// costs 9 instructions instead of 19.  U + (H << 32) < 2^288 + 2^257, the bound R9:R8 < 3 * 2^32
// relies on.
FM_DEV void fm_reduce_add(Fe& r, const uint32_t t[16], const Fe& w) {
  uint32_t U[8];
  const uint32_t U8 = fm_add8(U, t, w.v);
  fm_reduce_V(r, U, U8, t + 8);
}

// Multiply / square: forward-carried columns (fm_mul512x / fm_sqr512x), then the reduction.  (The column-shuffle
// and fold-as-completed schedules were measured slower: profiles/r01_fmbench.txt.)
FM_DEV void fm_mul(Fe& r, const Fe& a, const Fe& b) {
  uint32_t t[16];
  fm_mul512x(t, a.v, b.v);
  fm_reduce(r, t);
}

FM_DEV void fm_sqr(Fe& r, const Fe& a) {
  uint32_t t[16];
  fm_sqr512x(t, a.v);
  fm_reduce(r, t);
}

// r = a^2 + w (mod p), lazy; w < 2^256 (fm_reduce_add).
FM_DEV void fm_sqr_add(Fe& r, const Fe& a, const Fe& w) {
  uint32_t t[16];
  fm_sqr512x(t, a.v);
  fm_reduce_add(r, t, w);
}

// a - b mod p for a < 2^256, b < p.
FM_DEV void fm_sub(Fe& r, const Fe& a, const Fe& b) {
  uint32_t d[8], m, k0, k1;
  uint64_t b2;           // lane mask: the correction borrowed out of limb 1 (head comment, rare carries)
  asm("v_sub_co_u32_e32 %0, vcc, %12, %20\n\t"
      KHB_NOP
      "v_subb_co_u32_e32 %1, vcc, %13, %21, vcc\n\t"
      KHB_NOP
      "v_subb_co_u32_e32 %2, vcc, %14, %22, vcc\n\t"
      KHB_NOP
      "v_subb_co_u32_e32 %3, vcc, %15, %23, vcc\n\t"
      KHB_NOP
      "v_subb_co_u32_e32 %4, vcc, %16, %24, vcc\n\t"
      KHB_NOP
      "v_subb_co_u32_e32 %5, vcc, %17, %25, vcc\n\t"
      KHB_NOP
      "v_subb_co_u32_e32 %6, vcc, %18, %26, vcc\n\t"
      KHB_NOP
      "v_subb_co_u32_e32 %7, vcc, %19, %27, vcc\n\t"
      // m = borrow ? 0xffffffff : 0 ; subtract (0x1000003D1 & m), i.e. add p on borrow
      KHB_NOP
      "v_subb_co_u32_e32 %8, vcc, 0, %28, vcc\n\t"
      "v_and_b32_e32 %9, 0x3d1, %8\n\t"
      "v_and_b32_e32 %10, 1, %8\n\t"
      "v_sub_co_u32_e32 %0, vcc, %0, %9\n\t"
      KHB_NOP
      // the borrow into limb 2 (probability ~2^-32) goes to the mask and is propagated in the rare branch
      "v_subb_co_u32_e64 %1, %11, %1, %10, vcc"
      : "=&v"(d[0]), "=&v"(d[1]), "=&v"(d[2]), "=&v"(d[3]), "=&v"(d[4]), "=&v"(d[5]), "=&v"(d[6]), "=&v"(d[7]),
        "=&v"(m), "=&v"(k0), "=&v"(k1), "=s"(b2)
      : "v"(a.v[0]), "v"(a.v[1]), "v"(a.v[2]), "v"(a.v[3]), "v"(a.v[4]), "v"(a.v[5]), "v"(a.v[6]), "v"(a.v[7]),
        "v"(b.v[0]), "v"(b.v[1]), "v"(b.v[2]), "v"(b.v[3]), "v"(b.v[4]), "v"(b.v[5]), "v"(b.v[6]), "v"(b.v[7]),
        "v"(0u)
      : "vcc");
  if (fm_any_mask(b2)) {
    uint32_t bo = fm_mask_bit(b2);
#pragma unroll
    for (int i = 2; i < 8; ++i) {
      const uint32_t t = d[i] - bo;
      bo = (bo && d[i] == 0) ? 1u : 0u;
      d[i] = t;
    }
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) r.v[i] = d[i];
}

// r = a + 0x1000003D1 (mod 2^256) with carry-out, as a chain (the "subtract p" step).
FM_DEV uint32_t fm_add_k(uint32_t t[8], const uint32_t s[8]) {
  uint32_t c;
  asm("v_add_co_u32_e32 %0, vcc, 0x3d1, %9\n\t"
      KHB_NOP
      "v_addc_co_u32_e32 %1, vcc, 1, %10, vcc\n\t"
      KHB_NOP
      "v_addc_co_u32_e32 %2, vcc, 0, %11, vcc\n\t"
      KHB_NOP
      "v_addc_co_u32_e32 %3, vcc, 0, %12, vcc\n\t"
      KHB_NOP
      "v_addc_co_u32_e32 %4, vcc, 0, %13, vcc\n\t"
      KHB_NOP
      "v_addc_co_u32_e32 %5, vcc, 0, %14, vcc\n\t"
      KHB_NOP
      "v_addc_co_u32_e32 %6, vcc, 0, %15, vcc\n\t"
      KHB_NOP
      "v_addc_co_u32_e32 %7, vcc, 0, %16, vcc\n\t"
      KHB_NOP
      "v_addc_co_u32_e32 %8, vcc, 0, %17, vcc"
      : "=&v"(t[0]), "=&v"(t[1]), "=&v"(t[2]), "=&v"(t[3]), "=&v"(t[4]), "=&v"(t[5]), "=&v"(t[6]), "=&v"(t[7]),
        "=&v"(c)
      : "v"(s[0]), "v"(s[1]), "v"(s[2]), "v"(s[3]), "v"(s[4]), "v"(s[5]), "v"(s[6]), "v"(s[7]), "v"(0u)
      : "vcc");
  return c;
}

// canonical a mod p for a < 2^256
FM_DEV void fm_canon(Fe& r, const Fe& a) {
  uint32_t t[8];
  const uint32_t c = fm_add_k(t, a.v);
  const bool sel = c != 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.v[i] = sel ? t[i] : a.v[i];
}

// a + b mod p, lazy: for a < p and b < 2^256 (so a + b < 2^257 - 0x1000003D1) the sum folds its
// carry back as 2^256 = 0x1000003D1 (mod p) and stays < 2^256.  Feeds a product only.
FM_DEV void fm_add_lazy(Fe& r, const Fe& a, const Fe& b) {
  uint32_t s[8];
  const uint32_t c = fm_add8(s, a.v, b.v);
  // fold the carry as 2^256 = 0x1000003D1: limbs 0..1 always; the carry into limb 2 (~2^-30 per call: the
  // fold into a random 256-bit value) goes to a lane mask and is propagated only behind the rare branch
  uint32_t k;
  uint64_t c2;
  asm("v_mul_u32_u24_e32 %2, 0x3d1, %4\n\t"
      "v_add_co_u32_e32 %0, vcc, %0, %2\n\t"
      KHB_NOP
      "v_addc_co_u32_e64 %1, %3, %1, %4, vcc"
      : "+v"(s[0]), "+v"(s[1]), "=&v"(k), "=s"(c2)
      : "v"(c)
      : "vcc");
  if (fm_any_mask(c2)) fm_propagate<2>(s, fm_mask_bit(c2));
#pragma unroll
  for (int i = 0; i < 8; ++i) r.v[i] = s[i];
}

// a + b mod p, a, b < p, canonical result
FM_DEV void fm_add(Fe& r, const Fe& a, const Fe& b) {
  uint32_t s[8];
  const uint32_t c = fm_add8(s, a.v, b.v);
  uint32_t t[8];
  const uint32_t ct = fm_add_k(t, s);
  const bool sel = (c | ct) != 0;    // a+b >= p  <=>  carry out of a+b or of (a+b mod 2^256)+K
#pragma unroll
  for (int i = 0; i < 8; ++i) r.v[i] = sel ? t[i] : s[i];
}

FM_DEV void fm_sqr_n(Fe& r, const Fe& a, int n) {
  r = a;
  for (int i = 0; i < n; ++i) fm_sqr(r, r);
}

// a^(p-2) (inv(0) = 0); lazy result (congruent, < 2^256).
FM_DEV void fm_inv(Fe& r, const Fe& a) {
  Fe x2, x3, x6, x9, x11, x22, x44, x88, x176, x220, x223, t;
  fm_sqr(x2, a);            fm_mul(x2, x2, a);
  fm_sqr(x3, x2);           fm_mul(x3, x3, a);
  fm_sqr_n(x6, x3, 3);      fm_mul(x6, x6, x3);
  fm_sqr_n(x9, x6, 3);      fm_mul(x9, x9, x3);
  fm_sqr_n(x11, x9, 2);     fm_mul(x11, x11, x2);
  fm_sqr_n(x22, x11, 11);   fm_mul(x22, x22, x11);
  fm_sqr_n(x44, x22, 22);   fm_mul(x44, x44, x22);
  fm_sqr_n(x88, x44, 44);   fm_mul(x88, x88, x44);
  fm_sqr_n(x176, x88, 88);  fm_mul(x176, x176, x88);
  fm_sqr_n(x220, x176, 44); fm_mul(x220, x220, x44);
  fm_sqr_n(x223, x220, 3);  fm_mul(x223, x223, x3);
  fm_sqr_n(t, x223, 23);    fm_mul(t, t, x22);
  fm_sqr_n(t, t, 5);        fm_mul(t, t, a);
  fm_sqr_n(t, t, 3);        fm_mul(t, t, x2);
  fm_sqr_n(t, t, 2);        fm_mul(r, t, a);
}

}  // namespace khb
