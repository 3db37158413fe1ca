// Baby-step table build (kBaby): what the x,y walk does with each x (bloom_add into L1/L2/L3, the gate, bPtable).
#pragma once
#include "scan_args.hpp"

namespace khbk {

// bloom_add (bloom.cpp:61-85, 159-162) of a 32-byte x into the sub-bloom of a level that starts at bit `base`
// (ScanArgs::bstride) of `words`.
__device__ __forceinline__ void bloom_add_words(uint32_t* __restrict__ words, uint64_t base, const BloomGeom& g,
                                                uint64_t a, uint64_t b) {
  uint64_t pos = mod_bits(a, g);
  const uint64_t bm = mod_bits(b, g);
  uint64_t h = a;
  for (uint32_t i = 0; i < g.hashes; ++i) {
    if (i) {
      const uint64_t nh = h + b;
      const bool wrapped = nh < h;
      h = nh;
      pos += bm;
      if (pos >= g.bits) pos -= g.bits;
      if (wrapped) pos = (pos >= g.wrap) ? pos - g.wrap : pos + g.bits - g.wrap;
    }
    // bf[pos >> 3] |= 1 << (pos & 7): little-endian words, so bit (bit & 31) of the aligned word bit >> 5
    const uint64_t bit = base + pos;
    atomicOr(words + (bit >> 5), 1u << (bit & 31));
  }
}

// Baby step ic = job * job_keys + 1024 j + t (key ic + 1): thread_bPload (keyhunt.cpp:4404-4592).
__device__ __forceinline__ void baby_point(const ScanArgs& A, const Fe& x, uint32_t job, uint32_t j, uint32_t t) {
  const uint64_t ic = (uint64_t)job * A.job_keys + (uint64_t)j * KHB_GROUP + t;
  if (ic >= A.blimit[0] && ic >= A.blimit[1] && ic >= A.blimit[2] && ic >= A.glimit) return;
  uint64_t w[4];
  x_words(w, x);
  const uint64_t a = xxh64_32(w, KHB_BLOOM_SEED);
  if (A.gate_w && ic < A.glimit) {
    // the word index in 64 bits: a 2^38-bit gate has 2^32 blocks, 2^33 words
    const uint64_t w0 = 2 * (uint64_t)(x.v[0] & A.gate_mask);
    for (uint32_t p = 0; p < A.gate_probes; ++p)      // gate_block_pass: bit (w1 >> 5p) mod 32 of word p mod 2
      atomicOr(A.gate_w + (w0 + (p & 1u)), 1u << ((x.v[1] >> (5 * p)) & 31u));
  }
  const uint64_t b = xxh64_32(w, a);
  const uint32_t sub = x.v[7] >> 24;
#pragma unroll 1
  for (int l = 0; l < 3; ++l)
    if (A.bw[l] && ic < A.blimit[l]) bloom_add_words(A.bw[l], sub * A.bstride[l], A.bgeom[l], a, b);
  if (A.bp && ic < A.blimit[2]) {
    // struct bsgs_xvalue {value = x bytes 16..21 (Get32Bytes order), pad[2] = 0, index = ic}
    uint32_t* o = A.bp + 4 * ic;
    o[0] = __builtin_bswap32(x.v[3]);
    o[1] = (x.v[2] >> 24) | (((x.v[2] >> 16) & 0xffu) << 8);
    o[2] = (uint32_t)ic;
    o[3] = (uint32_t)(ic >> 32);
  }
}

}  // namespace khbk
