// -m xpoint (keyhunt.cpp:3005-3062): the first 20 bytes of the big-endian x of a public key are probed in the target
// bloom as they are, no hash in between (Get32Bytes, then bloom_check(&bloom, rawvalue, 20)).  Host and device share
// this code (KHB_HD) so tests/native checks it on the CPU.
//
// Byte conventions: Fe limbs are little-endian words (v[7] most significant), so Get32Bytes(x) is the word stream
// x.v[7] ... x.v[0] big-endian and its first 20 bytes are x.v[7] ... x.v[3].  They are returned as five words whose
// little-endian bytes are those bytes, the convention of hash160.hpp's outputs and of bloom_check20: one byte swap
// per word.  The low 96 bits of x (v[0..2]) are not read.
#pragma once
#include <stdint.h>
#include "fe.hpp"
#include "bloom_probe.hpp"

namespace khb {

// x canonical (the reference serialises the reduced coordinate).
KHB_HD void x_be20(uint32_t h[5], const Fe& x) {
#pragma unroll
  for (int k = 0; k < 5; ++k) h[k] = bswap32(x.v[7 - k]);
}

}  // namespace khb
