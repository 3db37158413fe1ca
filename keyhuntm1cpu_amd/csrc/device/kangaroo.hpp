// Pollard's kangaroo (lambda) walk with distinguished points: k_kang_walk's vocabulary and its one step.
//
// The step rule, which tests/kangaroo_ref.py and the host's kang_cpu_walk restate: a kangaroo at canonical (x, y) with
// the unsigned 256-bit distance d takes jump j = x.v[0] & 31, or (j + 1) & 31 when x == J_j.x (the point is +-J_j; the
// 32 J.x are distinct, so the second choice never collides), and becomes (x, y) + J_j, d + s_j.  The new point is a
// distinguished point iff (x.v[1] & (2^dp - 1)) == 0.  Jump index and DP test read the canonical x.
#pragma once
#include "walk.hpp"

#ifndef KHB_KANG_PER_LANE
// Kangaroo slots per lane: one field inversion (~270 products) is shared by this many jumps (6 products each).
// 64 walked 14.7 G jumps/s against 12.7 G at 32 and 9.6 G at 16, three alternating runs each (tools/bench_kangaroo.py
// --ab; DESIGN.md §2g, profiles/kangaroo).
#define KHB_KANG_PER_LANE 64
#endif
#ifndef KHB_KANG_WAVES_PER_SIMD
#define KHB_KANG_WAVES_PER_SIMD 4   // occupancy target of k_kang_walk (128 VGPRs; DESIGN.md §2g has its resource usage)
#endif

namespace khbk {

constexpr uint32_t kKangPerLane = KHB_KANG_PER_LANE;
constexpr uint32_t kKangJumps = 32;
constexpr uint32_t kKangJumpWords = 24;              // x, y, distance: 8 words each
constexpr uint32_t kKangRingDefault = 1u << 18;

// A reported distinguished point, as the kernel writes it to the ring.
struct KangDpDev {
  uint32_t i;
  uint32_t x[8];
  uint32_t d[8];
};

struct KangArgs {
  Fe* __restrict__ x;                    // state [slot][lane], `stride` lanes per slot: kangaroo i is slot
  Fe* __restrict__ y;                    // i % kKangPerLane of lane i / kKangPerLane
  Fe* __restrict__ d;                    // distances, 8 little-endian words
  Fe* __restrict__ scr;                  // prefix products [slot][lane]
  const uint32_t* __restrict__ jumps;    // [kKangJumpWords][32]: word k of jump j at 32 k + j
  KangDpDev* __restrict__ ring;
  uint32_t ring_cap;
  unsigned long long* __restrict__ cnt;  // [0] distinguished points [1] jumps made [2] second choices
  uint32_t n;                            // kangaroos
  uint32_t stride;
  uint32_t steps;
  uint32_t dp_mask;                      // 2^dp - 1
};

// The jump table in LDS, word-major: lanes of a wave that pick different jumps read different banks, lanes that pick
// the same one share a broadcast.
typedef uint32_t KangJumpLds[kKangJumpWords][kKangJumps];

__device__ __forceinline__ Fe kang_jump_fe(const KangJumpLds& jt, uint32_t j, uint32_t at) {
  Fe r;
#pragma unroll
  for (int k = 0; k < 8; ++k) r.v[k] = jt[at + k][j];
  return r;
}

// The jump of a kangaroo at canonical x and that jump's x; second = the x == J_j.x rule fired.
__device__ __forceinline__ uint32_t kang_pick(const KangJumpLds& jt, const Fe& x, Fe& jx, bool& second) {
  uint32_t j = x.v[0] & (kKangJumps - 1);
  jx = kang_jump_fe(jt, j, 0);
  second = fe_eq(jx, x);
  if (second) {
    j = (j + 1) & (kKangJumps - 1);
    jx = kang_jump_fe(jt, j, 0);
  }
  return j;
}

// One step of the lane's m kangaroos (slots 0 .. m - 1; an empty slot is not stepped and leaves the batch product
// alone): the forward pass stores the prefix products of dx = J_j.x - x, one inversion, and the backward pass peels
// each kangaroo's inverse, adds J_j, adds s_j to the distance, stores the state and reports a distinguished point.
__device__ __forceinline__ void kang_step(const KangArgs& A, const KangJumpLds& jt, uint32_t lane, uint32_t m,
                                          uint32_t& seconds) {
  const size_t S = A.stride;
  Fe* const X = A.x + lane;
  Fe* const Y = A.y + lane;
  Fe* const D = A.d + lane;
  Fe* const scr = A.scr + lane;
  Fe acc;
  for (uint32_t s = 0; s < m; ++s) {
    const Fe x = X[s * S];
    Fe jx, dx;
    bool second;
    kang_pick(jt, x, jx, second);
    seconds += second ? 1u : 0u;
    fm_sub(dx, jx, x);
    if (s == 0) acc = dx; else fm_mul(acc, acc, dx);
    scr_st(scr + s * S, acc);
  }
  Fe inv;
  fm_inv(inv, acc);
  for (uint32_t s = m; s-- > 0;) {
    AffPt P{X[s * S], Y[s * S]};
    Fe dist = D[s * S];
    AffPt J;
    bool second;
    const uint32_t j = kang_pick(jt, P.x, J.x, second);
    J.y = kang_jump_fe(jt, j, 8);
    Fe is;
    if (s > 0) {
      Fe dx;
      fm_sub(dx, J.x, P.x);
      fm_mul(is, inv, scr_ld(scr + (s - 1) * S));
      fm_mul(inv, inv, dx);
    } else {
      is = inv;
    }
    aff_add(P, P, J, is);
    const Fe sj = kang_jump_fe(jt, j, 16);
    // a plain add through all eight words: a carry out of the top is dropped, so the distance is kept mod 2^256, as
    // the model's and the host's is (the accepted widths never get there; test_gpu_kangaroo_directed.py pins the wrap)
    fm_add8(dist.v, dist.v, sj.v);
    X[s * S] = P.x;
    Y[s * S] = P.y;
    D[s * S] = dist;
    if ((P.x.v[1] & A.dp_mask) == 0) {
      const unsigned long long slot = atomicAdd(&A.cnt[0], 1ull);
      if (slot < A.ring_cap) {
        KangDpDev r;
        r.i = lane * kKangPerLane + s;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          r.x[k] = P.x.v[k];
          r.d[k] = dist.v[k];
        }
        A.ring[slot] = r;
      }
    }
  }
}

}  // namespace khbk
