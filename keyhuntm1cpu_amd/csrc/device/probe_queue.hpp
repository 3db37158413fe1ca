// The level-1 probe of the -m bsgs scan: the survivor queue, the gate's tests, probe / probe_pair / the gate's phases.
#pragma once
#include "scan_args.hpp"

namespace khbk {

// ---- level-1 probe with a per-wave survivor queue ---------------------------------------------
// Without a gate every x pays the first XXH64 and one bit load: L1 bit 0; the ~50 % whose bit is
// set are pushed to a per-wave LDS queue (x, a, job, giant-step index); whenever 64 are queued the
// whole wave finishes 64 of them together (second XXH64 + remaining bits, bloom_rest).  Without
// the queue a wave would run the second hash and the dependent bit loads whenever ANY of its lanes
// survived, i.e. for every x, with one memory round trip per bit per probe site.
//
// With a level-0 gate (khb_load_gate) x pays no hash at all: one byte of a 2^L-bit map (L = 28 at
// k = 1, 32 MiB) addressed by the low L bits of x, with the bit of every baby-step x of the L1 set
// set, so no L1 member is ever dropped.  Only the gate's survivors (~1.5 %) are queued, and the
// drain runs the whole L1 check (XXH64 a, bloom_full).  The candidate stream is the L1 candidates
// whose gate bit is set: every true member, and ~1.5 % of the false positives that
// bsgs_secondcheck would reject.
constexpr uint32_t kDrainAt = 64;          // drain threshold (entries): one per lane
constexpr uint32_t kQCap = kDrainAt + 64;           // entries per wave: < kDrainAt resident + <= 64 pushed
constexpr uint32_t kQWords = 10;           // x[8], job, step index (SoA in LDS)
constexpr uint32_t kWavesPerBlock = kBlock / 64;

// The count lives in LDS, not in a register: lanes of a wave may diverge (the ragged last lane of
// a job, the tail of the item loop), and a register copy would go stale in the inactive lanes.
struct ProbeQueue {
  uint32_t* q;            // this wave's LDS region: kQWords arrays of kQCap words
  // this wave's queued-entry count, typed as an LDS pointer: through a generic (flat) pointer
  // every count access was a flat_load/flat_store, which counts against vmcnt AND lgkmcnt and
  // made each one wait for all outstanding vector-memory operations (the prefetched prefix).
  volatile __attribute__((address_space(3))) uint32_t* n;
};

__device__ __forceinline__ uint32_t lane_rank(uint64_t mask) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// Read queued entry k (x, job, step).
__device__ __forceinline__ void q_read(const ProbeQueue& Q, uint32_t k, Fe& x, uint32_t& job, uint32_t& step) {
#pragma unroll
  for (int d = 0; d < 8; ++d) x.v[d] = Q.q[d * kQCap + k];
  job = Q.q[8 * kQCap + k];
  step = Q.q[9 * kQCap + k];
}

// Finish the newest min(n, active lanes) queued entries, one per lane, while n >= threshold.
__device__ __forceinline__ void q_drain(const ScanArgs& A, ProbeQueue& Q, uint32_t threshold) {
  for (;;) {
    const uint32_t n = *Q.n;
    if (n < threshold || n == 0) break;
    const uint64_t em = __ballot(1);
    const uint32_t take = min(n, (uint32_t)__popcll(em));
    const uint32_t r = lane_rank(em);
    *Q.n = n - take;
    asm volatile("" ::: "memory");
    if (r < take) {
      Fe x;
      uint32_t job, step;
      q_read(Q, n - take + r, x, job, step);
      fm_canon(x, x);                   // gated pushes hold lazy x (x_out)
      uint64_t w[4];
      x_words(w, x);
      // the whole level-1 check (bit 0 again for ungated pushes: the first hash is not queued)
      if (bloom_full<1>(sub_bloom(A.bloom, A.geom, x), A.geom, w, xxh64_32(w, KHB_BLOOM_SEED)))
        emit_cand(A, job, step);
    }
    asm volatile("" ::: "memory");
  }
}

// Queue x if its first bit (L1 bit 0, or the gate bit) is set.
__device__ __forceinline__ void q_push(ProbeQueue& Q, bool hit, const Fe& x, uint32_t job, uint32_t step) {
  const uint64_t m = __ballot(hit);
  const uint32_t n = *Q.n;
  if (hit) {
    const uint32_t k = n + lane_rank(m);
#pragma unroll
    for (int d = 0; d < 8; ++d) Q.q[d * kQCap + k] = x.v[d];
    Q.q[8 * kQCap + k] = job;
    Q.q[9 * kQCap + k] = step;
  }
  asm volatile("" ::: "memory");
  *Q.n = n + (uint32_t)__popcll(m);
}

// The gate's bits in x's 64-bit block (lo, hi words): probe p tests bit b_p = (w1 >> 5p) mod 32 of word
// p mod 2 (p = 0: lo, 1: hi, 2: lo), w1 = x.v[1].  Each probe is one left shift by 31 - b_p = (~w1 >> 5p)
// mod 32 that brings its bit to bit 31 (the hardware takes a 32-bit shift's amount mod 32, so the amounts
// need no mask and no word select); the block passes when the AND of the three shifted words is negative.
// The amounts are computed once per x and shared by the stage-1 fold's test and the full gate's.  Fewer
// probes than 3 need no per-lane masks: probe 2 repeats probe 0 (shift distance 0 instead of 10,
// wave-uniform), and for one probe khb_load_gate sets every block's hi word, so probe 1 always passes.
struct GateBits {
  uint32_t a0, a1, a2;   // left-shift amounts (mod 32) of probes 0, 1, 2
};
__device__ __forceinline__ uint32_t gate_s2(const ScanArgs& A) { return A.gate_probes >= 3 ? 10u : 0u; }
__device__ __forceinline__ GateBits gate_bits(uint32_t w1, uint32_t s2) {
  const uint32_t n = ~w1;
  return GateBits{n, n >> 5, n >> s2};
}
// v_lshlrev_b32 as the hardware reads it (amount mod 32); opaque to the compiler, which otherwise masks
// an amount computed in another basic block with a v_and_b32 (round-4 ISA of the fold's second test)
__device__ __forceinline__ uint32_t shl_mod32(uint32_t x, uint32_t s) {
  uint32_t r;
  asm("v_lshlrev_b32 %0, %1, %2" : "=v"(r) : "v"(s), "v"(x));
  return r;
}
__device__ __forceinline__ bool gate_block_pass(uint2 w, GateBits b) {
  return (int32_t)(shl_mod32(w.x, b.a0) & shl_mod32(w.y, b.a1) & shl_mod32(w.x, b.a2)) < 0;
}
__device__ __forceinline__ uint2 gate_block(const uint8_t* g, uint32_t mask, const Fe& x) {
  return reinterpret_cast<const uint2*>(g)[x.v[0] & mask];
}

// kScanG: gate test of one walk step's two x (x2 absent at step 511: has2 = false, uniform), in phases, so that the
// walk runs the next step's field products between a load and its first use instead of waiting out two dependent
// round trips (the fold from L2, the gate from the Infinity Cache) with nothing to issue:
//   gate_issue_first   x1's first load, as soon as x1 is finished (x2's product and squaring run behind it);
//   gate_issue_second  x2's first load;
//   gate_advance       test the fold, load the full gate's block for the fold's survivors (STAGES >= 1);
//   gate_finish        test the gate; survivors (~0.04 % of x) go to the queue.
// STAGES (gate_stages): 0 loads the gate's block first and gate_advance is empty; 1 tests the stage-1 fold first; 2 tests
// the stage-0 filter before the fold (x1's filter word is loaded by gate_issue_first, and gate_issue_second tests both
// words and loads the fold's blocks: the filter's trip hides behind x2's arithmetic).  Each stage is a superset of the
// next, so the queued x are exactly the full gate's survivors in every case.
// The state between the phases is local to one walk; lanes walk a group in lock-step, so its lane masks live under one
// exec mask, and nothing is pending when the walk returns.  A block is loaded only in the lanes still in the running
// (exec-masked) and tested in all of them, the lane mask ANDed in: the common path has no branch, and no wave-wide
// early-out either (at k = 1 some lane of a wave's 128 x passes the fold in all but ~1e-9 of the steps).
struct GatePending {
  Fe x1, x2;               // lazy x (x_out), as the queue holds them
  uint32_t t1, t2;         // their indices in the group (wave-uniform)
  uint2 b1, b2;            // the block last loaded for each x (stale where m1 / m2 is off)
  uint64_t m1, m2;         // lane masks: the lanes whose x has passed every stage tested so far
};
// What crosses a phase lives in as few VGPRs as it can: the lane masks in SGPR pairs (opaque, or the compiler keeps the
// fold's shifted words in VGPRs to AND them into the gate's), and the shift amounts are recomputed from x's word 1 in
// every phase (from an opaque v_not_b32, or they are kept: 3 VGPRs per x).  With either in VGPRs the pair loop spilled.
__device__ __forceinline__ uint64_t lane_mask(bool b) {
  uint64_t m = __builtin_amdgcn_ballot_w64(b);
  asm volatile("" : "+s"(m));
  return m;
}
__device__ __forceinline__ bool in_mask(uint64_t m) { return __builtin_amdgcn_inverse_ballot_w64(m); }
__device__ __forceinline__ GateBits gate_bits_again(uint32_t w1, uint32_t s2) {
  uint32_t n;
  asm volatile("v_not_b32 %0, %1" : "=v"(n) : "v"(w1));
  return GateBits{n, n >> 5, n >> s2};
}
// Nothing crosses a phase boundary in the scheduler: the field products are non-volatile asm, and without this
// the loads' first uses (and with them the waits) move up in front of the products meant to cover them.
__device__ __forceinline__ void gate_fence() { __builtin_amdgcn_sched_barrier(0); }

template <int STAGES>
__device__ __forceinline__ void gate_issue_first(const ScanArgs& A, GatePending& G, const Fe& x1, uint32_t t1) {
  G.x1 = x1;
  G.t1 = t1;
  G.m1 = lane_mask(true);
  if constexpr (STAGES == 2)
    G.b1 = uint2{A.gate0[x1.v[0] & A.gate0_mask], 0};   // stage 0 (L2-resident, one bit per member: ~63 % of x pass at k = 4)
  else
    G.b1 = gate_block(STAGES == 1 ? A.gate1 : A.gate, STAGES == 1 ? A.gate1_mask : A.gate_mask, x1);
  gate_fence();
}
template <int STAGES>
__device__ __forceinline__ void gate_issue_second(const ScanArgs& A, GatePending& G, bool has2, const Fe& x2,
                                                  uint32_t t2) {
  G.x2 = x2;
  G.t2 = t2;
  G.m2 = lane_mask(has2);
  if (!has2) G.b2 = uint2{0, 0};
  if constexpr (STAGES == 2) {
    // the fold's line (read from the MALL at k = 4) is fetched only for stage 0's survivors
    uint32_t v2 = 0;
    if (has2) v2 = A.gate0[x2.v[0] & A.gate0_mask];
    gate_fence();
    G.m1 = lane_mask((int32_t)shl_mod32(G.b1.x, gate_bits_again(G.x1.v[1], 0).a1) < 0);
    G.m2 = lane_mask(has2 & ((int32_t)shl_mod32(v2, gate_bits_again(x2.v[1], 0).a1) < 0));
    if (in_mask(G.m1)) G.b1 = gate_block(A.gate1, A.gate1_mask, G.x1);
    if (in_mask(G.m2)) G.b2 = gate_block(A.gate1, A.gate1_mask, x2);
  } else {
    if (has2) G.b2 = gate_block(STAGES == 1 ? A.gate1 : A.gate, STAGES == 1 ? A.gate1_mask : A.gate_mask, x2);
  }
  gate_fence();
}
// stage 1 (the fold: L2-resident at k = 1); the full gate's line is fetched only for its survivors
template <int STAGES>
__device__ __forceinline__ void gate_advance(const ScanArgs& A, GatePending& G) {
  if constexpr (STAGES >= 1) {
    gate_fence();
    const uint32_t s2 = gate_s2(A);
    G.m1 &= lane_mask(gate_block_pass(G.b1, gate_bits_again(G.x1.v[1], s2)));
    G.m2 &= lane_mask(gate_block_pass(G.b2, gate_bits_again(G.x2.v[1], s2)));
    if (in_mask(G.m1)) G.b1 = gate_block(A.gate, A.gate_mask, G.x1);
    if (in_mask(G.m2)) G.b2 = gate_block(A.gate, A.gate_mask, G.x2);
    gate_fence();
  }
}
template <int STAGES>
__device__ __forceinline__ void gate_finish(const ScanArgs& A, ProbeQueue& Q, GatePending& G, uint32_t job,
                                            uint32_t base) {
  gate_fence();
  const uint32_t s2 = gate_s2(A);
  const uint64_t h1 = G.m1 & lane_mask(gate_block_pass(G.b1, gate_bits_again(G.x1.v[1], s2)));
  const uint64_t h2 = G.m2 & lane_mask(gate_block_pass(G.b2, gate_bits_again(G.x2.v[1], s2)));
  G.m1 = G.m2 = 0;
  if ((h1 | h2) == 0) return;
  q_push(Q, in_mask(h1), G.x1, job, base + G.t1);
  q_drain(A, Q, kDrainAt);
  q_push(Q, in_mask(h2), G.x2, job, base + G.t2);
  q_drain(A, Q, kDrainAt);
}

// Gate bits of x (blocked gate), or without a gate L1 bit 0 (a = the first XXH64).
__device__ __forceinline__ bool first_bit(const ScanArgs& A, const Fe& x, uint64_t& a) {
  if (A.gate) {
    a = 0;
    return gate_block_pass(gate_block(A.gate, A.gate_mask, x), gate_bits(x.v[1], gate_s2(A)));
  }
  uint64_t w[4];
  x_words(w, x);
  a = xxh64_32(w, KHB_BLOOM_SEED);
  return test_bit(sub_bloom(A.bloom, A.geom, x), mod_bits(a, A.geom));
}

template <bool DUMP>
__device__ __forceinline__ void probe(const ScanArgs& A, ProbeQueue& Q, const Fe& x, uint32_t job, uint32_t j,
                                      uint32_t t) {
  if (DUMP) {
    uint8_t* o = A.xdump + ((uint64_t)(j - A.group_begin) * KHB_GROUP + t) * 32;
    fe_to_be(o, x);
  } else {
    uint64_t a;
    const bool hit = first_bit(A, x, a);
    q_push(Q, hit, x, job, j * KHB_GROUP + t);
    q_drain(A, Q, kDrainAt);
  }
}

// The two points of one backward step (C - GSn[i], C + GSn[i]): both first hashes are computed
// before either bloom bit is awaited, so the two loads share one memory round trip.
template <bool DUMP>
__device__ __forceinline__ void probe_pair(const ScanArgs& A, ProbeQueue& Q, const Fe& x1, const Fe& x2,
                                           uint32_t job, uint32_t j, uint32_t t1, uint32_t t2) {
  if (!DUMP) {
    uint64_t a1, a2;
    const bool h1 = first_bit(A, x1, a1);
    const bool h2 = first_bit(A, x2, a2);
    q_push(Q, h1, x1, job, j * KHB_GROUP + t1);
    q_drain(A, Q, kDrainAt);
    q_push(Q, h2, x2, job, j * KHB_GROUP + t2);
    q_drain(A, Q, kDrainAt);
    return;
  }
  probe<DUMP>(A, Q, x1, job, j, t1);
  probe<DUMP>(A, Q, x2, job, j, t2);
}

}  // namespace khbk
