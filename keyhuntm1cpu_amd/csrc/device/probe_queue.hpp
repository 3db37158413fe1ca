// The level-1 probe of the -m bsgs scan: the survivor queue, the gate's tests, probe / probe_pair / gate_pair.
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

// kScanG: gate test of one walk step's two x (x2 absent at step 511: has2 = false, uniform).  Both
// blocks are loaded before either is waited for; survivors (~0.04 % of x) go to the queue.
// STAGES (gate_stages): 1 tests the stage-1 fold first, 2 tests the stage-0 filter before the fold.  Each stage
// is a superset of the next, so the queued x are exactly the full gate's survivors in every case.
template <int STAGES>
__device__ __forceinline__ void gate_pair(const ScanArgs& A, ProbeQueue& Q, const Fe& x1, uint32_t step1, bool has2,
                                          const Fe& x2, uint32_t step2, uint32_t job) {
  bool h1, h2;
  const uint32_t s2 = gate_s2(A);
  const GateBits b1 = gate_bits(x1.v[1], s2), b2 = gate_bits(x2.v[1], s2);
  if constexpr (STAGES >= 1) {
    bool s1 = true, s2p = has2;
    if constexpr (STAGES == 2) {
      // stage 0 (L2-resident, one bit per member: ~63 % of x pass at k = 4); the fold's line (read from the MALL at
      // k = 4) is fetched only for its survivors.  No ballot: with ~63 % passing a wave almost never skips.
      const uint32_t v1 = A.gate0[x1.v[0] & A.gate0_mask], v2 = A.gate0[x2.v[0] & A.gate0_mask];
      s1 = (int32_t)shl_mod32(v1, b1.a1) < 0;
      s2p = has2 && (int32_t)shl_mod32(v2, b2.a1) < 0;
    }
    // stage 1 (the fold: L2-resident at k = 1); the full gate's line is fetched only for its survivors
    uint2 f1, f2;                                  // read only where loaded (s1 / s2p)
    if (STAGES == 1 || s1) f1 = gate_block(A.gate1, A.gate1_mask, x1);
    if (STAGES == 1 || s2p) f2 = gate_block(A.gate1, A.gate1_mask, x2);
    s1 = s1 && gate_block_pass(f1, b1);
    s2p = s2p && gate_block_pass(f2, b2);
    if (__ballot(s1 || s2p) == 0) return;
    uint2 w1, w2;                                  // read only where loaded (s1 / s2p)
    if (s1) w1 = gate_block(A.gate, A.gate_mask, x1);
    if (s2p) w2 = gate_block(A.gate, A.gate_mask, x2);
    h1 = s1 && gate_block_pass(w1, b1);
    h2 = s2p && gate_block_pass(w2, b2);
  } else {
    const uint2 w1 = gate_block(A.gate, A.gate_mask, x1), w2 = gate_block(A.gate, A.gate_mask, x2);
    h1 = gate_block_pass(w1, b1);
    h2 = has2 && gate_block_pass(w2, b2);
  }
  if (__ballot(h1 || h2) == 0) return;
  q_push(Q, h1, x1, job, step1);
  q_drain(A, Q, kDrainAt);
  q_push(Q, h2, x2, job, step2);
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
