// k_giant_scan's vocabulary: the modes (scan_modes.hpp), constants, AffPt, ScanArgs, the result-ring writers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../../include/khbsgs.h"
#include "scan_modes.hpp"
#include "fe.hpp"
#include "fe_asm.hpp"
#include "bloom_probe.hpp"

using namespace khb;

namespace khbk {

struct AffPt {
  Fe x, y;
};

#ifndef KHB_GATE1
#define KHB_GATE1 1               // default stage-1 fold of the level-0 gate: KHB_GATE_STAGE1_AUTO (khbsgs.h)
#endif
#ifndef KHB_GATE0
// default stage-0 filter in front of the fold (khb_set_gate_stage0): none.  The 2 MiB filter at k = 4 (KHB_GATE_STAGE0_AUTO)
// ran 4.6 % SLOWER on config C (48,629 vs 50,948 Mkeys/s, 3 + 3 alternating runs, profiles/r06a/gate0): it cuts the
// fold's MALL reads to 63 % but adds one L2 lane-load per x, and a gate lane-load costs its memory-pipeline cycles
// wherever it is served.
#define KHB_GATE0 0
#endif
#ifndef KHB_WAVES_PER_SIMD
// occupancy target of k_giant_scan (launch bounds).  Round 4: 4 waves/SIMD (128 VGPRs, 262,144 lanes; the walk's
// hot path has the same 1,171 VALU per step as at 3 waves) ran 3.0 % faster than 3 (168 VGPRs) with two
// launches in flight, at 3,072 and at 4,096 chunks per launch, and 5 waves (96 VGPRs, spilling) 16 % slower
// (profiles/r04q/waves_pipe_ab.txt).  Round 3, before the L2 gate fold and the non-temporal prefix stream,
// had measured 3 waves 1.4-1.6 % faster than 4 (profiles/r03_calibration/occupancy_ab*.txt).
#define KHB_WAVES_PER_SIMD 4
#endif
constexpr uint32_t kBlock = 256;
#ifndef KHB_BATCH
#define KHB_BATCH 8               // -m bsgs groups per work item (scan_batch): two inversions per item
#endif
constexpr uint32_t kBatch = KHB_BATCH;
#ifndef KHB_HALF_STREAM
// 1 (the product since round 6): the half prefix stream (walk_group_g_half): the gated scan's forward pass stores only
// the odd prefixes and the walk rebuilds each even one from its odd neighbour, one extra product per two walk steps
// for half the HBM stream.  Exact (the same products of the same operands in the same order).  Whole-bench +1.1 % on
// one box (round 5, profiles/r05e) and +1.2 % on another (55,423 vs 54,777 Mkeys/s, 3 + 3 alternating runs,
// profiles/r06a/half); the board runs at its power cap and the halved stream lowers the energy per cycle (launch
// clock 2,310 vs 2,184 MHz).  DESIGN.md §5.
#define KHB_HALF_STREAM 1
#endif
constexpr bool kHalfStream = KHB_HALF_STREAM != 0;

#ifndef KHB_ADDR_WAVES_PER_SIMD
#define KHB_ADDR_WAVES_PER_SIMD KHB_WAVES_PER_SIMD   // occupancy target of the -m address hash kernels
#endif
#ifndef KHB_ADDR_E_WAVES_PER_SIMD
#define KHB_ADDR_E_WAVES_PER_SIMD KHB_ADDR_WAVES_PER_SIMD   // occupancy target of the -e address kernels
#endif
#ifndef KHB_ADDR_ETH_WAVES_PER_SIMD
// occupancy target of the -c eth kernel: 3 waves (168 VGPRs, no scratch) with the rolled Keccak measured 2.4 % less
// kernel time than 4 (128 VGPRs, 208 B of scratch) and 27 % less than 2 (profiles/eth)
#define KHB_ADDR_ETH_WAVES_PER_SIMD 3
#endif
#ifndef KHB_ADDR_X_WAVES_PER_SIMD
// occupancy target of the -m xpoint kernels: 3 waves (164 and 163 VGPRs, no scratch); at 4 (128 VGPRs) both kernels
// spill, 184 and 192 B of scratch per lane (profiles/xpoint)
#define KHB_ADDR_X_WAVES_PER_SIMD 3
#endif
#ifndef KHB_VANITY_WAVES_PER_SIMD
// occupancy target of the -m vanity kernels: the address kernels'.  At 4 waves (128 VGPRs) every vanity instance
// uses scratch as its address twin does, within 24 B per lane of it (228 to 412 B against 236 to 432 B)
#define KHB_VANITY_WAVES_PER_SIMD KHB_ADDR_WAVES_PER_SIMD
#endif
// the occupancy target of each mode's Occupancy (scan_modes.hpp), in that enum's order
constexpr int kOccWaves[kOccCount] = {KHB_WAVES_PER_SIMD,          KHB_ADDR_WAVES_PER_SIMD,   KHB_ADDR_E_WAVES_PER_SIMD,
                                      KHB_ADDR_ETH_WAVES_PER_SIMD, KHB_ADDR_X_WAVES_PER_SIMD, KHB_VANITY_WAVES_PER_SIMD};
constexpr int waves_per_simd(int m) { return kOccWaves[traits(m).occ]; }
constexpr uint32_t kHalf = KHB_GROUP / 2;            // 512
constexpr uint32_t kCandCap = 1u << 20;
constexpr uint32_t kAddrHitCap = 1u << 18;
constexpr uint32_t kDegenCap = 4096;
constexpr size_t kCounterBytes = 64;                 // ScanArgs::counters
constexpr size_t kHostCounterBytes = 128;            // ScanArgs::host_counters (launch_epilogue)

struct ScanArgs {
  const uint8_t* __restrict__ bloom;
  BloomGeom geom;
  const AffPt* __restrict__ gsn;       // [0..511] GSn, [512] _2GSn
  const AffPt* __restrict__ offs;      // lane start offsets
  const AffPt* __restrict__ gofs;      // per-group centre offsets j*_2GSn (scan_batch)
  const AffPt* __restrict__ centres;   // per-job group-0 centre (khb_submit: pinned host memory, read in place)
  Fe* __restrict__ scratch;            // prefix products [512][lanes]
  khb_cand* __restrict__ cand;         // candidate ring (khb_submit: pinned host memory, written in place)
  khb_degenerate* __restrict__ degen;  // degenerate-group ring (same)
  uint32_t* __restrict__ counters;     // [0] candidates [1] degenerate groups [2] work-item cursor (dynamic items)
                                       // [3] waves finished (launch_epilogue)
                                       // [4..5] groups walked (u64, count_walked)
                                       // [8..15] shader clock probe (clock_probe): memtime, realtime at the
                                       // first wave's start, then at its end (u64 each)
  uint32_t* __restrict__ host_counters;  // launch_epilogue: the last wave copies counters[0..15] here (pinned host
                                         // memory), adds its end clocks at [16..19] and zeroes counters[0..7] for
                                         // the slot's next launch; null = off
  uint32_t total_waves;                // waves of the launch (launch_epilogue)
  uint8_t* __restrict__ xdump;         // dump modes only
  uint32_t* __restrict__ ahits;        // -m address hits: {job, group, t, kind} x ahit_cap
  uint32_t ahit_cap;
  // kBaby: blooms written as 32-bit words (null = level skipped).  Bit pos of sub-bloom sub is bit
  // sub * bstride[l] + pos of the level: bstride = 32 x words per sub-bloom for khb_build_baby's word-aligned
  // sub-blooms, 8 x bytes_per_sub for the packed layout the probe reads (khb_build_l1_resident), where a word
  // may straddle two sub-blooms
  uint32_t* __restrict__ bw[3];
  BloomGeom bgeom[3];
  uint64_t bstride[3];
  uint64_t blimit[3];                  // ic < blimit[l] goes into level l (l1ext, m2, m3)
  uint32_t* __restrict__ bp;           // m3 x 16-byte struct bsgs_xvalue records (null = skipped)
  // level-0 gate (khb_load_gate): a blocked bloom of (gate_mask + 1) 64-bit blocks; x selects
  // block x.v[0] & gate_mask and in it bit (x.v[1] >> 5p) & 31 of word p & 1, p < gate_probes, all
  // set for every x of the L1 set; null = no gate.  kBaby writes it (gate_w, ic < glimit).
  const uint8_t* __restrict__ gate;
  uint32_t* __restrict__ gate_w;
  uint32_t gate_probes;
  uint64_t glimit;
  uint32_t gate_mask;                  // blocks - 1
  // stage-1 gate (khb_set_gate_stage1): the level-0 gate OR-folded to (gate1_mask + 1) blocks, block i of
  // the fold = OR of blocks j of the gate with j & gate1_mask == i; null = no stage 1
  const uint8_t* __restrict__ gate1;
  uint32_t gate1_mask;
  // stage-0 filter (khb_set_gate_stage0): one bit per baby-step x, the gate's hi words (probe 1) OR-folded to
  // (gate0_mask + 1) 32-bit words, word i = OR of the hi words of the gate's blocks j with j & gate0_mask == i;
  // null = no stage 0
  const uint32_t* __restrict__ gate0;
  uint32_t gate0_mask;
  uint64_t job_keys;                   // baby steps per job
  uint64_t n_items;
  uint32_t n_jobs, group_begin, group_end, gpl, lanes_per_job, stride, cand_cap, degen_cap;
  // -m vanity (khb_load_vanity; device/vanity.hpp): van_n sorted disjoint intervals, five words per bound with word 0
  // the most significant, and the 2^16-bit bucket bitmap every block copies into LDS at kernel entry
  const uint32_t* __restrict__ van_lo;
  const uint32_t* __restrict__ van_hi;
  const uint32_t* __restrict__ van_bitmap;
  uint32_t van_n;
};

__device__ __forceinline__ void emit_cand(const ScanArgs& A, uint32_t job, uint32_t a) {
  uint32_t k = atomicAdd(&A.counters[0], 1u);
  if (k < A.cand_cap) A.cand[k] = khb_cand{job, a};
}

__device__ __forceinline__ void emit_ahit(const ScanArgs& A, uint32_t job, uint32_t j, uint32_t t, uint32_t kind) {
  const uint32_t k = atomicAdd(&A.counters[0], 1u);
  if (k < A.ahit_cap) {
    uint32_t* o = A.ahits + 4 * (size_t)k;
    o[0] = job; o[1] = j; o[2] = t; o[3] = kind;
  }
}

// Degenerate group j of job (a collapsed batch inverse); j | 0x80000000: a collapsed centre add in front of group j.
__device__ __forceinline__ void emit_degen(const ScanArgs& A, uint32_t job, uint32_t j) {
  const uint32_t k = atomicAdd(&A.counters[1], 1u);
  if (k < A.degen_cap) A.degen[k] = khb_degenerate{job, j};
}

}  // namespace khbk
