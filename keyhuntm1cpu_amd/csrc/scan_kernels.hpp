// Device side of libkhbsgs (gfx950): the giant-step walk and its kernel k_giant_scan<MODE>, shared by
// the translation units that instantiate it (k_bsgs.hip: -m bsgs scan / x dump; k_addr*.hip: -m address, -m xpoint;
// k_vanity.hip: -m vanity; k_baby.hip: baby-step tables) and by khbsgs.hip (launch_scan, the C ABI).  Splitting the
// instances over units lets `make -j` compile them in parallel; device/scan_modes.hpp says what each mode is.
//
// Hot path replaced: keyhunt.cpp:3867-4004 (thread_process_bsgs group loop + level-1 bloom probe).
//
// Work decomposition:
//   job   = one (chunk, target) pair; the host supplies its group-0 centre startP.
//   item  = consecutive 1024-point groups of one job (scan_batch: 8 groups with two inversions).
//   grid  = persistent: one residency of lanes; each wave takes the next 64 items from a launch counter.
// One lane's group maps 1:1 onto one reference group, so a collapsed batch inverse (dx == 0)
// reproduces the reference's all-zero inverses exactly (IntGroup.cpp:36-58 + IntMod.cpp:497-500).
// This file keeps the kernel, its work-item handout and the launch's counters; the rest is under device/ (DESIGN.md §2).
#pragma once
#include "device/walk.hpp"

namespace khbk {

// Groups walked by the launch: a wave sum of every lane's count, one 64-bit atomic per wave into
// counters[4..5].  The host compares it with n_jobs x group_count (khb_collect: KHB_EINCOMPLETE), so
// a work-item handout that skipped or repeated a group cannot go unnoticed.  Called with the wave
// reconverged (after the item loop).
__device__ __forceinline__ void count_walked(uint32_t* counters, uint32_t walked) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) walked += __shfl_xor(walked, o);
  if ((threadIdx.x & 63u) == 0 && walked)
    atomicAdd(reinterpret_cast<unsigned long long*>(counters + 4), (unsigned long long)walked);
}

// Shader clock over the launch: the first wave of block 0 samples s_memtime (shader clock) and
// s_memrealtime (100 MHz) when it starts and when it leaves (it takes work items until the launch's
// queue is empty, so it spans the launch); the host turns the two deltas into MHz (khb_stats.shader_mhz).
// The samples are stored with ordinary (vector) global stores by one lane.
__device__ __forceinline__ void clock_probe(uint32_t* counters, int at) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const uint64_t t = __builtin_amdgcn_s_memtime(), r = __builtin_amdgcn_s_memrealtime();
    uint64_t* c = reinterpret_cast<uint64_t*>(counters + 8) + 2 * at;
    // agent-scope (write-through) vector stores: launch_epilogue's last wave may run on another XCD
    __hip_atomic_store(c, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(c + 1, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// End of a launch without copy kernels (round 5): every wave releases its counter updates and adds one to
// counters[3]; the wave whose add is the launch's last reads the counters memory-side (agent-scope atomics,
// coherent across the XCDs' L2s), writes them to the slot's pinned host block with vector stores and zeroes
// counters[0..7] for the slot's next launch.  With the candidate / degenerate rings and the centres in
// pinned host memory as well, a khb_submit stream holds only this kernel and its two events: no memset
// before it and no device-to-host blit after it, which had waited for CU slots behind the other slot's
// persistent scan.  khb_collect checks host counters[3] == total_waves.
__device__ __forceinline__ void launch_epilogue(const ScanArgs& A) {
  if (!A.host_counters) return;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");     // this wave's atomics and probe stores have landed
  uint32_t prev = 0;
  if ((threadIdx.x & 63u) == 0)
    prev = __hip_atomic_fetch_add(&A.counters[3], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  prev = __shfl(prev, 0);
  if (prev != A.total_waves - 1) return;
  const uint32_t l = threadIdx.x & 63u;
  if (l < 16) {
    const uint32_t v = l < 8 ? __hip_atomic_exchange(&A.counters[l], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                             : __hip_atomic_fetch_add(&A.counters[l], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    A.host_counters[l] = v;
  }
  // the launch's end on the shader clock and the 100 MHz clock ([16..19]): with block 0's start sample on the
  // 100 MHz clock ([10..11]; s_memrealtime is one clock for the device, s_memtime one per XCD) the host gets
  // the launch's execution span, which the events cannot give while the other slot's launch still holds the
  // CUs the queued kernel waits for (khb_stats.kernel_ms)
  const uint64_t t = __builtin_amdgcn_s_memtime(), r = __builtin_amdgcn_s_memrealtime();
  if (l < 4) A.host_counters[16 + l] = (uint32_t)((l < 2 ? t : r) >> (32 * (l & 1u)));
  __threadfence_system();
}

template <int MODE>
__global__ __launch_bounds__(kBlock, waves_per_simd(MODE)) void k_giant_scan(ScanArgs A) {
  clock_probe(A.counters, 0);
  constexpr bool QUEUE = is_scan(MODE);
  const uint32_t lane = blockIdx.x * blockDim.x + threadIdx.x;
  Fe* scr = A.scratch + lane;
  __shared__ uint32_t s_queue[QUEUE ? kWavesPerBlock : 1][QUEUE ? kQWords * kQCap : 1];
  __shared__ uint32_t s_count[kWavesPerBlock];
  const uint32_t wave = QUEUE ? threadIdx.x >> 6 : 0;
  ProbeQueue Q{s_queue[wave], (volatile __attribute__((address_space(3))) uint32_t*)&s_count[wave]};
  if (QUEUE) *Q.n = 0;
  if constexpr (is_vanity(MODE)) vanity_load_bitmap(A.van_bitmap);   // before any lane leaves: it ends in a barrier
  uint32_t walked = 0;     // groups this lane walked (count_walked: the host checks the launch's total)
  // Dynamic work items: each wave takes the next 64 items from a launch-wide counter
  // (counters[2], zeroed per launch), so a wave that runs ahead keeps taking work and every SIMD
  // stays 4 waves deep until the queue is empty; a static lane-strided split left the launch's
  // tail to its slowest waves.  Each lane keeps its own scratch column (scr) for every item.
  for (;;) {
    const uint32_t wl = threadIdx.x & 63u;
    uint32_t b = 0;
    if (wl == 0) b = atomicAdd(&A.counters[2], 64u);
    b = __builtin_amdgcn_readfirstlane(b);
    if (b >= A.n_items) break;
    const uint64_t item = (uint64_t)b + wl;
    if (item >= A.n_items) continue;               // the launch's last 64 items may be ragged
    const uint32_t job = (uint32_t)(item / A.lanes_per_job);
    const uint32_t m = (uint32_t)(item % A.lanes_per_job);
    if constexpr (is_batched(MODE)) {
      const uint32_t g0 = A.group_begin + m * kBatch;
      const uint32_t g1 = min(g0 + kBatch, A.group_end);
      walked += scan_batch<MODE>(A, Q, job, g0, g1, scr);
    } else {
      const uint32_t g0 = A.group_begin + m * A.gpl;
      const uint32_t g1 = min(g0 + A.gpl, A.group_end);
      AffPt C = A.centres[job];
      const uint32_t mo = g0 / A.gpl;
      if (mo != 0) {
        if (add_direct(C, C, A.offs[mo]) && !is_dump(MODE)) emit_degen(A, job, g0 | 0x80000000u);
      }
      for (uint32_t j = g0; j < g1; ++j, ++walked) scan_group<MODE>(A, C, job, j, scr);
    }
  }
  if (QUEUE) q_drain(A, Q, 1);   // the wave has reconverged: finish what is still queued
  count_walked(A.counters, walked);
  clock_probe(A.counters, 1);
  launch_epilogue(A);
}

// The launch of every instance.  A unit states its instances once, as a ScanInstances<...> object, and launch_scan
// (khbsgs.hip) finds them by mode: KHB_EINVAL for a mode no unit instantiates.  The compiler emits a unit's kernels in
// the reverse of its list, so the lists run from the last instance to the first: the code objects' layout of before.
using ScanLauncher = void (*)(uint32_t blocks, hipStream_t stream, const ScanArgs& A);
extern ScanLauncher g_scan_launchers[kModeCount];

template <int MODE>
void launch_instance(uint32_t blocks, hipStream_t stream, const ScanArgs& A) {
  hipLaunchKernelGGL(k_giant_scan<MODE>, dim3(blocks), dim3(kBlock), 0, stream, A);
}

template <int... MODES>
struct ScanInstances {
  ScanInstances() { ((g_scan_launchers[MODES] = &launch_instance<MODES>), ...); }
};

int launch_scan(int mode, uint32_t blocks, hipStream_t stream, const ScanArgs& A);

}  // namespace khbk
