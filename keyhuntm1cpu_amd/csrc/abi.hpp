// Host side of libkhbsgs.so shared by the translation units behind include/khbsgs.h: the context and its
// submission slots, error mapping, an owned device buffer and the helpers more than one unit uses.
//   khbsgs.hip        contexts, slots, the scan ABI (submit / collect / scan of both kinds; `search` to a kernel mode
//                     by device/scan_modes.hpp) and launch_scan, the one way to a k_giant_scan launch for every unit
//   khb_tables.hip    table loads, gate stages, baby and resident builds, the resident inspection calls
//   khb_selftest.hip  field / probe / hash160 self-tests and the point dumps
//   k_check.hip       the second / third check: its kernel, tables and khb_check
//   k_mini.hip        -m minikeys: its kernels, table, launch state and the khb_mini_* calls
//   k_kang.hip        the kangaroo walk: its kernels, herd state, rings and the khb_kang_* calls
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <new>
#include <utility>
#include <vector>
#include "scan_kernels.hpp"
#include "device/confirm.hpp"

namespace khbk {
struct CheckIn;                        // k_check.hip
struct CheckOut;
struct MiniState;                      // k_mini.hip
struct KangState;                      // k_kang.hip
}  // namespace khbk

// One submission's device state.  A context owns two (KHB_QUEUE_DEPTH): khb_submit fills the next
// free slot on its own stream, so a second batch's workgroups take the CUs the first batch's last
// waves leave idle (its launch tail), and khb_collect retires the slots in submission order.
//
// Round 5: the scans' host hand-over lives in pinned, coherent host memory that the kernel reads and writes in
// place: the centres (read once per work item), the candidate / degenerate / -m address hit rings (written as
// hits occur, a few per launch) and a copy of the counters that the launch's last wave writes
// (launch_epilogue).  A khb_submit stream is then [event, kernel, event] with no memset or copy kernels, and
// khb_collect only waits for the slot's end event and copies from host memory.
struct Slot {
  hipStream_t stream = nullptr;
  khb::Fe* d_scratch = nullptr;        // lane-private prefix scratch (allocated on the slot's first use)
  khbk::AffPt* d_centres = nullptr;    // device copy for the synchronous helpers (dump, baby build)
  khbk::AffPt* h_centres = nullptr;    // pinned, coherent; the scans read it in place
  uint32_t centres_cap = 0;
  khb_cand* h_cand = nullptr;          // pinned, coherent rings written by the kernel
  khb_degenerate* h_degen = nullptr;
  uint32_t* h_ahits = nullptr;         // -m address hits (allocated on the first -m address submission)
  uint32_t* d_counters = nullptr;
  uint32_t* h_counters = nullptr;      // pinned, coherent (launch_epilogue, or a copy after the helpers)
  bool counters_zero = false;          // d_counters is all zero (a scan's epilogue left it so): no memset
  hipEvent_t ev0 = nullptr, ev1 = nullptr;   // launch begin / end (khb_stats: kernel_ms, launch_*_ms)
  uint64_t pending_steps = 0;
  uint32_t total_waves = 0;            // of the launch in flight (host_counters_ok)
  int kind = 0;                        // in flight: 1 = -m bsgs scan, 2 = -m address scan
};
constexpr int kQueueDepth = 2;

struct khb_ctx {
  int device = -1;
  int last_hip = 0;
  uint32_t handoff_seen = 0, handoff_total = 0;   // the last collect's epilogue wave count (khb_last_handoff)
  uint32_t lanes = 0;
  uint8_t* d_bloom = nullptr;          // 256 x geom.bytes_per_sub bytes (a whole number of 32-bit words)
  khb::BloomGeom geom{};
  uint64_t gate_bytes = 0;             // of d_gate (up to 32 GiB: khb_build_l1_resident)
  uint8_t* d_gate = nullptr;           // level-0 gate (khb_load_gate), null = none
  uint8_t* d_gate1 = nullptr;          // its stage-1 fold, null = none
  uint32_t gate1_mask = 0;
  uint32_t gate1_log2 = KHB_GATE1;     // khb_set_gate_stage1: fold size for gates loaded later
  uint32_t* d_gate0 = nullptr;         // the stage-0 filter, null = none
  uint32_t gate0_mask = 0;
  uint32_t gate0_log2 = KHB_GATE0;     // khb_set_gate_stage0: filter size for gates loaded later
  uint32_t gate_mask = 0, gate_probes = 0;
  khbk::AffPt* d_gsn = nullptr;
  khbk::AffPt* d_offs = nullptr;
  uint32_t n_offs = 0, gpl = 0;
  khbk::AffPt* d_gofs = nullptr;       // per-group offsets expanded from gpl > 1 lane offsets
  bool gofs_stale = true;
  Slot slot[kQueueDepth];              // slot[0] also serves the synchronous helpers (dump, self-tests)
  int head = 0;                        // oldest in-flight slot
  int queued = 0;                      // submissions in flight (0..kQueueDepth)
  uint32_t cand_cap = khbk::kCandCap;  // candidate ring entries a launch may fill (khb_set_candidate_capacity)
  // The context's clock (khb_stats.launch_begin_ms / launch_end_ms; khb_reset_epoch restarts it): the
  // `epoch` event sits epoch_ms after the clock's origin.  hipEventElapsedTime is a float, so the anchor
  // moves forward once its distance to a launch passes kReanchorMs (a float ms keeps ~4 us at 60 s, but
  // ~1 ms after 4.6 h): begin = epoch_ms + elapsed(epoch, ev0) in double, end = begin + the launch's own
  // elapsed(ev0, ev1) (the busy-time union no longer drifts on long CLI runs).
  // The previous anchor stays valid as a fallback for a launch of the other slot that began before the
  // current anchor was recorded (a negative distance).
  hipEvent_t epoch = nullptr;
  hipEvent_t epoch_prev = nullptr;
  double epoch_ms = 0.0, epoch_prev_ms = 0.0;
  bool have_prev = false;
  // -m address
  uint8_t* d_abloom = nullptr;
  khb::BloomGeom ageom{};
  // -m vanity (khb_load_vanity): van_n intervals as lo words [5 van_n], hi words [5 van_n], then the bucket bitmap
  // (kVanityBitmapWords words), one allocation; null = none loaded
  uint32_t* d_van = nullptr;
  uint32_t van_n = 0;
  // -m minikeys (k_mini.hip): the window table of khb_load_mini_table, the launch state (a stream and queues of the
  // mode's own, allocated on first use) and the survivor queue's capacity (0 = sized from the launch)
  khb::CPt* d_mini_tab = nullptr;
  uint32_t mini_w = 0;
  khbk::MiniState* mini = nullptr;
  uint32_t mini_queue_cap = 0;
  bool mini_busy = false;              // a khb_mini_submit is in flight
  // second / third check (khb_load_check_tables, khb_check): tables, a high-priority stream of its own
  // and buffers grown to the largest batch
  khb::CheckTables ck{};
  void* d_ck = nullptr;                // one allocation holding every check table
  bool ck_loaded = false;
  hipStream_t ck_stream = nullptr;
  khbk::CheckIn* d_ck_in = nullptr;
  khbk::CheckOut* d_ck_out = nullptr;
  khb::CPt* d_ck_targets = nullptr;
  uint32_t ck_cap = 0, ck_tcap = 0;
  // the targets on the device (d_ck_targets) as the caller passed them: a khb_check with the same bytes
  // uploads only its CheckIn records (no O(n_targets) conversion and upload per batch)
  std::vector<uint8_t> ck_targets_be;
  // the kangaroo walk (k_kang.hip): jump table, herd state, rings and a stream of its own, allocated on first use
  khbk::KangState* kang = nullptr;
};

#pragma GCC visibility push(hidden)    // the library exports the khb_* of include/khbsgs.h only
namespace khbk {

inline int hip_fail(khb_ctx* c, hipError_t e) {
  if (c) c->last_hip = (int)e;
  // The runtime keeps the last error for hipGetLastError: a failed allocation the caller recovers
  // from (khb_reserve_slots -> depth 1) would otherwise fail the next launch check of khb_submit.
  (void)hipGetLastError();
  return e == hipErrorOutOfMemory ? KHB_ENOMEM : KHB_EHIP;
}
#define KHB_TRY(c, x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return hip_fail((c), e_); } while (0)

// A device allocation that lives as long as its scope.
template <class T>
struct DevBuf {
  T* p = nullptr;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { hipFree(p); }
  hipError_t alloc(size_t n) { return hipMalloc(&p, sizeof(T) * n); }
  operator T*() const { return p; }
};

// Host staging of n elements; false when the allocation fails (KHB_ENOMEM).
template <class T>
bool host_alloc(std::vector<T>& v, size_t n) {
  try {
    v.resize(n);
  } catch (const std::bad_alloc&) {
    return false;
  }
  return true;
}

// After a kernel launch on `stream`: the launch's error, then the stream drained.
inline int sync_launch(khb_ctx* c, hipStream_t stream) {
  KHB_TRY(c, hipGetLastError());
  KHB_TRY(c, hipStreamSynchronize(stream));
  return KHB_OK;
}

// n big-endian x||y points (64 bytes each) as little-endian limbs (AffPt, khb::CPt).
template <class Pt>
void pts_from_be(Pt* dst, const uint8_t* src, uint32_t n) {
  for (uint32_t i = 0; i < n; ++i) {
    fe_from_be(dst[i].x, src + 64 * (size_t)i);
    fe_from_be(dst[i].y, src + 64 * (size_t)i + 32);
  }
}

// n big-endian field elements (32 bytes each).
inline void fes_from_be(Fe* dst, const uint8_t* src, uint32_t n) {
  for (uint32_t i = 0; i < n; ++i) fe_from_be(dst[i], src + 32 * (size_t)i);
}

// A bloom level's geometry with the Barrett constants of mod_bits (bloom_probe.hpp).
inline BloomGeom bloom_geom(uint64_t bytes_per_sub, uint64_t bits, uint32_t hashes) {
  BloomGeom g{};
  g.bytes_per_sub = bytes_per_sub;
  g.bits = bits;
  g.magic = (uint64_t)(((unsigned __int128)1 << 64) / bits);
  g.wrap = (uint64_t)(((unsigned __int128)1 << 64) % bits);
  g.hashes = hashes;
  return g;
}

inline bool bloom_args_ok(uint64_t bytes, uint64_t bits, uint32_t hashes) {
  return bytes && bits >= 2 && (bits + 7) / 8 == bytes && hashes && hashes <= 255;   // bloom.cpp:110-113
}

// A level-0 gate of 2^log2_bits bits (at most 2^max_log2) with `probes` bits per x.
inline bool gate_args_ok(uint32_t log2_bits, uint32_t probes, uint32_t max_log2) {
  return log2_bits >= 13 && log2_bits <= max_log2 && probes >= 1 && probes <= KHB_GATE_MAX_PROBES;
}

// Groups the slot's last launch walked (count_walked, copied back with the counters).
inline uint64_t walked_groups(const Slot& S) {
  uint64_t v;
  memcpy(&v, S.h_counters + 4, sizeof v);
  return v;
}

// Entries (32 B) of lane-private scratch (device/walk.hpp): scan_group needs 512, scan_batch kBatch*514 + kBatch.
constexpr size_t kScratchEntries = (size_t)kBatch * (kHalf + 3) > kHalf ? (size_t)kBatch * (kHalf + 3) : kHalf;

// Defined in khbsgs.hip: the slot's centre buffers grown to n jobs, the per-group offsets of the batched walks, the
// shape checks every walk shares (bsgs: also the 32-bit step index), and a launch's arguments from the context.
int ensure_centres(khb_ctx* c, Slot& S, uint32_t n);
int ensure_gofs(khb_ctx* c);
int check_scan_args(khb_ctx* c, const uint8_t* centres, uint32_t n_jobs, uint32_t group_begin, uint32_t group_count,
                    bool bsgs);
ScanArgs make_args(khb_ctx* c, const Slot& S, uint32_t n_jobs, uint32_t group_begin, uint32_t group_count,
                   uint32_t per_item = 0);
// Defined in k_mini.hip: frees the context's -m minikeys state (khb_close).
void mini_free(khb_ctx* c);
// Defined in k_kang.hip: frees the context's kangaroo state (khb_close).
void kang_free(khb_ctx* c);

}  // namespace khbk
#pragma GCC visibility pop
