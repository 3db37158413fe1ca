// libkhbsgs.so -- MI355X (gfx950) BSGS giant-step engine behind the C ABI of include/khbsgs.h.  This unit: contexts,
// submission slots and the scan ABI, i.e. the launches of the k_giant_scan scan instances (scan_kernels.hpp +
// device/walk.hpp, scan_args.hpp; instantiated in k_bsgs/k_addr*.hip).  abi.hpp lists the other units.
#include "abi.hpp"

using namespace khbk;

namespace {

// Per-group centre offsets gofs[j] = j*_2GSn from lane offsets offs[m] = (m*gpl)*_2GSn:
// gofs[m*gpl + k] = offs[m] + k*_2GSn (gofs[0] is unused: group 0's centre is startP).
__global__ void k_expand_offsets(const AffPt* __restrict__ offs, uint32_t gpl, const AffPt* __restrict__ gsn,
                                 AffPt* __restrict__ out, uint32_t n) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint32_t m = j / gpl, k = j % gpl;
  const AffPt D = gsn[kHalf];
  AffPt p = offs[m];
  uint32_t todo = k;
  if (m == 0 && k) {
    p = D;
    todo = k - 1;
  }
  for (uint32_t t = 0; t < todo; ++t) {
    if (fe_eq(p.x, D.x)) {      // p == D (small multiples never meet -D): DoubleDirect, SECP256K1.cpp:376-401
      Fe x2, num, den, s, x, y;
      fm_sqr(x2, p.x);
      fm_canon(x2, x2);
      fm_add(num, x2, x2);
      fm_add(num, num, x2);
      fm_add(den, p.y, p.y);
      fm_inv(den, den);
      fm_mul(s, num, den);
      fm_canon(s, s);
      fm_sqr(x, s);
      fm_sub(x, x, p.x);
      fm_sub(x, x, p.x);
      fm_canon(x, x);
      fm_sub(y, p.x, x);
      fm_mul(y, y, s);
      fm_sub(y, y, p.y);
      fm_canon(y, y);
      p = AffPt{x, y};
    } else {
      add_direct(p, p, D);
    }
  }
  out[j] = p;
}

void free_slot(Slot& S);

// Device state of a slot: slot 0 at khb_open, slot 1 on the first queued submission or up front by
// khb_reserve_slots.  A failure part-way frees what was allocated, so the slot is either complete or
// empty (and the caller may go on with the slots it has).
int ensure_slot_alloc(khb_ctx* c, Slot& S) {
  KHB_TRY(c, hipStreamCreateWithFlags(&S.stream, hipStreamNonBlocking));
  KHB_TRY(c, hipMalloc(&S.d_scratch, sizeof(Fe) * kScratchEntries * c->lanes));
  KHB_TRY(c, hipHostMalloc((void**)&S.h_cand, sizeof(khb_cand) * kCandCap, hipHostMallocCoherent));
  KHB_TRY(c, hipHostMalloc((void**)&S.h_degen, sizeof(khb_degenerate) * kDegenCap, hipHostMallocCoherent));
  KHB_TRY(c, hipMalloc(&S.d_counters, kCounterBytes));
  // on the slot's own stream: a null-stream hipMemset of device memory may still be queued (behind the other
  // slot's running launch, for CU slots) when this slot's first launch starts, and would zero its counters
  // mid-launch (round 5: a lazily allocated slot 1 re-walked 6,144 groups, tools/debug/epilogue_diag.py)
  KHB_TRY(c, hipMemsetAsync(S.d_counters, 0, kCounterBytes, S.stream));
  S.counters_zero = true;
  KHB_TRY(c, hipHostMalloc((void**)&S.h_counters, kHostCounterBytes, hipHostMallocCoherent));
  KHB_TRY(c, hipEventCreate(&S.ev0));
  KHB_TRY(c, hipEventCreate(&S.ev1));
  return KHB_OK;
}

int ensure_slot(khb_ctx* c, Slot& S) {
  if (S.ev1) return KHB_OK;            // complete (ev1 is created last)
  const int rc = ensure_slot_alloc(c, S);
  if (rc) free_slot(S);
  return rc;
}

void free_slot(Slot& S) {
  if (S.stream) hipStreamSynchronize(S.stream);
  hipFree(S.d_scratch);
  hipFree(S.d_centres);
  if (S.h_cand) hipHostFree(S.h_cand);
  if (S.h_degen) hipHostFree(S.h_degen);
  if (S.h_ahits) hipHostFree(S.h_ahits);
  hipFree(S.d_counters);
  if (S.h_counters) hipHostFree(S.h_counters);
  if (S.h_centres) hipHostFree(S.h_centres);
  if (S.ev0) hipEventDestroy(S.ev0);
  if (S.ev1) hipEventDestroy(S.ev1);
  if (S.stream) hipStreamDestroy(S.stream);
  S = Slot{};
}

// The slot the next submission uses (KHB_EBUSY when every slot is in flight).
Slot* next_slot(khb_ctx* c, int& rc) {
  if (c->queued >= kQueueDepth) { rc = KHB_EBUSY; return nullptr; }
  // With nothing in flight the ring restarts at slot 0 (allocated by khb_open), so a caller that keeps
  // one submission in flight -- the depth-1 fallback after KHB_ENOMEM from khb_reserve_slots -- never
  // touches slot 1.  Collect order stays submission order.
  if (c->queued == 0) c->head = 0;
  Slot& S = c->slot[(c->head + c->queued) % kQueueDepth];
  rc = ensure_slot(c, S);
  return rc ? nullptr : &S;
}

// kernel_ms and the launch's interval on the context's clock (khb_reset_epoch), from the slot's events;
// the shader clock from the kernel's clock_probe samples.
// Called after S's stream has drained (the slot's launch is complete and the stream idle).
//
// Round 5: a scan launched by khb_submit / khb_addr_submit (launch_epilogue) is timed by its own clocks: block 0's
// first wave samples s_memtime / s_memrealtime when it starts (the launch's first workgroup) and the launch's last
// wave when it leaves, so kernel_ms is the launch's execution span on the 100 MHz clock and the shader clock is
// the average over that span.  The interval on the context's clock ends at the slot's end event and begins that
// span earlier.  The events alone would also count the time the queued launch waits, dispatched, for the CUs
// the other slot's running launch still holds (nothing but a kernel sits on the slot's stream since round 5).
constexpr float kReanchorMs = 60000.f;
void launch_times(khb_ctx* c, const Slot& S, khb_stats* st, bool epilogue) {
  uint64_t p[4], q[2];
  memcpy(p, S.h_counters + 8, sizeof p);
  memcpy(q, S.h_counters + 16, sizeof q);
  // The shader clock from block 0's first wave alone (its start and exit): s_memtime counts per XCD, so a
  // ratio across two waves on different XCDs is meaningless.  The 100 MHz s_memrealtime is one clock for the
  // whole device: the execution span runs from block 0's start to the last wave's exit (q[1]).
  const bool clocks = p[3] > p[1] && p[2] > p[0];
  st->shader_mhz = clocks ? (float)(100.0 * (double)(p[2] - p[0]) / (double)(p[3] - p[1])) : 0.f;
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, S.ev0, S.ev1) != hipSuccess) ms = -1.f;
  st->event_ms = ms;
  if (epilogue && q[1] > p[1] && ms >= 0.f) {
    const float span = (float)((double)(q[1] - p[1]) * 1e-5);     // 100 MHz ticks -> ms
    if (span < ms) ms = span;
  }
  st->kernel_ms = ms;
  float e = -1.f, ep = -1.f, b = -1.f;
  double end = -1.0;
  const bool cur = c->epoch && hipEventElapsedTime(&b, c->epoch, S.ev0) == hipSuccess && b >= 0.f;
  if (cur && hipEventElapsedTime(&e, c->epoch, S.ev1) == hipSuccess && e >= 0.f)
    end = c->epoch_ms + (double)e;
  else if (c->have_prev && hipEventElapsedTime(&ep, c->epoch_prev, S.ev1) == hipSuccess && ep >= 0.f)
    end = c->epoch_prev_ms + (double)ep;
  if (end >= 0.0 && ms >= 0.f) {
    st->launch_begin_ms = end - (double)ms;
    st->launch_end_ms = end;
  } else {
    st->launch_begin_ms = st->launch_end_ms = -1.0;
  }
  float d = 0.f;
  if (cur && b > kReanchorMs && c->epoch_prev && hipEventRecord(c->epoch_prev, S.stream) == hipSuccess &&
      hipEventSynchronize(c->epoch_prev) == hipSuccess &&
      hipEventElapsedTime(&d, c->epoch, c->epoch_prev) == hipSuccess) {
    // the new anchor (recorded now on the idle stream) becomes current; the old one the fallback
    std::swap(c->epoch, c->epoch_prev);
    c->epoch_prev_ms = c->epoch_ms;
    c->epoch_ms += (double)d;
    c->have_prev = true;
  }
}

// The scans' launch without copy kernels: centres read in place from the slot's pinned block, counters
// zeroed by the previous scan's epilogue (a memset only after a helper used them), the last wave's copy of
// them in h_counters; h_counters[3] is poisoned so that khb_collect can tell the epilogue ran.
int prepare_host_launch(khb_ctx* c, Slot& S, ScanArgs& A, uint32_t blocks) {
  if (!S.counters_zero) KHB_TRY(c, hipMemsetAsync(S.d_counters, 0, kCounterBytes, S.stream));
  S.counters_zero = false;             // until khb_collect sees the epilogue's copy
  memset(S.h_counters, 0, kHostCounterBytes);
  S.h_counters[3] = 0xFFFFFFFFu;
  A.centres = S.h_centres;
  A.host_counters = S.h_counters;
  A.total_waves = blocks * kWavesPerBlock;
  return KHB_OK;
}

// After the slot's end event: the epilogue's copy is complete iff it counted every wave of the launch.
// The launch epilogue counted every wave (else KHB_EHANDOFF; the counts are kept for khb_last_handoff).
bool host_counters_ok(khb_ctx* c, const Slot& S) {
  c->handoff_seen = S.h_counters[3];
  c->handoff_total = S.total_waves;
  return S.h_counters[3] == S.total_waves;
}

}  // namespace

namespace khbk {

int ensure_centres(khb_ctx* c, Slot& S, uint32_t n) {
  if (n <= S.centres_cap) return KHB_OK;
  if (S.d_centres) hipFree(S.d_centres);
  if (S.h_centres) hipHostFree(S.h_centres);
  S.d_centres = nullptr;
  S.h_centres = nullptr;
  S.centres_cap = 0;
  uint32_t cap = n < 1024 ? 1024 : n;
  KHB_TRY(c, hipMalloc(&S.d_centres, sizeof(AffPt) * cap));
  KHB_TRY(c, hipHostMalloc((void**)&S.h_centres, sizeof(AffPt) * cap, hipHostMallocCoherent));
  S.centres_cap = cap;
  return KHB_OK;
}

// per_item: groups per work item (the lane-offset stride gpl, or kBatch for scan_batch modes)
ScanArgs make_args(khb_ctx* c, const Slot& S, uint32_t n_jobs, uint32_t group_begin, uint32_t group_count,
                   uint32_t per_item) {
  ScanArgs A{};
  if (per_item == 0) per_item = c->gpl;
  A.bloom = c->d_bloom;
  A.geom = c->geom;
  A.gate = c->d_gate;
  A.gate_mask = c->gate_mask;
  A.gate_probes = c->gate_probes;
  A.gate1 = c->d_gate1;
  A.gate1_mask = c->gate1_mask;
  A.gate0 = c->d_gate0;
  A.gate0_mask = c->gate0_mask;
  A.gsn = c->d_gsn;
  A.offs = c->d_offs;
  A.gofs = c->gpl == 1 ? c->d_offs : c->d_gofs;
  A.centres = S.d_centres;
  A.scratch = S.d_scratch;
  A.cand = S.h_cand;
  A.degen = S.h_degen;
  A.counters = S.d_counters;
  A.n_jobs = n_jobs;
  A.group_begin = group_begin;
  A.group_end = group_begin + group_count;
  A.gpl = c->gpl;
  A.lanes_per_job = (group_count + per_item - 1) / per_item;
  A.n_items = (uint64_t)n_jobs * A.lanes_per_job;
  A.stride = c->lanes;
  A.cand_cap = c->cand_cap;
  A.degen_cap = kDegenCap;
  return A;
}

int check_scan_args(khb_ctx* c, const uint8_t* centres, uint32_t n_jobs, uint32_t group_begin, uint32_t group_count,
                    bool bsgs) {
  if (!c || !centres || n_jobs == 0 || group_count == 0) return KHB_EINVAL;
  if (!c->d_gsn || !c->d_offs || c->gpl == 0) return KHB_ESTATE;
  if (group_begin % c->gpl) return KHB_EINVAL;
  uint64_t end = (uint64_t)group_begin + group_count;
  if (end > 0xFFFFFFFFull) return KHB_EINVAL;
  if (bsgs && end * KHB_GROUP > 0xFFFFFFFFull) return KHB_EINVAL;  // a = j*1024+t fits 32 bits (keyhunt.cpp:3948)
  if ((end + c->gpl - 1) / c->gpl > c->n_offs) return KHB_EINVAL;  // offsets table too short
  return KHB_OK;
}

// Per-group centre offsets for scan_batch: the lane offsets themselves when gpl == 1, else
// expanded once on the device (k_expand_offsets) after the giant table and offsets are loaded.
int ensure_gofs(khb_ctx* c) {
  if (c->gpl == 1 || !c->gofs_stale) return KHB_OK;
  const uint32_t n = c->n_offs * c->gpl;
  if (c->d_gofs) { hipFree(c->d_gofs); c->d_gofs = nullptr; }
  KHB_TRY(c, hipMalloc(&c->d_gofs, sizeof(AffPt) * (size_t)n));
  hipLaunchKernelGGL(k_expand_offsets, dim3((n + 255) / 256), dim3(256), 0, c->slot[0].stream, c->d_offs, c->gpl,
                     c->d_gsn, c->d_gofs, n);
  if (const int rc = sync_launch(c, c->slot[0].stream)) return rc;
  c->gofs_stale = false;
  return KHB_OK;
}

ScanLauncher g_scan_launchers[kModeCount];   // filled by the units' ScanInstances while the library loads

int launch_scan(int mode, uint32_t blocks, hipStream_t stream, const ScanArgs& A) {
  if (mode < 0 || mode >= kModeCount || !g_scan_launchers[mode]) return KHB_EINVAL;
  g_scan_launchers[mode](blocks, stream, A);
  return KHB_OK;
}

}  // namespace khbk

namespace {

// khb_submit (kind 1: -m bsgs over the level-1 bloom, kBatch groups per item on the per-group offsets) and
// khb_addr_submit (kind 2: -m address over the address bloom, gpl groups per item, hits in the slot's h_ahits;
// `search` selects the kernel, BTC hash160, -c eth, -m xpoint or -m vanity, and is not read for kind 1).
int submit_scan(khb_ctx* c, int kind, const uint8_t* centres, uint32_t n_jobs, uint32_t group_begin,
                uint32_t group_count, int search) {
  const bool bsgs = kind == 1;
  int rc = check_scan_args(c, centres, n_jobs, group_begin, group_count, bsgs);
  if (rc) return rc;
  SearchMode sm;
  if (!bsgs && !decode_search(search, sm)) return KHB_EINVAL;
  if (!(bsgs ? (void*)c->d_bloom : sm.vanity ? (void*)c->d_van : (void*)c->d_abloom)) return KHB_ESTATE;
  if (c->queued && c->slot[c->head].kind != kind) return KHB_EBUSY;     // a scan of the other kind is in flight
  if (c->mini_busy) return KHB_EBUSY;                                   // or a -m minikeys launch
  KHB_TRY(c, hipSetDevice(c->device));
  Slot* Sp = next_slot(c, rc);
  if (!Sp) return rc;
  Slot& S = *Sp;
  if ((rc = ensure_centres(c, S, n_jobs))) return rc;
  if (bsgs) {
    if ((rc = ensure_gofs(c))) return rc;
  } else if (!S.h_ahits) {
    KHB_TRY(c, hipHostMalloc((void**)&S.h_ahits, sizeof(khb_addr_hit) * kAddrHitCap, hipHostMallocCoherent));
  }
  ScanArgs A = make_args(c, S, n_jobs, group_begin, group_count, bsgs ? kBatch : 0);
  if (bsgs) {
    if (A.n_items > 0xFFFFFF00ull) return KHB_EINVAL;      // the 32-bit work-item counter (KHB_DYN)
  } else {
    A.bloom = c->d_abloom;
    A.geom = c->ageom;
    A.ahits = S.h_ahits;
    A.ahit_cap = khb_addr_hit_capacity(c);
    if (sm.vanity) {
      A.van_lo = c->d_van;
      A.van_hi = c->d_van + 5 * (size_t)c->van_n;
      A.van_bitmap = c->d_van + 10 * (size_t)c->van_n;
      A.van_n = c->van_n;
    }
  }
  pts_from_be(S.h_centres, centres, n_jobs);
  const uint32_t blocks = c->lanes / kBlock;
  if ((rc = prepare_host_launch(c, S, A, blocks))) return rc;
  KHB_TRY(c, hipEventRecord(S.ev0, S.stream));
  const int mode = bsgs ? (c->d_gate0 ? kScanG2 : c->d_gate1 ? kScanG1 : c->d_gate ? kScanG : kScan) : scan_mode_of(sm);
  if ((rc = launch_scan(mode, blocks, S.stream, A))) return rc;
  KHB_TRY(c, hipGetLastError());
  KHB_TRY(c, hipEventRecord(S.ev1, S.stream));
  S.total_waves = A.total_waves;
  S.kind = kind;
  S.pending_steps = (uint64_t)n_jobs * group_count * KHB_GROUP;
  c->queued++;
  return KHB_OK;
}

// khb_collect (kind 1: `out` takes khb_cand entries, degen the degenerate ring) and khb_addr_collect (kind 2: `out`
// takes khb_addr_hit entries; degen is null) of the oldest submission, which must be of that kind.
int collect_scan(khb_ctx* c, int kind, void* out, uint32_t cap, khb_degenerate* degen, uint32_t degen_cap,
                 khb_stats* st) {
  if (!c) return KHB_EINVAL;
  if (!c->queued || c->slot[c->head].kind != kind) return KHB_ESTATE;
  KHB_TRY(c, hipSetDevice(c->device));
  Slot& S = c->slot[c->head];
  S.kind = 0;
  c->head = (c->head + 1) % kQueueDepth;
  c->queued--;
  KHB_TRY(c, hipEventSynchronize(S.ev1));
  if (!host_counters_ok(c, S)) return KHB_EHANDOFF;   // the launch's epilogue did not complete
  S.counters_zero = true;
  const bool bsgs = kind == 1;
  const uint32_t n = S.h_counters[0], nd = S.h_counters[1];
  const uint32_t ring_cap = bsgs ? c->cand_cap : khb_addr_hit_capacity(c);
  uint32_t take = n < ring_cap ? n : ring_cap;
  if (take > cap) take = cap;
  if (take && out) {
    if (bsgs)
      memcpy(out, S.h_cand, sizeof(khb_cand) * take);
    else
      memcpy(out, S.h_ahits, sizeof(khb_addr_hit) * take);
  }
  uint32_t dt = nd < kDegenCap ? nd : kDegenCap;
  if (dt > degen_cap) dt = degen_cap;
  if (dt && degen) memcpy(degen, S.h_degen, sizeof(khb_degenerate) * dt);
  const uint64_t steps = walked_groups(S) * KHB_GROUP;
  if (st) {
    st->n_cand = n;
    st->n_degenerate = nd;
    st->giant_steps = steps;
    launch_times(c, S, st, true);
  }
  return steps == S.pending_steps ? KHB_OK : KHB_EINCOMPLETE;
}

}  // namespace

extern "C" {

const char* khb_strerror(int code) {
  switch (code) {
    case KHB_OK: return "ok";
    case KHB_EINVAL: return "invalid argument";
    case KHB_ENODEV: return "no usable gfx950 device";
    case KHB_ENOMEM: return "out of memory";
    case KHB_EHIP: return "HIP runtime error";
    case KHB_ESTATE: return "call order violated (tables not loaded?)";
    case KHB_EBUSY: return "submission in flight";
    case KHB_EINCOMPLETE: return "the device walked a different number of groups than submitted";
    case KHB_EHANDOFF: return "the launch's end-of-launch hand-off did not count every wave (khb_last_handoff)";
    default: return "unknown error";
  }
}

int khb_last_hip_error(const khb_ctx* c) { return c ? c->last_hip : 0; }
void* khb_stream(khb_ctx* c) { return c ? (void*)c->slot[0].stream : nullptr; }
uint32_t khb_lanes(const khb_ctx* c) { return c ? c->lanes : 0; }
int khb_abi_version(void) { return KHB_ABI_VERSION; }

#ifndef KHB_VARIANT
#define KHB_VARIANT "product"        // tools/build_variant.sh names its timing builds (-DKHB_VARIANT=\"<name>\")
#endif
#ifndef KHB_BUILD_DEFINES
#define KHB_BUILD_DEFINES ""         // the extra -D flags of a tools/build_variant.sh build, comma-separated
#endif
#define KHB_STR2(x) #x
#define KHB_STR(x) KHB_STR2(x)
const char* khb_build_info(void) {
  return "abi=" KHB_STR(KHB_ABI_VERSION) " arch=gfx950 variant=" KHB_VARIANT
         " waves_per_simd=" KHB_STR(KHB_WAVES_PER_SIMD) " addr_waves_per_simd=" KHB_STR(KHB_ADDR_WAVES_PER_SIMD)
         " addr_eth_waves_per_simd=" KHB_STR(KHB_ADDR_ETH_WAVES_PER_SIMD)
         " addr_x_waves_per_simd=" KHB_STR(KHB_ADDR_X_WAVES_PER_SIMD)
         " vanity_waves_per_simd=" KHB_STR(KHB_VANITY_WAVES_PER_SIMD)
         " batch=" KHB_STR(KHB_BATCH) " gate1=" KHB_STR(KHB_GATE1) " half_stream=" KHB_STR(KHB_HALF_STREAM)
         " gate0=" KHB_STR(KHB_GATE0) " defines=" KHB_BUILD_DEFINES " compiler=" __clang_version__;
}

int khb_last_handoff(const khb_ctx* c, uint32_t* waves_seen, uint32_t* waves_total) {
  if (!c) return KHB_EINVAL;
  if (waves_seen) *waves_seen = c->handoff_seen;
  if (waves_total) *waves_total = c->handoff_total;
  return KHB_OK;
}

uint32_t khb_groups_per_item(void) { return kBatch; }

int khb_reserve_slots(khb_ctx* c, int depth) {
  if (!c || depth < 1 || depth > kQueueDepth) return KHB_EINVAL;
  if (c->queued) return KHB_EBUSY;
  KHB_TRY(c, hipSetDevice(c->device));
  for (int i = 1; i < depth; ++i) {
    const int rc = ensure_slot(c, c->slot[i]);
    if (rc) return rc;                 // the slot is left empty (ensure_slot frees a partial one)
  }
  return KHB_OK;
}

int khb_set_candidate_capacity(khb_ctx* c, uint32_t cap) {
  if (!c || cap == 0 || cap > kCandCap) return KHB_EINVAL;
  if (c->queued) return KHB_EBUSY;
  c->cand_cap = cap;
  return KHB_OK;
}

uint32_t khb_candidate_capacity(const khb_ctx* c) { return c ? c->cand_cap : 0; }

uint32_t khb_addr_hit_capacity(const khb_ctx* c) {
  return c ? (c->cand_cap < kAddrHitCap ? c->cand_cap : kAddrHitCap) : 0;
}

int khb_reset_epoch(khb_ctx* c) {
  if (!c) return KHB_EINVAL;
  if (c->queued) return KHB_EBUSY;
  KHB_TRY(c, hipSetDevice(c->device));
  KHB_TRY(c, hipEventRecord(c->epoch, c->slot[0].stream));
  c->epoch_ms = c->epoch_prev_ms = 0.0;
  c->have_prev = false;
  return KHB_OK;
}

uint32_t khb_default_lanes(int device) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return 0;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return 0;
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return 0;
  return (uint32_t)prop.multiProcessorCount * 4u * KHB_WAVES_PER_SIMD * 64u;
}

int khb_device_count(int* n) {
  if (!n) return KHB_EINVAL;
  int k = 0;
  if (hipGetDeviceCount(&k) != hipSuccess) k = 0;
  *n = k;
  return KHB_OK;
}

int khb_open(int device, uint32_t lanes, khb_ctx** out) {
  if (!out) return KHB_EINVAL;
  *out = nullptr;
  const uint32_t full = khb_default_lanes(device);     // one full residency; 0 = no such gfx950 device
  if (!full) return KHB_ENODEV;
  khb_ctx* c = new (std::nothrow) khb_ctx();
  if (!c) return KHB_ENOMEM;
  c->device = device;
  if (lanes == 0) lanes = full;
  lanes = (lanes + kBlock - 1) / kBlock * kBlock;
  c->lanes = lanes;
  hipError_t e = hipSetDevice(device);
  int rc = e == hipSuccess ? ensure_slot(c, c->slot[0]) : hip_fail(c, e);
  if (!rc && (e = hipEventCreate(&c->epoch)) == hipSuccess && (e = hipEventCreate(&c->epoch_prev)) == hipSuccess)
    e = hipEventRecord(c->epoch, c->slot[0].stream);
  if (!rc && e != hipSuccess) rc = hip_fail(c, e);
  if (rc) {
    khb_close(c);
    return rc;
  }
  *out = c;
  return KHB_OK;
}

int khb_close(khb_ctx* c) {
  if (!c) return KHB_OK;
  if (c->device >= 0) hipSetDevice(c->device);
  for (Slot& S : c->slot) free_slot(S);
  if (c->epoch) hipEventDestroy(c->epoch);
  if (c->epoch_prev) hipEventDestroy(c->epoch_prev);
  if (c->ck_stream) {
    hipStreamSynchronize(c->ck_stream);
    hipStreamDestroy(c->ck_stream);
  }
  hipFree(c->d_ck);
  hipFree(c->d_ck_in);
  hipFree(c->d_ck_out);
  hipFree(c->d_ck_targets);
  hipFree(c->d_bloom);
  hipFree(c->d_gate);
  hipFree(c->d_gate1);
  hipFree(c->d_gate0);
  hipFree(c->d_gsn);
  hipFree(c->d_offs);
  hipFree(c->d_gofs);
  hipFree(c->d_abloom);
  hipFree(c->d_van);
  mini_free(c);
  kang_free(c);
  delete c;
  return KHB_OK;
}

int khb_mem_info(khb_ctx* c, uint64_t* free_bytes, uint64_t* total_bytes, uint64_t* slot_bytes) {
  if (!c) return KHB_EINVAL;
  KHB_TRY(c, hipSetDevice(c->device));
  size_t f = 0, t = 0;
  KHB_TRY(c, hipMemGetInfo(&f, &t));
  if (free_bytes) *free_bytes = f;
  if (total_bytes) *total_bytes = t;
  if (slot_bytes) *slot_bytes = sizeof(Fe) * kScratchEntries * c->lanes;
  return KHB_OK;
}

int khb_submit(khb_ctx* c, const uint8_t* centres, uint32_t n_jobs, uint32_t group_begin, uint32_t group_count) {
  return submit_scan(c, 1, centres, n_jobs, group_begin, group_count, 0);
}

int khb_collect(khb_ctx* c, khb_cand* cand, uint32_t cap, khb_degenerate* degen, uint32_t degen_cap, khb_stats* st) {
  return collect_scan(c, 1, cand, cap, degen, degen_cap, st);
}

int khb_scan(khb_ctx* c, const uint8_t* centres, uint32_t n_jobs, uint32_t group_begin, uint32_t group_count,
             khb_cand* cand, uint32_t cap, khb_stats* st) {
  if (c && c->queued) return KHB_EBUSY;   // khb_collect would retire the older submission, not this one
  int rc = khb_submit(c, centres, n_jobs, group_begin, group_count);
  if (rc) return rc;
  return khb_collect(c, cand, cap, nullptr, 0, st);
}

// ---------------------------------------------------------------------------------- -m address
int khb_addr_submit(khb_ctx* c, const uint8_t* centres, uint32_t n_jobs, uint32_t group_begin, uint32_t group_count,
                    int search) {
  return submit_scan(c, 2, centres, n_jobs, group_begin, group_count, search);
}

int khb_addr_collect(khb_ctx* c, khb_addr_hit* hits, uint32_t cap, khb_stats* st) {
  return collect_scan(c, 2, hits, cap, nullptr, 0, st);
}

int khb_addr_scan(khb_ctx* c, const uint8_t* centres, uint32_t n_jobs, uint32_t group_begin, uint32_t group_count,
                  int search, khb_addr_hit* hits, uint32_t cap, khb_stats* st) {
  if (c && c->queued) return KHB_EBUSY;   // as khb_scan
  int rc = khb_addr_submit(c, centres, n_jobs, group_begin, group_count, search);
  if (rc) return rc;
  return khb_addr_collect(c, hits, cap, st);
}

}  // extern "C"
