// libkhbsgs.so: the tables a context scans against.  Loads from the host (blooms, level-0 gate, giant table, lane
// offsets), the gate's derived stages, the baby-step builds on the device (khb_build_baby to the host,
// khb_build_l1_resident in place, launching k_giant_scan<kBaby> of k_baby.hip) and the calls that inspect what
// is installed (khb_resident_*, khb_gate_probe).
#include "abi.hpp"

using namespace khbk;

namespace {

// ---- the stages derived from a gate on the device (build_gate_stages_device)
// One probe: every block's hi word set, so the kernels' fixed three-probe test (device/bloom_probe.hpp
// gate_block_pass: probe 1 reads hi, probe 2 repeats probe 0) gives the one-probe answer.
__global__ void k_gate_hifill(uint2* __restrict__ gate, uint64_t nb) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < nb; j += stride) gate[j].y = 0xFFFFFFFFu;
}

// Stage-1 fold: thread i owns fold block i = OR of the gate's blocks i, i + nb1, ... (coalesced, no atomics).
// A superset of the gate: no member is ever dropped.
__global__ void k_gate_fold(const uint2* __restrict__ gate, uint64_t nb, uint2* __restrict__ fold, uint32_t nb1) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nb1) return;
  uint2 f = make_uint2(0u, 0u);
  for (uint64_t j = i; j < nb; j += nb1) {
    const uint2 g = gate[j];
    f.x |= g.x;
    f.y |= g.y;
  }
  fold[i] = f;
}

// Stage-0 filter: word i = OR of the hi words (probe 1's bit of every member) of the gate's blocks j with
// j mod nw0 == i.  nw0 divides the fold's block count, so those are the hi words of the fold's blocks i, i + nw0, ...
__global__ void k_gate_stage0(const uint2* __restrict__ fold, uint32_t nb1, uint32_t* __restrict__ z, uint32_t nw0) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nw0) return;
  uint32_t v = 0;
  for (uint32_t j = i; j < nb1; j += nw0) v |= fold[j].y;
  z[i] = v;
}

// Bits set in n_words 32-bit words (grid-stride; one atomic per block).
__global__ void k_popcount(const uint32_t* __restrict__ w, uint64_t n_words, unsigned long long* __restrict__ total) {
  __shared__ unsigned long long part[256 / 64];
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  unsigned long long n = 0;
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n_words; j += stride) n += __popc(w[j]);
  for (int d = 32; d > 0; d >>= 1) n += __shfl_down(n, d, 64);
  if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (uint32_t k = 1; k < blockDim.x / 64; ++k) n += part[k];
    atomicAdd(total, n);
  }
}

// Gate self-test with the scan's own device functions: bit 0 = the full gate passes x, bit 1 = the stage-1 fold
// (1 when there is none), bit 2 = the stage-0 filter (1 when there is none).
__global__ void k_gate_probe(ScanArgs A, const Fe* __restrict__ xs, uint8_t* __restrict__ out, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Fe x = xs[i];
  const GateBits b = gate_bits(x.v[1], gate_s2(A));
  uint32_t r = gate_block_pass(gate_block(A.gate, A.gate_mask, x), b) ? 1u : 0u;
  r |= (!A.gate1 || gate_block_pass(gate_block(A.gate1, A.gate1_mask, x), b)) ? 2u : 0u;
  r |= (!A.gate0 || (int32_t)shl_mod32(A.gate0[x.v[0] & A.gate0_mask], b.a1) < 0) ? 4u : 0u;
  out[i] = (uint8_t)r;
}

// No gate installed: the gate, its fold and stage 0 freed, their masks and sizes zero.
void drop_gate(khb_ctx* c) {
  hipFree(c->d_gate);
  hipFree(c->d_gate1);
  hipFree(c->d_gate0);
  c->d_gate = c->d_gate1 = nullptr;
  c->d_gate0 = nullptr;
  c->gate_mask = c->gate1_mask = c->gate0_mask = 0;
  c->gate_bytes = 0;
  c->gate_probes = 0;
}

// No bloom installed in (d, g): a geometry is only ever set together with a fully written buffer.
void drop_bloom(uint8_t*& d, BloomGeom& g) {
  hipFree(d);
  d = nullptr;
  g = BloomGeom{};
}

// Neither a level-1 bloom nor a gate installed.
void drop_tables(khb_ctx* c) {
  drop_bloom(c->d_bloom, c->geom);
  drop_gate(c);
}

// A device copy of `bytes` host bytes in a new allocation at dst.
template <class T>
int upload(khb_ctx* c, T*& dst, const void* src, size_t bytes) {
  KHB_TRY(c, hipMalloc(&dst, bytes));
  KHB_TRY(c, hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
  return KHB_OK;
}

// khb_load_bloom / khb_load_addr_bloom: (d, g) is replaced by the caller's bloom, or left empty on failure.
int load_bloom(khb_ctx* c, uint8_t*& d, BloomGeom& g, const uint8_t* bf, uint64_t bytes_per_sub, size_t total,
               uint64_t bits, uint32_t hashes) {
  if (!bf || !bloom_args_ok(bytes_per_sub, bits, hashes)) return KHB_EINVAL;
  if (c->queued || c->mini_busy) return KHB_EBUSY;
  KHB_TRY(c, hipSetDevice(c->device));
  drop_bloom(d, g);
  if (const int rc = upload(c, d, bf, total)) {
    drop_bloom(d, g);
    return rc;
  }
  g = bloom_geom(bytes_per_sub, bits, hashes);
  return KHB_OK;
}

// The sizes (log2 bytes, 0 = none) of the stage-1 fold of a gate of `bytes` bytes and of the stage-0 filter in front
// of a fold of 2^f_log2 bytes, as set by khb_set_gate_stage1 / khb_set_gate_stage0.
// KHB_GATE_STAGE1_AUTO: an L2-sized 2 MiB fold of a gate of up to 32 MiB (k = 1: -8.6 % time with two
// launches in flight, profiles/r04k/stage1_k1_nt_pipe_ab.txt; 4 MiB equal on the half-stream product, r06d), a
// 32 MiB fold of a larger one (k = 4: the 128 MiB gate beside the 57.5 MiB L1 bloom).  Round 4 (full prefix stream)
// had measured 16 MiB 3.5 % faster than 32 MiB (profiles/r04l/k4_stage1_ab.txt); with the half prefix stream's
// halved MALL traffic 32 MiB is 1.3 % faster than 16 MiB and 0.8 % than 64 MiB (5 rounds each, profiles/r06e).
uint32_t fold_log2_for(const khb_ctx* c, uint64_t bytes) {
  return c->gate1_log2 != KHB_GATE_STAGE1_AUTO ? c->gate1_log2 : bytes <= (1u << 25) ? 21u : 25u;
}
// Stage 0 is off by default (KHB_GATE0).  KHB_GATE_STAGE0_AUTO puts a 2 MiB one-bit-per-member filter in front of a
// fold larger than 2 MiB (k >= 4, where the fold is read from the MALL for every x); none at k = 1, whose 2 MiB
// fold is itself L2-resident.
uint32_t stage0_log2_for(const khb_ctx* c, uint32_t f_log2) {
  return c->gate0_log2 != KHB_GATE_STAGE0_AUTO ? c->gate0_log2 : f_log2 > 21 ? 21u : 0u;
}

// The structures derived from a gate already on the device (c->d_gate, gate_bytes, gate_probes set; khb_load_gate
// and khb_build_l1_resident): the one-probe hi-word fill, the stage-1 fold and the stage-0 filter.  With one probe
// every hi word is set, so a stage-0 filter would pass everything: none.  On failure the caller drops the gate.
int build_gate_stages_device(khb_ctx* c, hipStream_t stream) {
  const uint64_t bytes = c->gate_bytes, nb = bytes / 8;
  const uint32_t fill_blocks = (uint32_t)(nb / 256 < 65536 ? (nb + 255) / 256 : 65536);
  if (c->gate_probes == 1) {
    hipLaunchKernelGGL(k_gate_hifill, dim3(fill_blocks), dim3(256), 0, stream, (uint2*)c->d_gate, nb);
    KHB_TRY(c, hipGetLastError());
  }
  const uint32_t f_log2 = fold_log2_for(c, bytes);
  if (f_log2 && (1ull << f_log2) < bytes) {
    const uint32_t nb1 = (uint32_t)((1ull << f_log2) / 8);
    KHB_TRY(c, hipMalloc(&c->d_gate1, (size_t)nb1 * 8));
    hipLaunchKernelGGL(k_gate_fold, dim3((nb1 + 255) / 256), dim3(256), 0, stream, (const uint2*)c->d_gate, nb,
                       (uint2*)c->d_gate1, nb1);
    KHB_TRY(c, hipGetLastError());
    c->gate1_mask = nb1 - 1;
    const uint32_t z_log2 = stage0_log2_for(c, f_log2);
    if (z_log2 && c->gate_probes >= 2 && (1ull << z_log2) < (uint64_t)nb1 * 8) {
      const uint32_t nw0 = (uint32_t)((1ull << z_log2) / 4);
      KHB_TRY(c, hipMalloc(&c->d_gate0, (size_t)nw0 * 4));
      hipLaunchKernelGGL(k_gate_stage0, dim3((nw0 + 255) / 256), dim3(256), 0, stream, (const uint2*)c->d_gate1, nb1,
                         c->d_gate0, nw0);
      KHB_TRY(c, hipGetLastError());
      c->gate0_mask = nw0 - 1;
    }
  }
  KHB_TRY(c, hipStreamSynchronize(stream));
  return KHB_OK;
}

// The baby walk of khb_build_baby / khb_build_l1_resident on slot 0 (its centres in S.h_centres, A filled by the
// caller): the launch, its time in *kernel_ms, and KHB_EINCOMPLETE unless every group was walked.
int run_baby(khb_ctx* c, Slot& S, const ScanArgs& A, float* kernel_ms) {
  KHB_TRY(c, hipMemcpyAsync(S.d_centres, S.h_centres, sizeof(AffPt) * A.n_jobs, hipMemcpyHostToDevice, S.stream));
  S.counters_zero = false;
  KHB_TRY(c, hipMemsetAsync(S.d_counters, 0, kCounterBytes, S.stream));
  KHB_TRY(c, hipEventRecord(S.ev0, S.stream));
  if (const int rc = launch_scan(kBaby, c->lanes / kBlock, S.stream, A)) return rc;
  KHB_TRY(c, hipGetLastError());
  KHB_TRY(c, hipEventRecord(S.ev1, S.stream));
  KHB_TRY(c, hipStreamSynchronize(S.stream));
  KHB_TRY(c, hipMemcpy(S.h_counters, S.d_counters, kCounterBytes, hipMemcpyDeviceToHost));
  if (kernel_ms && hipEventElapsedTime(kernel_ms, S.ev0, S.ev1) != hipSuccess) *kernel_ms = -1.f;
  return walked_groups(S) == (uint64_t)A.n_jobs * (A.group_end - A.group_begin) ? KHB_OK : KHB_EINCOMPLETE;
}

// An installed table (khb_resident_read / khb_resident_popcount): its device address and size in bytes.
bool resident_table(const khb_ctx* c, int which, const uint8_t*& p, uint64_t& bytes) {
  switch (which) {
    case KHB_TABLE_L1: p = c->d_bloom; bytes = 256 * c->geom.bytes_per_sub; break;
    case KHB_TABLE_GATE: p = c->d_gate; bytes = c->gate_bytes; break;
    case KHB_TABLE_FOLD: p = c->d_gate1; bytes = ((uint64_t)c->gate1_mask + 1) * 8; break;
    case KHB_TABLE_STAGE0: p = (const uint8_t*)c->d_gate0; bytes = ((uint64_t)c->gate0_mask + 1) * 4; break;
    default: p = nullptr; bytes = 0; break;
  }
  if (!p) bytes = 0;
  return p != nullptr;
}

}  // namespace

extern "C" {

int khb_load_gate(khb_ctx* c, const uint8_t* gate, uint32_t log2_bits, uint32_t probes) {
  if (!c || (gate && !gate_args_ok(log2_bits, probes, 32))) return KHB_EINVAL;
  if (c->queued) return KHB_EBUSY;
  KHB_TRY(c, hipSetDevice(c->device));
  drop_gate(c);
  if (!gate) return KHB_OK;
  const uint64_t bytes = 1ull << (log2_bits - 3);
  int rc = upload(c, c->d_gate, gate, bytes);
  if (!rc) {
    c->gate_bytes = bytes;
    c->gate_mask = (uint32_t)((1ull << (log2_bits - 6)) - 1);
    c->gate_probes = probes;
    rc = build_gate_stages_device(c, c->slot[0].stream);
  }
  if (rc) drop_gate(c);
  return rc;
}

int khb_gate_stages(const khb_ctx* c) {
  if (!c) return KHB_EINVAL;
  return (c->d_gate ? 4 : 0) | (c->d_gate1 ? 2 : 0) | (c->d_gate0 ? 1 : 0);
}

int khb_set_gate_stage0(khb_ctx* c, uint32_t log2_bytes) {
  if (!c || (log2_bytes && log2_bytes != KHB_GATE_STAGE0_AUTO && (log2_bytes < 10 || log2_bytes > 30)))
    return KHB_EINVAL;
  if (c->queued) return KHB_EBUSY;
  c->gate0_log2 = log2_bytes;
  return KHB_OK;
}

int khb_set_gate_stage1(khb_ctx* c, uint32_t log2_bytes) {
  if (!c || (log2_bytes && log2_bytes != KHB_GATE_STAGE1_AUTO && (log2_bytes < 10 || log2_bytes > 31)))
    return KHB_EINVAL;
  if (c->queued) return KHB_EBUSY;
  c->gate1_log2 = log2_bytes;
  return KHB_OK;
}

int khb_load_bloom(khb_ctx* c, const uint8_t* bf, uint64_t bytes_per_sub, uint64_t bits_per_sub, uint32_t hashes) {
  if (!c) return KHB_EINVAL;
  return load_bloom(c, c->d_bloom, c->geom, bf, bytes_per_sub, (size_t)bytes_per_sub * 256, bits_per_sub, hashes);
}

int khb_load_addr_bloom(khb_ctx* c, const uint8_t* bf, uint64_t bytes, uint64_t bits, uint32_t hashes) {
  if (!c) return KHB_EINVAL;
  return load_bloom(c, c->d_abloom, c->ageom, bf, bytes, bytes, bits, hashes);
}

// The -m vanity interval table (device/vanity.hpp): one allocation of lo words, hi words and the bucket bitmap.
int khb_load_vanity(khb_ctx* c, const uint8_t* lo_be20, const uint8_t* hi_be20, uint32_t n) {
  if (!c || !lo_be20 || !hi_be20 || n == 0) return KHB_EINVAL;
  for (uint32_t i = 0; i < n; ++i) {
    if (memcmp(lo_be20 + 20 * (size_t)i, hi_be20 + 20 * (size_t)i, 20) > 0) return KHB_EINVAL;
    if (i + 1 < n && memcmp(hi_be20 + 20 * (size_t)i, lo_be20 + 20 * (size_t)(i + 1), 20) >= 0) return KHB_EINVAL;
  }
  if (c->queued) return KHB_EBUSY;
  KHB_TRY(c, hipSetDevice(c->device));
  std::vector<uint32_t> h;
  if (!host_alloc(h, 10 * (size_t)n + kVanityBitmapWords)) return KHB_ENOMEM;
  uint32_t* lo = h.data();
  uint32_t* hi = lo + 5 * (size_t)n;
  for (size_t k = 0; k < 5 * (size_t)n; ++k) {
    const uint8_t *a = lo_be20 + 4 * k, *b = hi_be20 + 4 * k;
    lo[k] = ((uint32_t)a[0] << 24) | ((uint32_t)a[1] << 16) | ((uint32_t)a[2] << 8) | a[3];
    hi[k] = ((uint32_t)b[0] << 24) | ((uint32_t)b[1] << 16) | ((uint32_t)b[2] << 8) | b[3];
  }
  vanity_build_bitmap(hi + 5 * (size_t)n, lo, hi, n);
  uint32_t* d = nullptr;
  KHB_TRY(c, hipMalloc(&d, sizeof(uint32_t) * h.size()));
  if (const hipError_t e = hipMemcpy(d, h.data(), sizeof(uint32_t) * h.size(), hipMemcpyHostToDevice)) {
    hipFree(d);
    return hip_fail(c, e);
  }
  hipFree(c->d_van);
  c->d_van = d;
  c->van_n = n;
  return KHB_OK;
}

int khb_load_giant_table(khb_ctx* c, const uint8_t* gsn) {
  if (!c || !gsn) return KHB_EINVAL;
  if (c->queued) return KHB_EBUSY;
  KHB_TRY(c, hipSetDevice(c->device));
  // 513 points, then p - x of each (the walk's negated table, GsnTable::nx)
  struct {
    AffPt pt[KHB_GIANT_TABLE];
    Fe nx[KHB_GIANT_TABLE];
  } h;
  pts_from_be(h.pt, gsn, KHB_GIANT_TABLE);
  const Fe zero{};
  for (int i = 0; i < KHB_GIANT_TABLE; ++i) fe_sub(h.nx[i], zero, h.pt[i].x);
  if (!c->d_gsn) KHB_TRY(c, hipMalloc(&c->d_gsn, sizeof(h)));
  KHB_TRY(c, hipMemcpy(c->d_gsn, &h, sizeof(h), hipMemcpyHostToDevice));
  c->gofs_stale = true;
  return KHB_OK;
}

int khb_load_lane_offsets(khb_ctx* c, const uint8_t* offs, uint32_t n, uint32_t gpl) {
  if (!c || !offs || n == 0 || gpl == 0) return KHB_EINVAL;
  if (c->queued) return KHB_EBUSY;
  KHB_TRY(c, hipSetDevice(c->device));
  std::vector<AffPt> h;
  if (!host_alloc(h, n)) return KHB_ENOMEM;
  pts_from_be(h.data(), offs, n);
  hipFree(c->d_offs);
  c->d_offs = nullptr;
  if (const int rc = upload(c, c->d_offs, h.data(), sizeof(AffPt) * n)) {
    hipFree(c->d_offs);                  // no offsets: a scan is refused (KHB_ESTATE) until a load succeeds
    c->d_offs = nullptr;
    return rc;
  }
  c->n_offs = n;
  c->gpl = gpl;
  c->gofs_stale = true;
  return KHB_OK;
}

int khb_build_baby(khb_ctx* c, const uint8_t* centres, uint32_t n_jobs, uint32_t groups_per_job, uint64_t l1ext,
                   uint64_t m2, uint64_t m3, const uint64_t bytes_per_sub[3], const uint64_t bits_per_sub[3],
                   const uint32_t hashes[3], uint8_t* l1, uint8_t* l2, uint8_t* l3, uint8_t* bp, uint8_t* gate,
                   uint32_t gate_log2, uint32_t gate_probes, float* kernel_ms) {
  int rc = check_scan_args(c, centres, n_jobs, 0, groups_per_job, false);
  if (rc) return rc;
  if (!bytes_per_sub || !bits_per_sub || !hashes) return KHB_EINVAL;
  if (gate && !gate_args_ok(gate_log2, gate_probes, 32)) return KHB_EINVAL;
  uint8_t* outs[3] = {l1, l2, l3};
  for (int l = 0; l < 3; ++l)
    if (outs[l] && !bloom_args_ok(bytes_per_sub[l], bits_per_sub[l], hashes[l])) return KHB_EINVAL;
  if (c->queued) return KHB_EBUSY;
  KHB_TRY(c, hipSetDevice(c->device));
  Slot& S = c->slot[0];
  if ((rc = ensure_centres(c, S, n_jobs))) return rc;
  pts_from_be(S.h_centres, centres, n_jobs);
  ScanArgs A = make_args(c, S, n_jobs, 0, groups_per_job);
  A.job_keys = (uint64_t)groups_per_job * KHB_GROUP;
  A.blimit[0] = l1 ? l1ext : 0;
  A.blimit[1] = l2 ? m2 : 0;
  A.blimit[2] = (l3 || bp) ? m3 : 0;
  DevBuf<uint32_t> dw[3], dbp, dgate;
  const uint64_t gate_bytes = gate ? (1ull << gate_log2) / 8 : 0;
  if (gate) {
    KHB_TRY(c, dgate.alloc(gate_bytes / 4));
    KHB_TRY(c, hipMemsetAsync(dgate, 0, gate_bytes, S.stream));
    A.gate_w = dgate;
    A.glimit = l1ext;
    A.gate_mask = (uint32_t)((1ull << (gate_log2 - 6)) - 1);
    A.gate_probes = gate_probes;
  }
  for (int l = 0; l < 3; ++l) {
    if (!outs[l]) continue;
    const uint64_t words = (bytes_per_sub[l] + 3) / 4;
    KHB_TRY(c, dw[l].alloc(256 * words));
    KHB_TRY(c, hipMemsetAsync(dw[l], 0, 256 * words * 4, S.stream));
    A.bw[l] = dw[l];
    A.bstride[l] = words * 32;           // word-aligned sub-blooms, repacked below
    A.bgeom[l] = bloom_geom(bytes_per_sub[l], bits_per_sub[l], hashes[l]);
  }
  if (bp && m3) {
    KHB_TRY(c, dbp.alloc(4 * m3));
    A.bp = dbp;
  }
  rc = run_baby(c, S, A, kernel_ms);
  if (rc && rc != KHB_EINCOMPLETE) return rc;        // a short walk still returns what it wrote
  std::vector<uint8_t> tmp;
  for (int l = 0; l < 3; ++l) {
    if (!outs[l]) continue;
    const uint64_t words = A.bstride[l] / 32, nb = bytes_per_sub[l];
    if (!host_alloc(tmp, 256 * words * 4)) return KHB_ENOMEM;
    KHB_TRY(c, hipMemcpy(tmp.data(), dw[l], 256 * words * 4, hipMemcpyDeviceToHost));
    for (int sub = 0; sub < 256; ++sub) memcpy(outs[l] + sub * nb, tmp.data() + sub * words * 4, nb);
  }
  if (dbp) KHB_TRY(c, hipMemcpy(bp, dbp, 16 * m3, hipMemcpyDeviceToHost));
  if (dgate) KHB_TRY(c, hipMemcpy(gate, dgate, gate_bytes, hipMemcpyDeviceToHost));
  return rc;
}

// ------------------------------------------------------------- resident level-1 bloom and gate
int khb_build_l1_resident(khb_ctx* c, const uint8_t* centres, uint32_t n_jobs, uint32_t groups_per_job,
                          uint64_t l1ext, uint64_t bytes_per_sub, uint64_t bits_per_sub, uint32_t hashes,
                          uint32_t gate_log2, uint32_t gate_probes, float* kernel_ms) {
  int rc = check_scan_args(c, centres, n_jobs, 0, groups_per_job, false);
  if (rc) return rc;
  if (l1ext == 0 || !bloom_args_ok(bytes_per_sub, bits_per_sub, hashes)) return KHB_EINVAL;
  if (gate_log2 && !gate_args_ok(gate_log2, gate_probes, 38)) return KHB_EINVAL;
  if (c->queued) return KHB_EBUSY;
  KHB_TRY(c, hipSetDevice(c->device));
  Slot& S = c->slot[0];
  if ((rc = ensure_centres(c, S, n_jobs))) return rc;
  pts_from_be(S.h_centres, centres, n_jobs);
  drop_tables(c);                        // a build replaces whatever is installed
  const uint64_t l1_bytes = 256 * bytes_per_sub, gate_bytes = gate_log2 ? 1ull << (gate_log2 - 3) : 0;
  auto build = [&]() -> int {
    KHB_TRY(c, hipMalloc(&c->d_bloom, l1_bytes));
    KHB_TRY(c, hipMemsetAsync(c->d_bloom, 0, l1_bytes, S.stream));
    if (gate_bytes) {
      KHB_TRY(c, hipMalloc(&c->d_gate, gate_bytes));
      KHB_TRY(c, hipMemsetAsync(c->d_gate, 0, gate_bytes, S.stream));
    }
    ScanArgs A = make_args(c, S, n_jobs, 0, groups_per_job);
    A.bloom = nullptr;                   // the walk only writes
    A.gate = nullptr;
    A.job_keys = (uint64_t)groups_per_job * KHB_GROUP;
    A.blimit[0] = l1ext;
    A.bw[0] = reinterpret_cast<uint32_t*>(c->d_bloom);
    A.bstride[0] = bytes_per_sub * 8;    // packed: the layout the probe reads, no repack
    A.bgeom[0] = bloom_geom(bytes_per_sub, bits_per_sub, hashes);
    if (gate_bytes) {
      A.gate_w = reinterpret_cast<uint32_t*>(c->d_gate);
      A.glimit = l1ext;
      A.gate_mask = (uint32_t)((1ull << (gate_log2 - 6)) - 1);
      A.gate_probes = gate_probes;
    }
    if (const int r = run_baby(c, S, A, kernel_ms)) return r;
    c->geom = A.bgeom[0];
    if (!gate_bytes) return KHB_OK;
    c->gate_bytes = gate_bytes;
    c->gate_mask = A.gate_mask;
    c->gate_probes = gate_probes;
    return build_gate_stages_device(c, S.stream);
  };
  if ((rc = build())) drop_tables(c);    // nothing half-built stays installed
  return rc;
}

int khb_resident_bytes(const khb_ctx* c, int which, uint64_t* bytes) {
  if (!c || !bytes || which < KHB_TABLE_L1 || which > KHB_TABLE_STAGE0) return KHB_EINVAL;
  const uint8_t* p;
  resident_table(c, which, p, *bytes);
  return KHB_OK;
}

int khb_resident_read(khb_ctx* c, int which, uint64_t offset, uint64_t bytes, uint8_t* out) {
  if (!c || which < KHB_TABLE_L1 || which > KHB_TABLE_STAGE0 || (bytes && !out)) return KHB_EINVAL;
  const uint8_t* p;
  uint64_t size;
  if (!resident_table(c, which, p, size)) return KHB_ESTATE;
  if (offset > size || bytes > size - offset) return KHB_EINVAL;
  if (c->queued) return KHB_EBUSY;
  KHB_TRY(c, hipSetDevice(c->device));
  if (bytes) KHB_TRY(c, hipMemcpy(out, p + offset, bytes, hipMemcpyDeviceToHost));
  return KHB_OK;
}

int khb_resident_popcount(khb_ctx* c, int which, uint64_t* bits_set) {
  if (!c || !bits_set || which < KHB_TABLE_L1 || which > KHB_TABLE_STAGE0) return KHB_EINVAL;
  const uint8_t* p;
  uint64_t size;
  if (!resident_table(c, which, p, size)) return KHB_ESTATE;
  if (c->queued) return KHB_EBUSY;
  KHB_TRY(c, hipSetDevice(c->device));
  Slot& S = c->slot[0];
  DevBuf<unsigned long long> d;
  KHB_TRY(c, d.alloc(1));
  KHB_TRY(c, hipMemsetAsync(d, 0, sizeof(unsigned long long), S.stream));
  const uint64_t words = size / 4;       // every table is a whole number of 32-bit words
  const uint32_t blocks = (uint32_t)(words / 256 < 16384 ? (words + 255) / 256 : 16384);
  hipLaunchKernelGGL(k_popcount, dim3(blocks), dim3(256), 0, S.stream, (const uint32_t*)p, words, d);
  if (const int rc = sync_launch(c, S.stream)) return rc;
  unsigned long long v = 0;
  KHB_TRY(c, hipMemcpy(&v, d, sizeof v, hipMemcpyDeviceToHost));
  *bits_set = v;
  return KHB_OK;
}

int khb_gate_probe(khb_ctx* c, const uint8_t* xs, uint8_t* out, uint32_t n) {
  if (!c || !xs || !out || n == 0) return KHB_EINVAL;
  if (!c->d_gate) return KHB_ESTATE;
  if (c->queued) return KHB_EBUSY;
  KHB_TRY(c, hipSetDevice(c->device));
  Slot& S = c->slot[0];
  std::vector<Fe> h;
  if (!host_alloc(h, n)) return KHB_ENOMEM;
  fes_from_be(h.data(), xs, n);
  DevBuf<Fe> d;
  DevBuf<uint8_t> dout;
  KHB_TRY(c, d.alloc(n));
  KHB_TRY(c, dout.alloc(n));
  KHB_TRY(c, hipMemcpy(d, h.data(), sizeof(Fe) * n, hipMemcpyHostToDevice));
  ScanArgs A{};
  A.gate = c->d_gate;
  A.gate_mask = c->gate_mask;
  A.gate_probes = c->gate_probes;
  A.gate1 = c->d_gate1;
  A.gate1_mask = c->gate1_mask;
  A.gate0 = c->d_gate0;
  A.gate0_mask = c->gate0_mask;
  hipLaunchKernelGGL(k_gate_probe, dim3((n + 255) / 256), dim3(256), 0, S.stream, A, (const Fe*)d.p, dout, n);
  if (const int rc = sync_launch(c, S.stream)) return rc;
  KHB_TRY(c, hipMemcpy(out, dout, n, hipMemcpyDeviceToHost));
  return KHB_OK;
}

}  // extern "C"
