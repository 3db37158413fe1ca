// libkhbsgs.so: -m minikeys (device/minikey.hpp; thread_process_minikeys, keyhunt.cpp:2338-2505).  Two kernels per
// launch on a stream of the mode's own:
//   k_mini_filter  the typo check of every candidate of the span (one SHA-256 block each); the offsets of the valid
//                  ones (1 in 256) are appended densely to a device queue, one atomic per wave and append
//   k_mini_keys    one lane per queued offset: the key (a second SHA-256 block), k*G over the window table,
//                  hash160 of the uncompressed key, the -m address bloom, and {offset, hash160} into the hit ring
// The second kernel reads the queue's length on the device, so the host does not wait between the two.  Neither queue
// loses an entry silently: the counters go on counting past the capacities and khb_mini_collect reports it.
#include "abi.hpp"
#include "device/minikey.hpp"

using namespace khbk;

namespace khbk {

struct MiniHitDev {
  uint32_t off;
  uint32_t h[5];
};

constexpr uint32_t kMiniParamBytes = 96;      // digits at 0..20, alphabet at 32..89
constexpr uint32_t kMiniAlphaAt = 32;
constexpr uint32_t kMiniRunMin = 64, kMiniRunMax = 4096;
constexpr uint32_t kMiniQueueMin = 1024;

struct MiniState {
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev_mid = nullptr, ev1 = nullptr;
  uint8_t* d_params = nullptr;
  uint8_t* h_params = nullptr;         // pinned
  uint32_t* d_cnt = nullptr;           // [0] valid, [1] bad keys, [2] bloom hits
  uint32_t* h_cnt = nullptr;           // pinned copy after the launch
  uint32_t* d_queue = nullptr;
  uint32_t queue_alloc = 0;            // entries of d_queue
  MiniHitDev* d_hits = nullptr;        // kAddrHitCap entries
  uint32_t launch_queue_cap = 0, launch_hit_cap = 0;
  uint64_t launch_count = 0;
};

struct MiniArgs {
  const uint8_t* params;
  uint64_t count;
  uint32_t run;
  uint32_t* queue;
  uint32_t queue_cap;
  uint32_t* cnt;
  const CPt* tab;
  uint32_t wbits;
  const uint8_t* bloom;
  BloomGeom geom;
  MiniHitDev* hits;
  uint32_t hit_cap;
};

}  // namespace khbk

namespace {

__device__ __forceinline__ void mini_load_alphabet(uint8_t* alpha, const uint8_t* __restrict__ params) {
  if (threadIdx.x < kMiniBase) alpha[threadIdx.x] = params[kMiniAlphaAt + threadIdx.x];
  __syncthreads();
}

// Lane L owns the candidates [L run, (L + 1) run) of the span, cut at count.  Every lane of a wave makes the same
// `run` steps (a lane past the end tests nothing), so the ballot of the append sees the whole wave.
__global__ __launch_bounds__(256) void k_mini_filter(MiniArgs A) {
  __shared__ uint8_t alpha[64];
  mini_load_alphabet(alpha, A.params);
  const uint64_t begin = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * A.run;
  uint8_t d[kMiniDigits];
#pragma unroll
  for (int i = 0; i < kMiniDigits; ++i) d[i] = A.params[i];
  mini_add(d, begin < A.count ? begin : 0);      // in range: the host checked first + count - 1
  uint32_t head[5];
  MiniPre pre;                                     // what the candidates of a 58^2 run share (device/minikey.hpp)
  mini_pack_head(head, alpha, d);
  mini_pre(pre, head, 0xB8u);
  uint32_t d19 = d[19], d20 = d[20], c20 = alpha[d19];
  for (uint32_t t = 0; t < A.run; ++t) {
    const uint64_t idx = begin + t;
    const uint32_t s0 = mini_sha_word0(pre, mini_w5_check(c20, alpha[d20]), 0xB8u);
    const bool ok = idx < A.count && (s0 >> 24) == 0;
    const uint64_t m = __ballot(ok);
    if (m) {                                       // wave-uniform
      const uint32_t leader = (uint32_t)__ffsll((unsigned long long)m) - 1u;
      uint32_t base = 0;
      if (__lane_id() == leader) base = atomicAdd(&A.cnt[0], (uint32_t)__popcll(m));
      base = __shfl(base, (int)leader);
      if (ok) {
        const uint32_t slot = base + lane_rank(m);
        if (slot < A.queue_cap) A.queue[slot] = (uint32_t)idx;
      }
    }
    if (++d20 == kMiniBase) {                      // every 58th step: character 20 changes
      d20 = 0;
      if (++d19 == kMiniBase) {                    // every 58^2-th: the carry runs into the head words
        d[19] = (uint8_t)(kMiniBase - 1);
        mini_carry(d, 19);                         // past 58^21 only in a lane past the end of the span
        mini_pack_head(head, alpha, d);
        mini_pre(pre, head, 0xB8u);
        d19 = 0;
      }
      c20 = alpha[d19];
    }
  }
}

// Grid-stride over the queue's entries; the length is what the filter counted, cut at the capacity.
__global__ __launch_bounds__(256) void k_mini_keys(MiniArgs A) {
  __shared__ uint8_t alpha[64];
  mini_load_alphabet(alpha, A.params);
  const uint32_t total = A.cnt[0];
  const uint32_t n = total < A.queue_cap ? total : A.queue_cap;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const uint32_t off = A.queue[i];
    uint8_t d[kMiniDigits];
#pragma unroll
    for (int k = 0; k < kMiniDigits; ++k) d[k] = A.params[k];
    mini_add(d, off);
    U8 key;
    mini_key(key, alpha, d);
    if (!mini_scalar_ok(key)) {                    // probability 2^-128: no public key, never a hit
      atomicAdd(&A.cnt[1], 1u);
      continue;
    }
    CPt P;
    mini_mul_g(P, key, A.tab, A.wbits);
    uint32_t h[5];
    hash160_uncompressed(h, P.x, P.y);
    if (bloom_check20(A.bloom, A.geom, h)) {
      const uint32_t slot = atomicAdd(&A.cnt[2], 1u);
      if (slot < A.hit_cap) {
        MiniHitDev r;
        r.off = off;
#pragma unroll
        for (int k = 0; k < 5; ++k) r.h[k] = h[k];
        A.hits[slot] = r;
      }
    }
  }
}

// khb_mini_pubkey: mini_scalar_ok and mini_mul_g on caller-supplied scalars.
__global__ __launch_bounds__(256) void k_mini_pubkey(const U8* __restrict__ k, const CPt* __restrict__ tab,
                                                     uint32_t wbits, CPt* __restrict__ out, uint8_t* __restrict__ bad,
                                                     uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const U8 key = k[i];
  CPt P;
  P.x = Fe{};
  P.y = Fe{};
  const bool ok = mini_scalar_ok(key);
  if (ok) mini_mul_g(P, key, tab, wbits);
  out[i] = P;
  bad[i] = ok ? 0 : 1;
}

int ensure_state(khb_ctx* c) {
  if (c->mini) return KHB_OK;
  MiniState* M = new (std::nothrow) MiniState();
  if (!M) return KHB_ENOMEM;
  c->mini = M;                         // khb_close frees whatever the steps below reached
  KHB_TRY(c, hipStreamCreateWithFlags(&M->stream, hipStreamNonBlocking));
  KHB_TRY(c, hipEventCreate(&M->ev0));
  KHB_TRY(c, hipEventCreate(&M->ev_mid));
  KHB_TRY(c, hipEventCreate(&M->ev1));
  KHB_TRY(c, hipMalloc(&M->d_params, kMiniParamBytes));
  KHB_TRY(c, hipHostMalloc((void**)&M->h_params, kMiniParamBytes, hipHostMallocDefault));
  KHB_TRY(c, hipMalloc(&M->d_cnt, 4 * sizeof(uint32_t)));
  KHB_TRY(c, hipHostMalloc((void**)&M->h_cnt, 4 * sizeof(uint32_t), hipHostMallocDefault));
  KHB_TRY(c, hipMalloc(&M->d_hits, sizeof(MiniHitDev) * kAddrHitCap));
  return KHB_OK;
}

bool state_ready(const khb_ctx* c) { return c->mini && c->mini->d_hits; }

int ensure_queue(khb_ctx* c, uint32_t entries) {
  MiniState& M = *c->mini;
  if (entries <= M.queue_alloc) return KHB_OK;
  hipFree(M.d_queue);
  M.d_queue = nullptr;
  M.queue_alloc = 0;
  KHB_TRY(c, hipMalloc(&M.d_queue, sizeof(uint32_t) * (size_t)entries));
  M.queue_alloc = entries;
  return KHB_OK;
}

bool digits_ok(const uint8_t* d) {
  for (int i = 0; i < kMiniDigits; ++i)
    if (d[i] >= kMiniBase) return false;
  return true;
}

bool alphabet_ok(const uint8_t* a) {
  bool seen[256] = {};
  for (uint32_t i = 0; i < kMiniBase; ++i) {
    if (seen[a[i]]) return false;
    seen[a[i]] = true;
  }
  return true;
}

// The span's arguments: digits below 58, 58 distinct alphabet bytes, 1 <= count <= 2^32 (the queues hold 32-bit
// offsets) and first + count <= 58^21.
int span_ok(const uint8_t* first, uint64_t count, const uint8_t* alphabet) {
  if (!first || !alphabet || count == 0 || count > (1ull << 32)) return KHB_EINVAL;
  if (!digits_ok(first) || !alphabet_ok(alphabet)) return KHB_EINVAL;
  uint8_t d[kMiniDigits];
  memcpy(d, first, kMiniDigits);
  return mini_add(d, count - 1) ? KHB_OK : KHB_EINVAL;
}

uint32_t filter_run(const khb_ctx* c, uint64_t count) {
  const uint64_t lanes = 4ull * c->lanes;
  uint64_t run = (count + lanes - 1) / lanes;
  if (run < kMiniRunMin) run = kMiniRunMin;
  if (run > kMiniRunMax) run = kMiniRunMax;
  return (uint32_t)run;
}

uint32_t filter_blocks(uint64_t count, uint32_t run) {
  const uint64_t lanes = (count + run - 1) / run;
  return (uint32_t)((lanes + 255) / 256);
}

void fill_params(MiniState& M, const uint8_t* first, const uint8_t* alphabet) {
  memset(M.h_params, 0, kMiniParamBytes);
  memcpy(M.h_params, first, kMiniDigits);
  memcpy(M.h_params + kMiniAlphaAt, alphabet, kMiniBase);
}

}  // namespace

namespace khbk {

void mini_free(khb_ctx* c) {
  if (MiniState* M = c->mini) {
    if (M->stream) hipStreamSynchronize(M->stream);
    hipFree(M->d_params);
    if (M->h_params) hipHostFree(M->h_params);
    hipFree(M->d_cnt);
    if (M->h_cnt) hipHostFree(M->h_cnt);
    hipFree(M->d_queue);
    hipFree(M->d_hits);
    if (M->ev0) hipEventDestroy(M->ev0);
    if (M->ev_mid) hipEventDestroy(M->ev_mid);
    if (M->ev1) hipEventDestroy(M->ev1);
    if (M->stream) hipStreamDestroy(M->stream);
    delete M;
    c->mini = nullptr;
  }
  hipFree(c->d_mini_tab);
  c->d_mini_tab = nullptr;
}

}  // namespace khbk

extern "C" {

int khb_load_mini_table(khb_ctx* c, const uint8_t* points_xy_be, uint32_t window_bits) {
  if (!c || !points_xy_be || (window_bits != 4 && window_bits != 8 && window_bits != 16)) return KHB_EINVAL;
  if (c->queued || c->mini_busy) return KHB_EBUSY;
  KHB_TRY(c, hipSetDevice(c->device));
  const size_t n = mini_table_points(window_bits);
  std::vector<CPt> h;
  if (!host_alloc(h, n)) return KHB_ENOMEM;
  for (size_t i = 0; i < n; ++i) {
    fe_from_be(h[i].x, points_xy_be + 64 * i);
    fe_from_be(h[i].y, points_xy_be + 64 * i + 32);
  }
  CPt* d = nullptr;
  KHB_TRY(c, hipMalloc(&d, sizeof(CPt) * n));
  if (const hipError_t e = hipMemcpy(d, h.data(), sizeof(CPt) * n, hipMemcpyHostToDevice)) {
    hipFree(d);
    return hip_fail(c, e);
  }
  hipFree(c->d_mini_tab);
  c->d_mini_tab = d;
  c->mini_w = window_bits;
  return KHB_OK;
}

int khb_mini_set_queue_capacity(khb_ctx* c, uint32_t cap) {
  if (!c) return KHB_EINVAL;
  if (c->mini_busy) return KHB_EBUSY;
  c->mini_queue_cap = cap;
  return KHB_OK;
}

uint32_t khb_mini_queue_capacity(const khb_ctx* c, uint64_t count) {
  if (!c) return 0;
  if (c->mini_queue_cap) return c->mini_queue_cap;
  const uint64_t want = count / 64 + kMiniQueueMin;      // 4 x the expected count / 256, and room for a small span
  return (uint32_t)(want < 0xFFFFFFFFull ? want : 0xFFFFFFFFull);
}

int khb_mini_submit(khb_ctx* c, const uint8_t* first_digits, uint64_t count, const uint8_t* alphabet) {
  if (!c) return KHB_EINVAL;
  if (const int rc = span_ok(first_digits, count, alphabet)) return rc;
  if (!c->d_mini_tab || !c->d_abloom) return KHB_ESTATE;
  if (c->queued || c->mini_busy) return KHB_EBUSY;
  KHB_TRY(c, hipSetDevice(c->device));
  if (const int rc = ensure_state(c)) return rc;
  if (!state_ready(c)) return KHB_ENOMEM;
  MiniState& M = *c->mini;
  const uint32_t qcap = khb_mini_queue_capacity(c, count);
  if (const int rc = ensure_queue(c, qcap)) return rc;
  fill_params(M, first_digits, alphabet);
  MiniArgs A{};
  A.params = M.d_params;
  A.count = count;
  A.run = filter_run(c, count);
  A.queue = M.d_queue;
  A.queue_cap = qcap;
  A.cnt = M.d_cnt;
  A.tab = c->d_mini_tab;
  A.wbits = c->mini_w;
  A.bloom = c->d_abloom;
  A.geom = c->ageom;
  A.hits = M.d_hits;
  A.hit_cap = khb_addr_hit_capacity(c);
  KHB_TRY(c, hipMemcpyAsync(M.d_params, M.h_params, kMiniParamBytes, hipMemcpyHostToDevice, M.stream));
  KHB_TRY(c, hipMemsetAsync(M.d_cnt, 0, 4 * sizeof(uint32_t), M.stream));
  KHB_TRY(c, hipEventRecord(M.ev0, M.stream));
  hipLaunchKernelGGL(k_mini_filter, dim3(filter_blocks(count, A.run)), dim3(256), 0, M.stream, A);
  KHB_TRY(c, hipGetLastError());
  KHB_TRY(c, hipEventRecord(M.ev_mid, M.stream));
  // one lane per queue entry up to a full residency; a launch with fewer survivors leaves the other lanes at once
  uint32_t kblocks = (qcap + 255) / 256;
  if (kblocks > c->lanes / 256) kblocks = c->lanes / 256;
  hipLaunchKernelGGL(k_mini_keys, dim3(kblocks), dim3(256), 0, M.stream, A);
  KHB_TRY(c, hipGetLastError());
  KHB_TRY(c, hipEventRecord(M.ev1, M.stream));
  KHB_TRY(c, hipMemcpyAsync(M.h_cnt, M.d_cnt, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, M.stream));
  M.launch_queue_cap = qcap;
  M.launch_hit_cap = A.hit_cap;
  M.launch_count = count;
  c->mini_busy = true;
  return KHB_OK;
}

int khb_mini_collect(khb_ctx* c, khb_mini_hit* hits, uint32_t cap, khb_mini_stats* st) {
  if (!c) return KHB_EINVAL;
  if (!c->mini_busy) return KHB_ESTATE;
  KHB_TRY(c, hipSetDevice(c->device));
  MiniState& M = *c->mini;
  c->mini_busy = false;
  KHB_TRY(c, hipStreamSynchronize(M.stream));
  const uint32_t valid = M.h_cnt[0], bad = M.h_cnt[1], nh = M.h_cnt[2];
  uint32_t take = nh < M.launch_hit_cap ? nh : M.launch_hit_cap;
  if (take > cap) take = cap;
  if (take && hits) {
    std::vector<MiniHitDev> h;
    if (!host_alloc(h, take)) return KHB_ENOMEM;
    KHB_TRY(c, hipMemcpy(h.data(), M.d_hits, sizeof(MiniHitDev) * take, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < take; ++i) {
      hits[i].offset = h[i].off;
      memcpy(hits[i].h160, h[i].h, 20);      // the words' little-endian bytes are the hash bytes
    }
  }
  if (st) {
    st->candidates = M.launch_count;
    st->valid = valid;
    st->bad_keys = bad;
    st->hits = nh;
    st->queue_overflow = valid > M.launch_queue_cap ? 1u : 0u;
    st->hit_overflow = nh > M.launch_hit_cap ? 1u : 0u;
    float a = -1.f, b = -1.f;
    if (hipEventElapsedTime(&a, M.ev0, M.ev_mid) != hipSuccess) a = -1.f;
    if (hipEventElapsedTime(&b, M.ev_mid, M.ev1) != hipSuccess) b = -1.f;
    st->filter_ms = a;
    st->keys_ms = b;
  }
  return KHB_OK;
}

int khb_mini_scan(khb_ctx* c, const uint8_t* first_digits, uint64_t count, const uint8_t* alphabet, khb_mini_hit* hits,
                  uint32_t cap, khb_mini_stats* st) {
  if (c && (c->queued || c->mini_busy)) return KHB_EBUSY;
  if (const int rc = khb_mini_submit(c, first_digits, count, alphabet)) return rc;
  return khb_mini_collect(c, hits, cap, st);
}

int khb_mini_filter(khb_ctx* c, const uint8_t* first_digits, uint64_t count, const uint8_t* alphabet,
                    uint64_t* offsets_out, uint32_t cap, uint64_t* n_out) {
  if (!c || !n_out || (cap && !offsets_out)) return KHB_EINVAL;
  if (const int rc = span_ok(first_digits, count, alphabet)) return rc;
  if (c->queued || c->mini_busy) return KHB_EBUSY;
  KHB_TRY(c, hipSetDevice(c->device));
  if (const int rc = ensure_state(c)) return rc;
  if (!state_ready(c)) return KHB_ENOMEM;
  MiniState& M = *c->mini;
  const uint32_t qcap = cap ? cap : 1;
  if (const int rc = ensure_queue(c, qcap)) return rc;
  fill_params(M, first_digits, alphabet);
  MiniArgs A{};
  A.params = M.d_params;
  A.count = count;
  A.run = filter_run(c, count);
  A.queue = M.d_queue;
  A.queue_cap = cap;
  A.cnt = M.d_cnt;
  KHB_TRY(c, hipMemcpyAsync(M.d_params, M.h_params, kMiniParamBytes, hipMemcpyHostToDevice, M.stream));
  KHB_TRY(c, hipMemsetAsync(M.d_cnt, 0, 4 * sizeof(uint32_t), M.stream));
  hipLaunchKernelGGL(k_mini_filter, dim3(filter_blocks(count, A.run)), dim3(256), 0, M.stream, A);
  if (const int rc = sync_launch(c, M.stream)) return rc;
  uint32_t n = 0;
  KHB_TRY(c, hipMemcpy(&n, M.d_cnt, sizeof n, hipMemcpyDeviceToHost));
  *n_out = n;
  const uint32_t take = n < cap ? n : cap;
  if (take) {
    std::vector<uint32_t> h;
    if (!host_alloc(h, take)) return KHB_ENOMEM;
    KHB_TRY(c, hipMemcpy(h.data(), M.d_queue, sizeof(uint32_t) * take, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < take; ++i) offsets_out[i] = h[i];
  }
  return KHB_OK;
}

int khb_mini_pubkey(khb_ctx* c, const uint8_t* scalars_be, uint8_t* xy_out, uint8_t* flags_out, uint32_t n) {
  if (!c || !scalars_be || !xy_out || !flags_out || n == 0) return KHB_EINVAL;
  if (!c->d_mini_tab) return KHB_ESTATE;
  if (c->mini_busy) return KHB_EBUSY;
  KHB_TRY(c, hipSetDevice(c->device));
  Slot& S = c->slot[0];
  std::vector<U8> hk;
  std::vector<CPt> hp;
  if (!host_alloc(hk, n) || !host_alloc(hp, n)) return KHB_ENOMEM;
  for (uint32_t i = 0; i < n; ++i) {
    Fe f;
    fe_from_be(f, scalars_be + 32 * (size_t)i);      // the same limb order as U8
    memcpy(hk[i].v, f.v, sizeof f.v);
  }
  DevBuf<U8> dk;
  DevBuf<CPt> dp;
  DevBuf<uint8_t> db;
  KHB_TRY(c, dk.alloc(n));
  KHB_TRY(c, dp.alloc(n));
  KHB_TRY(c, db.alloc(n));
  KHB_TRY(c, hipMemcpy(dk, hk.data(), sizeof(U8) * n, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_mini_pubkey, dim3((n + 255) / 256), dim3(256), 0, S.stream, dk.p, c->d_mini_tab, c->mini_w,
                     dp.p, db.p, n);
  if (const int rc = sync_launch(c, S.stream)) return rc;
  KHB_TRY(c, hipMemcpy(hp.data(), dp, sizeof(CPt) * n, hipMemcpyDeviceToHost));
  KHB_TRY(c, hipMemcpy(flags_out, db, n, hipMemcpyDeviceToHost));
  for (uint32_t i = 0; i < n; ++i) {
    fe_to_be(xy_out + 64 * (size_t)i, hp[i].x);
    fe_to_be(xy_out + 64 * (size_t)i + 32, hp[i].y);
  }
  return KHB_OK;
}

}  // extern "C"
