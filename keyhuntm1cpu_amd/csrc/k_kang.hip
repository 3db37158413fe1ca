// libkhbsgs.so: Pollard's kangaroo walk with distinguished points (device/kangaroo.hpp).  The herd's
// state lives on the device from launch to launch, so a launch is one kernel on a stream of the mode's own:
//   k_kang_walk     every lane steps its KHB_KANG_PER_LANE kangaroos `steps` times, one field inversion per step and
//                   lane, and appends the distinguished points to the launch's ring
//   k_kang_scatter  khb_kang_store: packed {x, y, d} records into the [slot][lane] state
//   k_kang_gather   khb_kang_read: the reverse
// Two rings alternate, so the host digests one launch's points while the next launch runs; launches, stores and reads
// of a context are ordered on its one stream.  The ring's counter goes on counting past the capacity and
// khb_kang_collect reports it.
#include "abi.hpp"
#include "device/kangaroo.hpp"

using namespace khbk;

namespace khbk {

struct KangRec {       // one kangaroo as store and read move it
  Fe x, y, d;
};

struct KangLaunch {
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  KangDpDev* d_ring = nullptr;
  uint32_t ring_alloc = 0;
  unsigned long long* d_cnt = nullptr;       // 4 counters
  unsigned long long* h_cnt = nullptr;       // pinned copy after the launch
  uint32_t cap = 0;                          // of the launch in flight
  uint64_t expect = 0;                       // herd x steps
};

struct KangState {
  hipStream_t stream = nullptr;
  uint32_t* d_jumps = nullptr;
  bool jumps = false;
  Fe *d_x = nullptr, *d_y = nullptr, *d_d = nullptr, *d_scr = nullptr;
  uint32_t stride = 0;                       // lanes allocated
  uint32_t herd = 0;
  uint32_t ring_cap = kKangRingDefault;
  KangLaunch L[2];
  uint32_t head = 0, queued = 0;             // launches in flight, oldest first: L[head & 1], L[(head + 1) & 1]
};

}  // namespace khbk

namespace {

__global__ __launch_bounds__(256, KHB_KANG_WAVES_PER_SIMD) void k_kang_walk(KangArgs A) {
  __shared__ KangJumpLds jt;
  for (uint32_t w = threadIdx.x; w < kKangJumpWords * kKangJumps; w += blockDim.x) (&jt[0][0])[w] = A.jumps[w];
  __syncthreads();
  const uint32_t lane = blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t first = (uint64_t)lane * kKangPerLane;
  if (lane >= A.stride || first >= A.n) return;
  const uint32_t left = A.n - (uint32_t)first;
  const uint32_t m = left < kKangPerLane ? left : kKangPerLane;
  uint32_t seconds = 0;
  for (uint32_t t = 0; t < A.steps; ++t) kang_step(A, jt, lane, m, seconds);
  atomicAdd(&A.cnt[1], (unsigned long long)m * A.steps);
  if (seconds) atomicAdd(&A.cnt[2], (unsigned long long)seconds);
}

// Kangaroo first + i of the herd <-> rec[i]; the caller checked first + n against the state's capacity.
__global__ __launch_bounds__(256) void k_kang_scatter(Fe* __restrict__ x, Fe* __restrict__ y, Fe* __restrict__ d,
                                                      uint32_t stride, const KangRec* __restrict__ rec, uint32_t first,
                                                      uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t k = first + i;
  const size_t at = (size_t)(k % kKangPerLane) * stride + k / kKangPerLane;
  x[at] = rec[i].x;
  y[at] = rec[i].y;
  d[at] = rec[i].d;
}

__global__ __launch_bounds__(256) void k_kang_gather(const Fe* __restrict__ x, const Fe* __restrict__ y,
                                                     const Fe* __restrict__ d, uint32_t stride,
                                                     KangRec* __restrict__ rec, uint32_t first, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t k = first + i;
  const size_t at = (size_t)(k % kKangPerLane) * stride + k / kKangPerLane;
  rec[i].x = x[at];
  rec[i].y = y[at];
  rec[i].d = d[at];
}

int ensure_state(khb_ctx* c) {
  if (c->kang) return KHB_OK;
  KangState* K = new (std::nothrow) KangState();
  if (!K) return KHB_ENOMEM;
  c->kang = K;                         // khb_close frees whatever the steps below reached
  KHB_TRY(c, hipStreamCreateWithFlags(&K->stream, hipStreamNonBlocking));
  KHB_TRY(c, hipMalloc(&K->d_jumps, sizeof(uint32_t) * kKangJumpWords * kKangJumps));
  for (KangLaunch& L : K->L) {
    KHB_TRY(c, hipEventCreate(&L.ev0));
    KHB_TRY(c, hipEventCreate(&L.ev1));
    KHB_TRY(c, hipMalloc(&L.d_cnt, 4 * sizeof(unsigned long long)));
    KHB_TRY(c, hipHostMalloc((void**)&L.h_cnt, 4 * sizeof(unsigned long long), hipHostMallocDefault));
  }
  return KHB_OK;
}

bool state_ready(const khb_ctx* c) { return c->kang && c->kang->L[1].h_cnt; }

void free_herd(KangState& K) {
  hipFree(K.d_x);
  hipFree(K.d_y);
  hipFree(K.d_d);
  hipFree(K.d_scr);
  K.d_x = K.d_y = K.d_d = K.d_scr = nullptr;
  K.stride = K.herd = 0;
}

// The state grown to hold `herd` kangaroos (lanes in whole blocks); the kangaroos already stored keep their places.
int ensure_herd(khb_ctx* c, uint32_t herd) {
  KangState& K = *c->kang;
  const uint32_t lanes = ((herd + kKangPerLane - 1) / kKangPerLane + kBlock - 1) / kBlock * kBlock;
  if (lanes <= K.stride) return KHB_OK;
  const size_t n = (size_t)lanes * kKangPerLane;
  Fe *x = nullptr, *y = nullptr, *d = nullptr, *s = nullptr;
  hipError_t e = hipMalloc(&x, sizeof(Fe) * n);
  if (e == hipSuccess) e = hipMalloc(&y, sizeof(Fe) * n);
  if (e == hipSuccess) e = hipMalloc(&d, sizeof(Fe) * n);
  if (e == hipSuccess) e = hipMalloc(&s, sizeof(Fe) * n);
  if (e == hipSuccess && K.herd) {         // slot s of the old lanes moves to slot s of the wider stride
    for (uint32_t slot = 0; slot < kKangPerLane && e == hipSuccess; ++slot) {
      const size_t from = (size_t)slot * K.stride, to = (size_t)slot * lanes, bytes = sizeof(Fe) * K.stride;
      e = hipMemcpy(x + to, K.d_x + from, bytes, hipMemcpyDeviceToDevice);
      if (e == hipSuccess) e = hipMemcpy(y + to, K.d_y + from, bytes, hipMemcpyDeviceToDevice);
      if (e == hipSuccess) e = hipMemcpy(d + to, K.d_d + from, bytes, hipMemcpyDeviceToDevice);
    }
  }
  if (e != hipSuccess) {
    hipFree(x);
    hipFree(y);
    hipFree(d);
    hipFree(s);
    return hip_fail(c, e);
  }
  const uint32_t keep = K.herd;
  free_herd(K);
  K.d_x = x;
  K.d_y = y;
  K.d_d = d;
  K.d_scr = s;
  K.stride = lanes;
  K.herd = keep;
  return KHB_OK;
}

int ensure_ring(khb_ctx* c, KangLaunch& L, uint32_t entries) {
  if (entries <= L.ring_alloc) return KHB_OK;
  hipFree(L.d_ring);
  L.d_ring = nullptr;
  L.ring_alloc = 0;
  KHB_TRY(c, hipMalloc(&L.d_ring, sizeof(KangDpDev) * (size_t)entries));
  L.ring_alloc = entries;
  return KHB_OK;
}

}  // namespace

namespace khbk {

void kang_free(khb_ctx* c) {
  KangState* K = c->kang;
  if (!K) return;
  if (K->stream) hipStreamSynchronize(K->stream);
  free_herd(*K);
  hipFree(K->d_jumps);
  for (KangLaunch& L : K->L) {
    hipFree(L.d_ring);
    hipFree(L.d_cnt);
    if (L.h_cnt) hipHostFree(L.h_cnt);
    if (L.ev0) hipEventDestroy(L.ev0);
    if (L.ev1) hipEventDestroy(L.ev1);
  }
  if (K->stream) hipStreamDestroy(K->stream);
  delete K;
  c->kang = nullptr;
}

}  // namespace khbk

extern "C" {

uint32_t khb_kang_per_lane(void) { return kKangPerLane; }

uint32_t khb_kang_full_herd(int device) {
  const uint32_t scan_lanes = khb_default_lanes(device);
  return scan_lanes / KHB_WAVES_PER_SIMD * KHB_KANG_WAVES_PER_SIMD * kKangPerLane;
}

int khb_kang_load_jumps(khb_ctx* c, const uint8_t* dist_be, const uint8_t* xy_be) {
  if (!c || !dist_be || !xy_be) return KHB_EINVAL;
  uint32_t h[kKangJumpWords * kKangJumps];
  Fe xs[kKangJumps];
  for (uint32_t j = 0; j < kKangJumps; ++j) {
    Fe y, s;
    fe_from_be(xs[j], xy_be + 64 * j);
    fe_from_be(y, xy_be + 64 * j + 32);
    fe_from_be(s, dist_be + 32 * j);
    for (uint32_t i = 0; i < j; ++i)
      if (fe_eq(xs[i], xs[j])) return KHB_EINVAL;      // the second choice of the step rule needs distinct x
    for (uint32_t k = 0; k < 8; ++k) {
      h[(k)*kKangJumps + j] = xs[j].v[k];
      h[(8 + k) * kKangJumps + j] = y.v[k];
      h[(16 + k) * kKangJumps + j] = s.v[k];
    }
  }
  KHB_TRY(c, hipSetDevice(c->device));
  if (const int rc = ensure_state(c)) return rc;
  if (!state_ready(c)) return KHB_ENOMEM;
  KangState& K = *c->kang;
  KHB_TRY(c, hipStreamSynchronize(K.stream));          // a launch in flight reads the table
  KHB_TRY(c, hipMemcpy(K.d_jumps, h, sizeof h, hipMemcpyHostToDevice));
  K.jumps = true;
  return KHB_OK;
}

int khb_kang_store(khb_ctx* c, uint32_t first, uint32_t n, const uint8_t* xy_be, const uint8_t* dist_be) {
  if (!c) return KHB_EINVAL;
  KHB_TRY(c, hipSetDevice(c->device));
  if (const int rc = ensure_state(c)) return rc;
  if (!state_ready(c)) return KHB_ENOMEM;
  KangState& K = *c->kang;
  if (n == 0) {                                        // forget the herd
    if (first) return KHB_EINVAL;
    KHB_TRY(c, hipStreamSynchronize(K.stream));
    K.herd = 0;
    return KHB_OK;
  }
  if (!xy_be || !dist_be || first > K.herd || (uint64_t)first + n > 0xFFFFFFFFull / 2) return KHB_EINVAL;
  KHB_TRY(c, hipStreamSynchronize(K.stream));          // behind the launches in flight, which read and write the state
  if (const int rc = ensure_herd(c, first + n)) return rc;
  std::vector<KangRec> h;
  if (!host_alloc(h, n)) return KHB_ENOMEM;
  for (uint32_t i = 0; i < n; ++i) {
    fe_from_be(h[i].x, xy_be + 64 * (size_t)i);
    fe_from_be(h[i].y, xy_be + 64 * (size_t)i + 32);
    fe_from_be(h[i].d, dist_be + 32 * (size_t)i);
  }
  DevBuf<KangRec> d;
  KHB_TRY(c, d.alloc(n));
  KHB_TRY(c, hipMemcpy(d, h.data(), sizeof(KangRec) * n, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_kang_scatter, dim3((n + 255) / 256), dim3(256), 0, K.stream, K.d_x, K.d_y, K.d_d, K.stride,
                     d.p, first, n);
  if (const int rc = sync_launch(c, K.stream)) return rc;
  if (first + n > K.herd) K.herd = first + n;
  return KHB_OK;
}

int khb_kang_read(khb_ctx* c, uint32_t first, uint32_t n, uint8_t* xy_be, uint8_t* dist_be) {
  if (!c || !xy_be || !dist_be || n == 0) return KHB_EINVAL;
  if (!c->kang || (uint64_t)first + n > c->kang->herd) return KHB_EINVAL;
  KHB_TRY(c, hipSetDevice(c->device));
  KangState& K = *c->kang;
  std::vector<KangRec> h;
  if (!host_alloc(h, n)) return KHB_ENOMEM;
  DevBuf<KangRec> d;
  KHB_TRY(c, d.alloc(n));
  hipLaunchKernelGGL(k_kang_gather, dim3((n + 255) / 256), dim3(256), 0, K.stream, K.d_x, K.d_y, K.d_d, K.stride,
                     d.p, first, n);
  if (const int rc = sync_launch(c, K.stream)) return rc;
  KHB_TRY(c, hipMemcpy(h.data(), d, sizeof(KangRec) * n, hipMemcpyDeviceToHost));
  for (uint32_t i = 0; i < n; ++i) {
    fe_to_be(xy_be + 64 * (size_t)i, h[i].x);
    fe_to_be(xy_be + 64 * (size_t)i + 32, h[i].y);
    fe_to_be(dist_be + 32 * (size_t)i, h[i].d);
  }
  return KHB_OK;
}

uint32_t khb_kang_herd(const khb_ctx* c) { return c && c->kang ? c->kang->herd : 0; }

int khb_kang_set_ring_capacity(khb_ctx* c, uint32_t cap) {
  if (!c || cap == 0) return KHB_EINVAL;
  KHB_TRY(c, hipSetDevice(c->device));
  if (const int rc = ensure_state(c)) return rc;
  if (!state_ready(c)) return KHB_ENOMEM;
  c->kang->ring_cap = cap;                             // of later launches
  return KHB_OK;
}

uint32_t khb_kang_ring_capacity(const khb_ctx* c) { return c && c->kang ? c->kang->ring_cap : kKangRingDefault; }

int khb_kang_submit(khb_ctx* c, uint32_t steps, uint32_t dp_bits) {
  if (!c || steps == 0 || dp_bits > 32) return KHB_EINVAL;
  if (!c->kang || !c->kang->jumps || !c->kang->herd) return KHB_EINVAL;
  KangState& K = *c->kang;
  if (K.queued == 2) return KHB_EBUSY;
  KHB_TRY(c, hipSetDevice(c->device));
  KangLaunch& L = K.L[(K.head + K.queued) & 1u];
  if (const int rc = ensure_ring(c, L, K.ring_cap)) return rc;
  KangArgs A{};
  A.x = K.d_x;
  A.y = K.d_y;
  A.d = K.d_d;
  A.scr = K.d_scr;
  A.jumps = K.d_jumps;
  A.ring = L.d_ring;
  A.ring_cap = K.ring_cap;
  A.cnt = L.d_cnt;
  A.n = K.herd;
  A.stride = K.stride;
  A.steps = steps;
  A.dp_mask = dp_bits == 32 ? 0xFFFFFFFFu : (1u << dp_bits) - 1u;
  const uint32_t lanes = (K.herd + kKangPerLane - 1) / kKangPerLane;      // <= stride
  KHB_TRY(c, hipMemsetAsync(L.d_cnt, 0, 4 * sizeof(unsigned long long), K.stream));
  KHB_TRY(c, hipEventRecord(L.ev0, K.stream));
  hipLaunchKernelGGL(k_kang_walk, dim3((lanes + kBlock - 1) / kBlock), dim3(kBlock), 0, K.stream, A);
  KHB_TRY(c, hipGetLastError());
  KHB_TRY(c, hipEventRecord(L.ev1, K.stream));
  KHB_TRY(c, hipMemcpyAsync(L.h_cnt, L.d_cnt, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, K.stream));
  L.cap = K.ring_cap;
  L.expect = (uint64_t)K.herd * steps;
  K.queued++;
  return KHB_OK;
}

int khb_kang_collect(khb_ctx* c, khb_kang_dp* out, uint32_t cap, khb_kang_stats* st) {
  if (!c) return KHB_EINVAL;
  if (!c->kang || !c->kang->queued) return KHB_ESTATE;
  KHB_TRY(c, hipSetDevice(c->device));
  KangState& K = *c->kang;
  KangLaunch& L = K.L[K.head & 1u];
  K.head++;
  K.queued--;
  // the oldest launch and the copy of its counters; a later launch in flight is not waited for
  KHB_TRY(c, K.queued ? hipEventSynchronize(K.L[K.head & 1u].ev0) : hipStreamSynchronize(K.stream));
  const uint64_t n_dp = L.h_cnt[0], walked = L.h_cnt[1], seconds = L.h_cnt[2];
  uint64_t take = n_dp < L.cap ? n_dp : L.cap;
  if (take > cap) take = cap;
  if (take && out) {
    std::vector<KangDpDev> h;
    if (!host_alloc(h, take)) return KHB_ENOMEM;
    KHB_TRY(c, hipMemcpy(h.data(), L.d_ring, sizeof(KangDpDev) * take, hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < take; ++i) {
      Fe x, d;
      memcpy(x.v, h[i].x, sizeof x.v);
      memcpy(d.v, h[i].d, sizeof d.v);
      out[i].kangaroo = h[i].i;
      fe_to_be(out[i].x_be, x);
      fe_to_be(out[i].dist_be, d);
    }
  }
  if (st) {
    st->steps_walked = walked;
    st->n_dp = n_dp;
    st->second_choice = seconds;
    st->dp_overflow = n_dp > L.cap ? 1u : 0u;
    float ms = -1.f;
    if (hipEventElapsedTime(&ms, L.ev0, L.ev1) != hipSuccess) ms = -1.f;
    st->kernel_ms = ms;
  }
  return walked == L.expect ? KHB_OK : KHB_EINCOMPLETE;
}

}  // extern "C"
