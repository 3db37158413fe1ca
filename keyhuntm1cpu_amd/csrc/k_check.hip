// k_check: the second and third check of level-1 candidates on the device (khb_check),
// bsgs_secondcheck / bsgs_thirdcheck of keyhunt.cpp:4271-4368 as restated in device/confirm.hpp.
// One lane per candidate; 64-lane workgroups (a batch is a few to a few thousand candidates).
// The kernel, its records and the two entry points that use them: khb_load_check_tables and khb_check.
#include "abi.hpp"

namespace khbk {

struct CheckIn {            // khb_check_in with the chunk base as little-endian limbs
  khb::U8 start;
  uint32_t a;
  uint32_t target;
};

struct CheckOut {
  khb::U8 key;
  uint32_t found, l2_hits, l3_hits, bp_hits;
};

__global__ __launch_bounds__(64) void k_check(khb::CheckTables T, const CheckIn* __restrict__ in,
                                              const khb::CPt* __restrict__ targets, uint32_t n_targets,
                                              CheckOut* __restrict__ out, uint32_t n) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  const CheckIn c = in[g];
  khb::CheckResult r{};
  CheckOut o{};
  if (c.target < n_targets) {
    const khb::CPt t = targets[c.target];
    o.found = khb::second_check(T, c.start, c.a, t, r) ? 1u : 0u;
  } else {
    o.found = 0xffffffffu;                     // rejected on the host before the launch; never reached
  }
  o.key = r.key;
  o.l2_hits = r.l2_hits;
  o.l3_hits = r.l3_hits;
  o.bp_hits = r.bp_hits;
  out[g] = o;
}

}  // namespace khbk

using namespace khbk;

namespace {

khb::U8 u8_from_be(const uint8_t* be) {
  Fe f;
  fe_from_be(f, be);
  khb::U8 r;
  memcpy(r.v, f.v, sizeof r.v);
  return r;
}

int ensure_check_buffers(khb_ctx* c, uint32_t n, uint32_t n_targets) {
  if (n > c->ck_cap) {
    hipFree(c->d_ck_in);
    hipFree(c->d_ck_out);
    c->d_ck_in = nullptr;
    c->d_ck_out = nullptr;
    c->ck_cap = 0;
    const uint32_t cap = n < 4096 ? 4096 : n;
    KHB_TRY(c, hipMalloc(&c->d_ck_in, sizeof(CheckIn) * cap));
    KHB_TRY(c, hipMalloc(&c->d_ck_out, sizeof(CheckOut) * cap));
    c->ck_cap = cap;
  }
  if (n_targets > c->ck_tcap) {
    c->ck_targets_be.clear();
    hipFree(c->d_ck_targets);
    c->d_ck_targets = nullptr;
    c->ck_tcap = 0;
    const uint32_t cap = n_targets < 256 ? 256 : n_targets;
    KHB_TRY(c, hipMalloc(&c->d_ck_targets, sizeof(khb::CPt) * cap));
    c->ck_tcap = cap;
  }
  return KHB_OK;
}

}  // namespace

extern "C" {

// ------------------------------------------------------------------- second / third check (§8(f)3)
int khb_load_check_tables(khb_ctx* c, const khb_check_tables* t) {
  if (!c || !t || !t->gtable || !t->amp2 || !t->amp3 || !t->bptable || t->m3 == 0 || t->m3 > (1ull << 40))
    return KHB_EINVAL;
  if (!t->l2 || !bloom_args_ok(t->l2_bytes_per_sub, t->l2_bits_per_sub, t->l2_hashes) || !t->l3 ||
      !bloom_args_ok(t->l3_bytes_per_sub, t->l3_bits_per_sub, t->l3_hashes))
    return KHB_EINVAL;
  KHB_TRY(c, hipSetDevice(c->device));
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  const size_t n_g = 32 * 256, o_g = 0, o_a2 = up(o_g + sizeof(khb::CPt) * n_g), o_a3 = up(o_a2 + sizeof(khb::CPt) * 32);
  const size_t b2 = 256 * (size_t)t->l2_bytes_per_sub, b3 = 256 * (size_t)t->l3_bytes_per_sub;
  const size_t o_l2 = up(o_a3 + sizeof(khb::CPt) * 32), o_l3 = up(o_l2 + b2), o_bp = up(o_l3 + b3);
  const size_t total = o_bp + 16 * (size_t)t->m3;
  std::vector<uint8_t> h;
  if (!host_alloc(h, total)) return KHB_ENOMEM;
  pts_from_be((khb::CPt*)(h.data() + o_g), t->gtable, (uint32_t)n_g);
  pts_from_be((khb::CPt*)(h.data() + o_a2), t->amp2, 32);
  pts_from_be((khb::CPt*)(h.data() + o_a3), t->amp3, 32);
  memcpy(h.data() + o_l2, t->l2, b2);
  memcpy(h.data() + o_l3, t->l3, b3);
  memcpy(h.data() + o_bp, t->bptable, 16 * (size_t)t->m3);
  if (c->ck_stream) KHB_TRY(c, hipStreamSynchronize(c->ck_stream));
  hipFree(c->d_ck);
  c->d_ck = nullptr;
  c->ck_loaded = false;
  KHB_TRY(c, hipMalloc(&c->d_ck, total));
  KHB_TRY(c, hipMemcpy(c->d_ck, h.data(), total, hipMemcpyHostToDevice));
  uint8_t* d = (uint8_t*)c->d_ck;
  khb::CheckTables& T = c->ck;
  T.gtab = (const khb::CPt*)(d + o_g);
  T.amp2 = (const khb::CPt*)(d + o_a2);
  T.amp3 = (const khb::CPt*)(d + o_a3);
  T.l2 = d + o_l2;
  T.l3 = d + o_l3;
  T.bp = d + o_bp;
  T.g2 = bloom_geom(t->l2_bytes_per_sub, t->l2_bits_per_sub, t->l2_hashes);
  T.g3 = bloom_geom(t->l3_bytes_per_sub, t->l3_bits_per_sub, t->l3_hashes);
  T.n_bp = t->m3;
  T.m_double = u8_from_be(t->m_double_be);
  T.m2_double = u8_from_be(t->m2_double_be);
  T.m3 = u8_from_be(t->m3_be);
  T.m3_double = u8_from_be(t->m3_double_be);
  c->ck_loaded = true;
  return KHB_OK;
}

int khb_check(khb_ctx* c, const uint8_t* targets_xy, uint32_t n_targets, const khb_check_in* in, uint32_t n,
              khb_check_out* out) {
  if (!c || (n && (!in || !out)) || (n_targets && !targets_xy)) return KHB_EINVAL;
  if (!c->ck_loaded) return KHB_ESTATE;
  if (n == 0) return KHB_OK;
  for (uint32_t i = 0; i < n; ++i)
    if (in[i].target >= n_targets) return KHB_EINVAL;
  KHB_TRY(c, hipSetDevice(c->device));
  if (!c->ck_stream) {
    int lo = 0, hi = 0;
    KHB_TRY(c, hipDeviceGetStreamPriorityRange(&lo, &hi));
    KHB_TRY(c, hipStreamCreateWithPriority(&c->ck_stream, hipStreamNonBlocking, hi));
  }
  int rc = ensure_check_buffers(c, n, n_targets);
  if (rc) return rc;
  std::vector<CheckIn> hin(n);
  std::vector<CheckOut> hout(n);
  for (uint32_t i = 0; i < n; ++i) {
    hin[i].start = u8_from_be(in[i].start_be);
    hin[i].a = in[i].a;
    hin[i].target = in[i].target;
  }
  KHB_TRY(c, hipMemcpyAsync(c->d_ck_in, hin.data(), sizeof(CheckIn) * n, hipMemcpyHostToDevice, c->ck_stream));
  const size_t tbytes = 64 * (size_t)n_targets;
  const bool same = c->ck_targets_be.size() == tbytes && (tbytes == 0 || !memcmp(c->ck_targets_be.data(), targets_xy, tbytes));
  std::vector<khb::CPt> ht;
  if (!same) {
    ht.resize(n_targets);
    pts_from_be(ht.data(), targets_xy, n_targets);
    c->ck_targets_be.clear();            // invalid until the upload below has been issued
    KHB_TRY(c, hipMemcpyAsync(c->d_ck_targets, ht.data(), sizeof(khb::CPt) * n_targets, hipMemcpyHostToDevice,
                              c->ck_stream));
    c->ck_targets_be.assign(targets_xy, targets_xy + tbytes);
  }
  hipLaunchKernelGGL(k_check, dim3((n + 63) / 64), dim3(64), 0, c->ck_stream, c->ck, c->d_ck_in, c->d_ck_targets,
                     n_targets, c->d_ck_out, n);
  KHB_TRY(c, hipGetLastError());
  KHB_TRY(c, hipMemcpyAsync(hout.data(), c->d_ck_out, sizeof(CheckOut) * n, hipMemcpyDeviceToHost, c->ck_stream));
  KHB_TRY(c, hipStreamSynchronize(c->ck_stream));
  for (uint32_t i = 0; i < n; ++i) {
    Fe k;
    memcpy(k.v, hout[i].key.v, sizeof k.v);
    fe_to_be(out[i].key_be, k);
    out[i].found = hout[i].found;
    out[i].l2_hits = hout[i].l2_hits;
    out[i].l3_hits = hout[i].l3_hits;
    out[i].bp_hits = hout[i].bp_hits;
  }
  return KHB_OK;
}

}  // extern "C"
