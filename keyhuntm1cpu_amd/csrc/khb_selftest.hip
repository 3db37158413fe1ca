// libkhbsgs.so: the self-test entry points of include/khbsgs.h (field operations, bloom probe, hash160 / ETH address / xpoint bytes) with their
// kernels, and the point dumps of the two walks (khb_dump_x, khb_addr_dump).  Synchronous, on slot 0.
#include "abi.hpp"

using namespace khbk;

namespace {

// hash160 self-test: for x||y points, kind 0/1 = compressed with prefix 02/03, 2 = uncompressed;
// out = 20 hash bytes + 1 byte bloom_check20 result (when a bloom is given).
__global__ void k_hash160(const Fe* __restrict__ xy, int kind, const uint8_t* __restrict__ bloom, BloomGeom g,
                          uint8_t* __restrict__ out, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Fe x = xy[2 * i], y = xy[2 * i + 1];
  uint32_t h[5];
  if (kind < 2)
    hash160_compressed(h, 2u + (uint32_t)kind, x);
  else
    hash160_uncompressed(h, x, y);
  uint8_t* o = out + 21 * (size_t)i;
  for (int k = 0; k < 5; ++k)
    for (int b = 0; b < 4; ++b) o[4 * k + b] = (uint8_t)(h[k] >> (8 * b));
  o[20] = bloom ? (bloom_check20(bloom, g, h) ? 1 : 0) : 0;
}

// Field self-test: the fast (fe_asm.hpp) operations, results canonicalised; op | KHB_FIELD_OP_RAW leaves the
// value as the function returned it (lazy, < 2^256).
__global__ void k_field_op(int op, const Fe* __restrict__ a, const Fe* __restrict__ b, Fe* __restrict__ r, uint32_t n) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Fe x = a[i], y = b[i], z;
  switch (op & ~KHB_FIELD_OP_RAW) {
    case 0: fm_mul(z, x, y); break;
    case 1: fm_sqr(z, x); break;
    case 2: fm_add(z, x, y); break;
    case 3: fm_sub(z, x, y); break;
    case 5: fm_add_lazy(z, x, y); break;     // x < p, y < 2^256
    case 6: fm_sqr_add(z, x, y); break;      // x, y < 2^256
    default: fm_inv(z, x); break;
  }
  if (!(op & KHB_FIELD_OP_RAW)) fm_canon(z, z);
  r[i] = z;
}

__global__ void k_probe(const uint8_t* __restrict__ bloom, BloomGeom g, const Fe* __restrict__ xs, uint8_t* hit, uint32_t n) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  hit[i] = bloom_probe_x(bloom, g, xs[i]) ? 1 : 0;
}

// khb_hash160 kind 3: the ETH address (device/keccak.hpp) of any 64 bytes x||y, same record as k_hash160.
__global__ void k_eth_address(const Fe* __restrict__ xy, const uint8_t* __restrict__ bloom, BloomGeom g,
                              uint8_t* __restrict__ out, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Fe x = xy[2 * i], y = xy[2 * i + 1];
  uint32_t h[5];
  eth_address(h, x, y);
  uint8_t* o = out + 21 * (size_t)i;
  for (int k = 0; k < 5; ++k)
    for (int b = 0; b < 4; ++b) o[4 * k + b] = (uint8_t)(h[k] >> (8 * b));
  o[20] = bloom ? (bloom_check20(bloom, g, h) ? 1 : 0) : 0;
}

// khb_hash160 kind 4: the 20 bytes -m xpoint probes for x (device/xpoint.hpp), same record as k_hash160.
__global__ void k_x_be20(const Fe* __restrict__ xy, const uint8_t* __restrict__ bloom, BloomGeom g,
                         uint8_t* __restrict__ out, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t h[5];
  x_be20(h, xy[2 * i]);
  uint8_t* o = out + 21 * (size_t)i;
  for (int k = 0; k < 5; ++k)
    for (int b = 0; b < 4; ++b) o[4 * k + b] = (uint8_t)(h[k] >> (8 * b));
  o[20] = bloom ? (bloom_check20(bloom, g, h) ? 1 : 0) : 0;
}

// khb_vanity_match: the vanity kernels' match stage on caller-supplied 20-byte values, the bitmap in LDS as there.
// h: five words per value in hash160_*'s order (their little-endian bytes are the value's bytes).
__global__ __launch_bounds__(256) void k_vanity_match(const uint32_t* __restrict__ lo, const uint32_t* __restrict__ hi,
                                                      const uint32_t* __restrict__ bitmap, uint32_t n_iv,
                                                      const uint32_t* __restrict__ h, uint8_t* __restrict__ hit,
                                                      uint32_t n) {
  vanity_load_bitmap(bitmap);            // every lane of the block reaches the barrier
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t w[5];
  for (int k = 0; k < 5; ++k) w[k] = h[5 * (size_t)i + k];
  hit[i] = vanity_match(vanity_lds(), lo, hi, n_iv, w) ? 1 : 0;
}

// khb_dump_x (kind 1: x of every point of the bsgs walk, 32 bytes each) and khb_addr_dump (kind 2: x||y of the
// address walk, 64 bytes each) of one job's groups.
int dump_points(khb_ctx* c, int kind, const uint8_t* centre, uint32_t group_begin, uint32_t group_count,
                uint8_t* out) {
  const bool bsgs = kind == 1;
  int rc = check_scan_args(c, centre, 1, group_begin, group_count, bsgs);
  if (rc) return rc;
  if (!out) return KHB_EINVAL;
  if (c->queued) return KHB_EBUSY;
  KHB_TRY(c, hipSetDevice(c->device));
  Slot& S = c->slot[0];
  if ((rc = ensure_centres(c, S, 1)) || (bsgs && (rc = ensure_gofs(c)))) return rc;
  pts_from_be(S.h_centres, centre, 1);
  const size_t bytes = (size_t)group_count * KHB_GROUP * (bsgs ? 32 : 64);
  DevBuf<uint8_t> d;
  KHB_TRY(c, d.alloc(bytes));
  KHB_TRY(c, hipMemcpyAsync(S.d_centres, S.h_centres, sizeof(AffPt), hipMemcpyHostToDevice, S.stream));
  S.counters_zero = false;
  KHB_TRY(c, hipMemsetAsync(S.d_counters, 0, kCounterBytes, S.stream));
  ScanArgs A = make_args(c, S, 1, group_begin, group_count, bsgs ? kBatch : 0);
  A.xdump = d;
  uint32_t blocks = (uint32_t)((A.n_items + kBlock - 1) / kBlock);
  if (blocks > c->lanes / kBlock) blocks = c->lanes / kBlock;
  if ((rc = launch_scan(bsgs ? kDump : kAddrDump, blocks, S.stream, A)) || (rc = sync_launch(c, S.stream))) return rc;
  KHB_TRY(c, hipMemcpy(out, d, bytes, hipMemcpyDeviceToHost));
  return KHB_OK;
}

}  // namespace

extern "C" {

int khb_dump_x(khb_ctx* c, const uint8_t* centre, uint32_t group_begin, uint32_t group_count, uint8_t* xs) {
  return dump_points(c, 1, centre, group_begin, group_count, xs);
}

int khb_addr_dump(khb_ctx* c, const uint8_t* centre, uint32_t group_begin, uint32_t group_count, uint8_t* xy) {
  return dump_points(c, 2, centre, group_begin, group_count, xy);
}

int khb_field_op(khb_ctx* c, int op, const uint8_t* a, const uint8_t* b, uint8_t* r, uint32_t n) {
  const int raw = op & KHB_FIELD_OP_RAW;
  op &= ~KHB_FIELD_OP_RAW;
  if (!c || !a || !r || n == 0 || op < 0 || op > 6 || (op != 1 && op != 4 && !b)) return KHB_EINVAL;
  if (raw && (op == 2 || op == 4)) return KHB_EINVAL;   // fm_add is canonical by contract; fm_inv's lazy value is not pinned
  op |= raw;
  KHB_TRY(c, hipSetDevice(c->device));
  Slot& S = c->slot[0];
  std::vector<Fe> h;                     // a, then b (zeros without one), then the results
  if (!host_alloc(h, (size_t)n * 3)) return KHB_ENOMEM;
  fes_from_be(h.data(), a, n);
  if (b) fes_from_be(h.data() + n, b, n);
  DevBuf<Fe> d;
  KHB_TRY(c, d.alloc((size_t)n * 3));
  KHB_TRY(c, hipMemcpy(d, h.data(), sizeof(Fe) * n * 2, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_field_op, dim3((n + 255) / 256), dim3(256), 0, S.stream, op, d, d + n, d + 2 * n, n);
  if (const int rc = sync_launch(c, S.stream)) return rc;
  KHB_TRY(c, hipMemcpy(h.data() + 2 * n, d + 2 * n, sizeof(Fe) * n, hipMemcpyDeviceToHost));
  for (uint32_t i = 0; i < n; ++i) fe_to_be(r + 32 * (size_t)i, h[2 * n + i]);
  return KHB_OK;
}

int khb_probe(khb_ctx* c, const uint8_t* xs, uint8_t* hit, uint32_t n) {
  if (!c || !xs || !hit || n == 0) return KHB_EINVAL;
  if (!c->d_bloom) return KHB_ESTATE;
  KHB_TRY(c, hipSetDevice(c->device));
  Slot& S = c->slot[0];
  std::vector<Fe> h;
  if (!host_alloc(h, n)) return KHB_ENOMEM;
  fes_from_be(h.data(), xs, n);
  DevBuf<Fe> d;
  DevBuf<uint8_t> dh;
  KHB_TRY(c, d.alloc(n));
  KHB_TRY(c, dh.alloc(n));
  KHB_TRY(c, hipMemcpy(d, h.data(), sizeof(Fe) * n, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_probe, dim3((n + 255) / 256), dim3(256), 0, S.stream, c->d_bloom, c->geom, d, dh, n);
  if (const int rc = sync_launch(c, S.stream)) return rc;
  KHB_TRY(c, hipMemcpy(hit, dh, n, hipMemcpyDeviceToHost));
  return KHB_OK;
}

int khb_vanity_match(khb_ctx* c, const uint8_t* h20, uint8_t* hit, uint32_t n) {
  if (!c || !h20 || !hit || n == 0) return KHB_EINVAL;
  if (!c->d_van) return KHB_ESTATE;
  KHB_TRY(c, hipSetDevice(c->device));
  Slot& S = c->slot[0];
  DevBuf<uint32_t> d;                    // 20 bytes per value: on a little-endian host already hash160_*'s words
  DevBuf<uint8_t> dh;
  KHB_TRY(c, d.alloc(5 * (size_t)n));
  KHB_TRY(c, dh.alloc(n));
  KHB_TRY(c, hipMemcpy(d, h20, 20 * (size_t)n, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_vanity_match, dim3((n + 255) / 256), dim3(256), 0, S.stream, c->d_van,
                     c->d_van + 5 * (size_t)c->van_n, c->d_van + 10 * (size_t)c->van_n, c->van_n, d.p, dh.p, n);
  if (const int rc = sync_launch(c, S.stream)) return rc;
  KHB_TRY(c, hipMemcpy(hit, dh, n, hipMemcpyDeviceToHost));
  return KHB_OK;
}

int khb_hash160(khb_ctx* c, int kind, const uint8_t* xy, uint8_t* out, uint32_t n) {
  if (!c || !xy || !out || n == 0 || kind < 0 || kind > 4) return KHB_EINVAL;
  KHB_TRY(c, hipSetDevice(c->device));
  Slot& S = c->slot[0];
  std::vector<AffPt> h;
  if (!host_alloc(h, n)) return KHB_ENOMEM;
  pts_from_be(h.data(), xy, n);
  DevBuf<AffPt> d;
  DevBuf<uint8_t> dout;
  KHB_TRY(c, d.alloc(n));
  KHB_TRY(c, dout.alloc(21 * (size_t)n));
  KHB_TRY(c, hipMemcpy(d, h.data(), sizeof(AffPt) * n, hipMemcpyHostToDevice));
  if (kind == 4)
    hipLaunchKernelGGL(k_x_be20, dim3((n + 255) / 256), dim3(256), 0, S.stream, (const Fe*)d.p, c->d_abloom, c->ageom,
                       dout, n);
  else if (kind == 3)
    hipLaunchKernelGGL(k_eth_address, dim3((n + 255) / 256), dim3(256), 0, S.stream, (const Fe*)d.p, c->d_abloom,
                       c->ageom, dout, n);
  else
    hipLaunchKernelGGL(k_hash160, dim3((n + 255) / 256), dim3(256), 0, S.stream, (const Fe*)d.p, kind, c->d_abloom,
                       c->ageom, dout, n);
  if (const int rc = sync_launch(c, S.stream)) return rc;
  KHB_TRY(c, hipMemcpy(out, dout, 21 * (size_t)n, hipMemcpyDeviceToHost));
  return KHB_OK;
}

}  // extern "C"
