// libkhhost.so: C ABI over the host engine (include/khhost.h).
#include <string.h>

#include <string>
#include <thread>
#include <vector>

#include "../../../include/khbsgs.h"
#include "../../../include/khhost.h"
#include "address_host.hpp"
#include "bsgs_host.hpp"
#include "engine.hpp"
#include "kang_host.hpp"
#include "mini_host.hpp"

using namespace khb;
using namespace khbk;   // SearchMode and its decoder (device/scan_modes.hpp)

struct khh_tables {
  Tables t;
};

struct khh_addr {
  AddrTargets T;
  AddrGen G;
  uint64_t n_seq = 0;
  uint32_t hit_cap = 0;      // tests: bloom-hit ring capacity per launch (0 = library default)
  std::vector<uint8_t> van_bytes;   // khh_addr_vanity_intervals: lo || hi of the merged intervals
};

struct khh_mini {
  MiniSearch S;
  uint32_t queue_cap = 0, hit_cap = 0;   // tests: the launches' capacities (0 = library defaults)
};

struct khh_kang {
  KangSearch S;
};

static void set_err(char* err, size_t n, const std::string& m) {
  if (err && n) {
    strncpy(err, m.c_str(), n - 1);
    err[n - 1] = 0;
  }
}

extern "C" {

int khh_abi_version(void) { return KHH_ABI_VERSION; }

// The khh_tables_new* constructors: geometry, Tables::obtain from src (threads and gpl defaulted here), and the
// results they hand back.  resident_gate: khh_tables_new_resident's explicit gate size.
static khh_tables* tables_new(const char* n_str, int k, int threads, uint32_t gpl, TableSource src,
                              uint32_t resident_gate, uint32_t* have, double* kernel_ms, char* err, size_t errlen) {
  Geometry g;
  std::string e;
  if (!make_geometry(n_str, k, g, e)) { set_err(err, errlen, e); return nullptr; }
  if (resident_gate && (resident_gate < 13 || resident_gate > 38)) {
    set_err(err, errlen, "[E] resident gate size: 0 or 13..38 (log2 bits)");
    return nullptr;
  }
  khh_tables* t = new khh_tables();
  src.threads = threads > 0 ? threads : (int)std::thread::hardware_concurrency();
  src.gpl = gpl ? gpl : 4;
  t->t.resident_gate = resident_gate;
  if (!t->t.obtain(g, src, have, e)) {
    set_err(err, errlen, e);
    delete t;
    return nullptr;
  }
  if (kernel_ms) *kernel_ms = t->t.build_gpu_ms;
  return t;
}

khh_tables* khh_tables_new(const char* n_str, int k, int threads, uint32_t gpl, char* err, size_t errlen) {
  return tables_new(n_str, k, threads, gpl, TableSource(), 0, nullptr, nullptr, err, errlen);
}

khh_tables* khh_tables_new_files(const char* n_str, int k, int threads, uint32_t gpl, const char* dir,
                                 int skip_checksum, int save, uint32_t* have, char* err, size_t errlen) {
  TableSource src;
  src.dir = dir ? dir : ".";
  src.skip_checksum = skip_checksum != 0;
  src.save = save != 0;
  return tables_new(n_str, k, threads, gpl, src, 0, have, nullptr, err, errlen);
}

khh_tables* khh_tables_new_gpu(const char* n_str, int k, int threads, uint32_t gpl, int device, double* kernel_ms,
                               char* err, size_t errlen) {
  TableSource src;
  src.device = device;
  return tables_new(n_str, k, threads, gpl, src, 0, nullptr, kernel_ms, err, errlen);
}

khh_tables* khh_tables_new_resident(const char* n_str, int k, int threads, uint32_t gpl, int device,
                                    uint32_t gate_log2, double* kernel_ms, char* err, size_t errlen) {
  TableSource src;
  src.device = device;
  src.resident = true;
  return tables_new(n_str, k, threads, gpl, src, gate_log2, nullptr, kernel_ms, err, errlen);
}

int khh_tables_is_resident(const khh_tables* t) { return t && t->t.resident ? 1 : 0; }

int khh_tables_set_resident_stages(khh_tables* t, uint32_t stage1_log2, uint32_t stage0_log2) {
  if (!t || !t->t.resident) return KHB_EINVAL;
  if (stage1_log2 > 1 && (stage1_log2 < 10 || stage1_log2 > 31)) return KHB_EINVAL;
  if (stage0_log2 > 1 && (stage0_log2 < 10 || stage0_log2 > 30)) return KHB_EINVAL;
  t->t.resident_stage1 = stage1_log2;
  t->t.resident_stage0 = stage0_log2;
  return 0;
}

uint32_t khh_resident_gate_log2(uint64_t l1ext, uint64_t budget_bytes) {
  return Tables::resident_gate_log2(l1ext, budget_bytes);
}

int khh_resident_keeps_fold(uint64_t l1ext, uint32_t gate_log2) {
  return Tables::resident_keeps_fold(l1ext, gate_log2) ? 1 : 0;
}

int khh_tables_save(const khh_tables* t, const char* dir, char* err, size_t errlen) {
  std::string e;
  if (!t->t.save_files(dir ? dir : ".", 0, e, nullptr)) {
    set_err(err, errlen, e);
    return -100;
  }
  return 0;
}

void khh_tables_free(khh_tables* t) { delete t; }

void khh_params(const khh_tables* t, uint64_t out[10]) {
  const Geometry& g = t->t.geo;
  out[0] = g.m; out[1] = g.m2; out[2] = g.m3; out[3] = g.aux; out[4] = g.cycles;
  out[5] = g.N.w[0]; out[6] = g.l1ext; out[7] = g.items1; out[8] = g.items2; out[9] = g.items3;
}

const uint8_t* khh_bloom(const khh_tables* t, int level, int idx, uint64_t* bytes, uint64_t* bits, uint32_t* hashes) {
  if (idx < 0 || idx > 255 || level < 1 || level > 3) return nullptr;
  const BloomFilter& b = level == 1 ? t->t.l1[idx] : level == 2 ? t->t.l2[idx] : t->t.l3[idx];
  if (bytes) *bytes = b.bytes;
  if (bits) *bits = b.bits;
  if (hashes) *hashes = b.hashes;
  if (level == 1 && t->t.resident) return nullptr;   // the geometry only: the bits live on the devices
  return b.bf.data();
}

void khh_giant_table(const khh_tables* t, uint8_t out[513 * 64]) {
  std::vector<uint8_t> v = t->t.giant_table_be();
  memcpy(out, v.data(), v.size());
}

void khh_amp_table(const khh_tables* t, int level, uint8_t out[32 * 64]) {
  const Pt* a = level == 2 ? t->t.amp2 : t->t.amp3;
  for (int i = 0; i < 32; ++i) pt_to_be(out + 64 * i, a[i]);
}

uint32_t khh_lane_offsets(const khh_tables* t, uint8_t* out, uint32_t* gpl) {
  if (gpl) *gpl = t->t.gpl;
  if (out) {
    std::vector<uint8_t> v = t->t.lane_offsets_be();
    memcpy(out, v.data(), v.size());
  }
  return (uint32_t)t->t.lane_offs.size();
}

uint32_t khh_gate_probes(const khh_tables* t) { return t->t.gate_probes; }

const uint8_t* khh_gate(const khh_tables* t, uint32_t* log2) {
  if (log2) *log2 = t->t.gate_log2;
  return t->t.gate_log2 ? t->t.gate.data() : nullptr;
}

const uint8_t* khh_bptable(const khh_tables* t, uint64_t* n) {
  static_assert(sizeof(XValue) == 16, "bsgs_xvalue is 16 bytes");
  if (n) *n = t->t.bp.size();
  return reinterpret_cast<const uint8_t*>(t->t.bp.data());
}

int khh_chunk_centre(const khh_tables* t, const uint8_t base_be[32], const uint8_t target_xy[64], uint8_t out_xy[64]) {
  const U256 base = U256::from_be(base_be);
  const Pt tg = pt_from_be(target_xy);
  const Pt aux = t->t.chunk_aux(base);
  Pt c;
  batch_add_direct(&tg, aux, 1, &c);
  pt_to_be(out_xy, c);
  return 0;
}

int khh_job_centres(const khh_tables* t, const uint8_t* bases_be, uint32_t n_chunks, const uint8_t* targets_xy,
                    uint32_t n_targets, uint8_t* out_xy, int threads) {
  if (!t || !bases_be || !targets_xy || !out_xy) return -1;
  std::vector<U256> bases(n_chunks);
  for (uint32_t c = 0; c < n_chunks; ++c) bases[c] = U256::from_be(bases_be + 32 * (size_t)c);
  std::vector<Pt> tp(n_targets);
  for (uint32_t j = 0; j < n_targets; ++j) tp[j] = pt_from_be(targets_xy + 64 * (size_t)j);
  job_centres(t->t, bases, tp, out_xy, threads);
  return 0;
}

int khh_secondcheck(const khh_tables* t, const uint8_t base_be[32], uint32_t a, const uint8_t target_xy[64],
                    uint8_t key_be[32]) {
  U256 key;
  if (!t->t.secondcheck(U256::from_be(base_be), a, pt_from_be(target_xy), key)) return 0;
  key.to_be(key_be);
  return 1;
}

struct khh_session {
  Session s;
  bool record = false;                 // tests: keep every level-1 candidate of the last run
  struct Rec {
    U256 base;
    uint32_t target, a;
  };
  std::vector<Rec> recorded;
};

khh_session* khh_session_open(const khh_tables* t, const int* devices, int n_devices, uint32_t lanes,
                              uint32_t chunks_per_batch, int check_threads, char* err, size_t errlen) {
  if (!t || !devices || n_devices <= 0) { set_err(err, errlen, "[E] bad arguments"); return nullptr; }
  SearchConfig cfg;
  cfg.devices.assign(devices, devices + n_devices);
  cfg.lanes = lanes;
  cfg.chunks_per_batch = chunks_per_batch;
  cfg.check_threads = check_threads;
  khh_session* s = new khh_session();
  std::string e;
  if (s->s.open(t->t, cfg, e)) {
    set_err(err, errlen, e);
    delete s;
    return nullptr;
  }
  return s;
}

void khh_session_close(khh_session* s) { delete s; }

int khh_session_resident_info(const khh_session* s, uint64_t* out, uint32_t cap_devices) {
  if (!s) return KHB_EINVAL;
  const std::vector<Session::ResidentInfo>& v = s->s.resident_info();
  for (size_t i = 0; out && i < v.size() && i < cap_devices; ++i) {
    const uint64_t r[KHH_RESIDENT_INFO] = {v[i].l1_bytes, v[i].gate_log2, v[i].gate_probes, v[i].fold_log2,
                                           v[i].stage0_log2, (uint64_t)(v[i].build_ms * 1e3), v[i].free_bytes,
                                           v[i].total_bytes};
    memcpy(out + KHH_RESIDENT_INFO * i, r, sizeof r);
  }
  return (int)v.size();
}

int khh_session_resident_bytes(khh_session* s, uint32_t index, int which, uint64_t* bytes) {
  khb_ctx* c = s ? s->s.context(index) : nullptr;
  return c ? khb_resident_bytes(c, which, bytes) : KHB_EINVAL;
}

int khh_session_resident_read(khh_session* s, uint32_t index, int which, uint64_t offset, uint64_t bytes,
                              uint8_t* out) {
  khb_ctx* c = s ? s->s.context(index) : nullptr;
  return c ? khb_resident_read(c, which, offset, bytes, out) : KHB_EINVAL;
}

int khh_session_resident_popcount(khh_session* s, uint32_t index, int which, uint64_t* bits_set) {
  khb_ctx* c = s ? s->s.context(index) : nullptr;
  return c ? khb_resident_popcount(c, which, bits_set) : KHB_EINVAL;
}

int khh_session_gate_probe(khh_session* s, uint32_t index, const uint8_t* xs, uint8_t* out, uint32_t n) {
  khb_ctx* c = s ? s->s.context(index) : nullptr;
  return c ? khb_gate_probe(c, xs, out, n) : KHB_EINVAL;
}

int khh_session_run(khh_session* s, const uint8_t* targets_xy, int n_targets, const uint8_t start_be[32],
                    const uint8_t end_be[32], uint64_t max_chunks, int random_chunks, int* found, uint8_t* keys_be,
                    uint64_t* stats_out, char* err, size_t errlen) {
  return khh_session_run_ex(s, targets_xy, n_targets, start_be, end_be, max_chunks, random_chunks, found, keys_be,
                            stats_out, stats_out ? 6 : 0, err, errlen);
}

int khh_session_run_ex(khh_session* s, const uint8_t* targets_xy, int n_targets, const uint8_t start_be[32],
                       const uint8_t end_be[32], uint64_t max_chunks, int random_chunks, int* found, uint8_t* keys_be,
                       uint64_t* stats_out, uint32_t stats_len, char* err, size_t errlen) {
  if (!s || !targets_xy || n_targets <= 0) return KHB_EINVAL;
  std::vector<Target> tg((size_t)n_targets);
  for (int k = 0; k < n_targets; ++k) tg[k].p = pt_from_be(targets_xy + 64 * k);
  SearchCallbacks cb;
  s->recorded.clear();
  if (s->record)
    cb.on_candidate = [s](const U256& base, int k, uint32_t a) { s->recorded.push_back({base, (uint32_t)k, a}); };
  std::vector<int> f;
  std::vector<U256> keys;
  SearchStats st;
  std::string e;
  int rc = s->s.run(tg, U256::from_be(start_be), U256::from_be(end_be), cb, f, keys, st, e, max_chunks,
                    random_chunks != 0);
  for (int k = 0; k < n_targets; ++k) {
    if (found) found[k] = f.empty() ? 0 : f[k];
    if (keys_be) (f.empty() ? U256() : keys[k]).to_be(keys_be + 32 * k);
  }
  if (stats_out) {
    const uint64_t v[KHH_SESSION_STATS] = {
        st.chunks, st.giant_steps, st.candidates, st.degenerate, (uint64_t)(st.kernel_seconds * 1e6), st.launches,
        st.rescans, (uint64_t)(st.busy_seconds * 1e6),
        st.shader_mhz_n ? (uint64_t)(1e3 * st.shader_mhz_sum / st.shader_mhz_n) : 0, st.device_checked,
        (uint64_t)(st.device_check_seconds * 1e6), (uint64_t)(st.event_seconds * 1e6)};
    memcpy(stats_out, v, sizeof(uint64_t) * (stats_len < KHH_SESSION_STATS ? stats_len : KHH_SESSION_STATS));
  }
  if (rc) set_err(err, errlen, e);
  return rc;
}

int khh_session_set_test_hooks(khh_session* s, uint32_t cand_cap, int use_gate, int record, const uint8_t* l1_concat) {
  if (!s) return KHB_EINVAL;
  s->s.config().record_candidates = record != 0;
  s->record = record != 0;
  return s->s.set_test_hooks(cand_cap, use_gate != 0, l1_concat);
}

int khh_session_set_check_mode(khh_session* s, int mode) {
  if (!s) return KHB_EINVAL;
  return s->s.set_check_mode(mode);
}

int khh_session_set_chunk_mode(khh_session* s, int mode) {
  if (!s || mode < kChunkSequential || mode > kChunkDance) return KHB_EINVAL;
  s->s.config().chunk_mode = mode;
  return 0;
}

uint64_t khh_chunk_sequence(int mode, const uint8_t start_be[32], const uint8_t end_be[32], const uint8_t two_n_be[32],
                            uint64_t seed, uint8_t* out_be, uint64_t cap) {
  if (mode < kChunkSequential || mode > kChunkDance) return 0;
  const U256 two_n = U256::from_be(two_n_be);
  if (two_n == U256()) return 0;
  ChunkCursor c(mode, U256::from_be(start_be), U256::from_be(end_be), two_n, seed);
  uint64_t n = 0;
  U256 base;
  while (n < cap && c.next(base)) {
    if (out_be) base.to_be(out_be + 32 * n);
    n++;
  }
  return n;
}

void khh_gtable(uint8_t out[32 * 256 * 64]) {
  const std::vector<uint8_t>& g = gtable_be();
  memcpy(out, g.data(), g.size());
}

uint64_t khh_session_recorded(const khh_session* s, uint8_t* bases_be, uint32_t* targets, uint32_t* a, uint64_t cap) {
  if (!s) return 0;
  for (uint64_t i = 0; i < s->recorded.size() && i < cap; ++i) {
    if (bases_be) s->recorded[i].base.to_be(bases_be + 32 * i);
    if (targets) targets[i] = s->recorded[i].target;
    if (a) a[i] = s->recorded[i].a;
  }
  return s->recorded.size();
}

int khh_search(const khh_tables* t, const uint8_t* targets_xy, int n_targets, const uint8_t start_be[32],
               const uint8_t end_be[32], const int* devices, int n_devices, uint32_t lanes,
               uint32_t chunks_per_batch, uint64_t max_chunks, int* found, uint8_t* keys_be, uint64_t* stats_out,
               char* err, size_t errlen) {
  khh_session* s = khh_session_open(t, devices, n_devices, lanes, chunks_per_batch, 0, err, errlen);
  if (!s) return KHB_ENODEV;
  int rc = khh_session_run(s, targets_xy, n_targets, start_be, end_be, max_chunks, 0, found, keys_be, stats_out, err,
                           errlen);                                 // khh_search's stats hold 6
  khh_session_close(s);
  return rc;
}

int khh_pubkey(const uint8_t key_be[32], uint8_t out_xy[64]) {
  const U256 k = U256::from_be(key_be);
  if (k.is_zero() || k >= secp_order()) return KHB_EINVAL;
  pt_to_be(out_xy, mul_g(k));
  return 0;
}

int khh_parse_pubkey(const char* hex, uint8_t out_xy[64], int* compressed) {
  Pt p;
  bool c = true;
  if (!parse_pubkey_hex(hex, p, c, nullptr)) return KHB_EINVAL;
  pt_to_be(out_xy, p);
  if (compressed) *compressed = c ? 1 : 0;
  return 0;
}

static khh_addr* addr_new(TargetKind kind, const char* text, int bloom_multiplier, const uint8_t stride_be[32],
                          uint64_t n_seq, uint32_t gpl, int threads, char* err, size_t errlen) {
  if (!text || n_seq < 1024 || n_seq % 1024) {
    set_err(err, errlen, "n must be a positive multiple of 1024");
    return nullptr;
  }
  khh_addr* a = new khh_addr();
  std::string e;
  if (!AddrTargets::load_text(text, bloom_multiplier, a->T, &e, kind)) {
    set_err(err, errlen, e);
    delete a;
    return nullptr;
  }
  const U256 stride = stride_be ? U256::from_be(stride_be) : U256(1);
  if (stride.is_zero()) {
    set_err(err, errlen, "stride must be positive");
    delete a;
    return nullptr;
  }
  if (threads <= 0) threads = (int)std::thread::hardware_concurrency();
  a->n_seq = n_seq;
  a->van_bytes = a->T.van.merged_bytes();
  a->G.build(stride, (uint32_t)(n_seq / 1024), gpl ? gpl : 16, threads);
  return a;
}

khh_addr* khh_addr_new(const char* text, int bloom_multiplier, const uint8_t stride_be[32], uint64_t n_seq,
                       uint32_t gpl, int threads, char* err, size_t errlen) {
  return addr_new(kTargetsBtc, text, bloom_multiplier, stride_be, n_seq, gpl, threads, err, errlen);
}

khh_addr* khh_addr_new_eth(const char* text, int bloom_multiplier, const uint8_t stride_be[32], uint64_t n_seq,
                           uint32_t gpl, int threads, char* err, size_t errlen) {
  return addr_new(kTargetsEth, text, bloom_multiplier, stride_be, n_seq, gpl, threads, err, errlen);
}

khh_addr* khh_addr_new_xpoint(const char* text, int bloom_multiplier, const uint8_t stride_be[32], uint64_t n_seq,
                              uint32_t gpl, int threads, char* err, size_t errlen) {
  return addr_new(kTargetsXpoint, text, bloom_multiplier, stride_be, n_seq, gpl, threads, err, errlen);
}

khh_addr* khh_addr_new_vanity(const char* text, const uint8_t stride_be[32], uint64_t n_seq, uint32_t gpl, int threads,
                              char* err, size_t errlen) {
  return addr_new(kTargetsVanity, text, 1, stride_be, n_seq, gpl, threads, err, errlen);
}

const uint8_t* khh_addr_vanity_intervals(const khh_addr* a, uint64_t* n) {
  if (n) *n = a ? a->van_bytes.size() / 40 : 0;
  return a && !a->van_bytes.empty() ? a->van_bytes.data() : nullptr;
}

int khh_addr_vanity_match(const khh_addr* a, const uint8_t* h20, uint8_t* out, uint64_t n) {
  if (!a || a->T.kind != kTargetsVanity || !h20 || !out) return KHB_EINVAL;
  for (uint64_t i = 0; i < n; ++i) {
    const uint8_t* h = h20 + 20 * i;
    out[i] = (uint8_t)((a->T.van.in_table(h) ? 1 : 0) | (a->T.van.matches(h) ? 2 : 0));
  }
  return KHB_OK;
}

int khh_vanity_target_ok(const char* s) {
  std::vector<VanityInterval> iv;
  return s && VanityTargets::intervals_of(s, iv) ? 1 : 0;
}

uint64_t khh_addr_counted(const khh_addr* a) { return a ? a->T.counted : 0; }

void khh_addr_free(khh_addr* a) { delete a; }

uint64_t khh_addr_skipped(const khh_addr* a) { return a ? a->T.skipped.size() : 0; }

const uint8_t* khh_addr_table(const khh_addr* a, uint64_t* n) {
  if (n) *n = a->T.table.size();
  return a->T.table.empty() ? nullptr : a->T.table[0].data();
}

const uint8_t* khh_addr_bloom(const khh_addr* a, uint64_t* bytes, uint64_t* bits, uint32_t* hashes) {
  if (bytes) *bytes = a->T.bloom.bytes;
  if (bits) *bits = a->T.bloom.bits;
  if (hashes) *hashes = a->T.bloom.hashes;
  return a->T.bloom.bf.data();
}

void khh_addr_giant_table(const khh_addr* a, uint8_t out[513 * 64]) {
  const std::vector<uint8_t> v = a->G.table_be();
  memcpy(out, v.data(), v.size());
}

uint32_t khh_addr_lane_offsets(const khh_addr* a, uint8_t* out, uint32_t* gpl) {
  if (gpl) *gpl = a->G.gpl;
  if (out) {
    const std::vector<uint8_t> v = a->G.offs_be();
    memcpy(out, v.data(), v.size());
  }
  return (uint32_t)a->G.offs.size();
}

int khh_addr_search(const khh_addr* a, const uint8_t start_be[32], const uint8_t end_be[32], int search,
                    int random_chunks, const int* devices, int n_devices, uint32_t lanes, uint64_t max_chunks,
                    uint8_t* keys_be, uint8_t* compressed, uint8_t* rmd, uint32_t cap, uint32_t* n_found,
                    uint64_t* stats_out, char* err, size_t errlen) {
  return khh_addr_search_ex(a, start_be, end_be, search, random_chunks, devices, n_devices, lanes, max_chunks, keys_be,
                            compressed, rmd, cap, n_found, stats_out, stats_out ? 6 : 0, err, errlen);
}

int khh_addr_search_ex(const khh_addr* a, const uint8_t start_be[32], const uint8_t end_be[32], int search,
                       int random_chunks, const int* devices, int n_devices, uint32_t lanes, uint64_t max_chunks,
                       uint8_t* keys_be, uint8_t* compressed, uint8_t* rmd, uint32_t cap, uint32_t* n_found,
                       uint64_t* stats_out, uint32_t stats_len, char* err, size_t errlen) {
  if (!a || !start_be || !end_be) return KHB_EINVAL;
  // KHB_SEARCH_ETH with -e is no search either, but addr_search answers it with the text about the handle's targets;
  // KHB_SEARCH_VANITY is the search's to add, not the caller's
  SearchMode sm;
  if ((!decode_search(search, sm) && search != (KHB_SEARCH_ETH | KHB_SEARCH_ENDOMORPHISM)) || sm.vanity) {
    set_err(err, errlen, "search must be 0, 1 or 2 (-l) or KHB_SEARCH_XPOINT, optionally with KHB_SEARCH_ENDOMORPHISM, "
                         "or KHB_SEARCH_ETH alone");
    return KHB_EINVAL;
  }
  AddrConfig cfg;
  cfg.search = search;
  cfg.start = U256::from_be(start_be);
  cfg.end = U256::from_be(end_be);
  cfg.n_seq = a->n_seq;
  cfg.random = random_chunks != 0;
  cfg.lanes = lanes;
  cfg.gpl = a->G.gpl;
  cfg.max_chunks = max_chunks;
  cfg.hit_cap = a->hit_cap;
  cfg.devices.clear();
  for (int i = 0; i < n_devices; ++i) cfg.devices.push_back(devices[i]);
  if (cfg.devices.empty()) cfg.devices.push_back(0);
  uint32_t nf = 0;
  AddrCallbacks cb;
  cb.on_found = [&](const AddrFound& f) {
    if (nf < cap) {
      if (keys_be) f.key.to_be(keys_be + 32 * (size_t)nf);
      if (compressed) compressed[nf] = f.compressed ? 1 : 0;
      if (rmd) memcpy(rmd + 20 * (size_t)nf, f.rmd.data(), 20);
    }
    ++nf;
  };
  AddrStats st;
  std::string e;
  const int rc = addr_search(a->T, a->G, cfg, cb, &st, &e);
  if (n_found) *n_found = nf;
  if (stats_out) {
    const uint64_t v[KHH_ADDR_STATS] = {
        st.chunks, st.keys, st.hits, st.degenerate, (uint64_t)(st.kernel_seconds * 1e6), st.launches,
        st.shader_mhz_n ? (uint64_t)(1e3 * st.shader_mhz_sum / st.shader_mhz_n) : 0, st.rescans};
    memcpy(stats_out, v, sizeof(uint64_t) * (stats_len < KHH_ADDR_STATS ? stats_len : KHH_ADDR_STATS));
  }
  if (rc) set_err(err, errlen, e);
  return rc;
}

int khh_addr_set_hit_capacity(khh_addr* a, uint32_t cap) {
  if (!a) return KHB_EINVAL;
  a->hit_cap = cap;
  return KHB_OK;
}

int khh_addr_confirm(const khh_addr* a, const uint8_t key_be[32], uint32_t kind, uint8_t out_key_be[32],
                     int* compressed) {
  if (!a || !key_be) return KHB_EINVAL;
  AddrFound f;
  if (!confirm_hit(a->T, U256::from_be(key_be), kind, &f)) return 0;
  if (out_key_be) f.key.to_be(out_key_be);
  if (compressed) *compressed = f.compressed ? 1 : 0;
  return 1;
}

void khh_eth_address(const uint8_t xy[64], uint8_t out[20]) { eth_address_xy(xy, out); }

// ---------------------------------------------------------------------------------- -m minikeys
khh_mini* khh_mini_new(const char* text, int bloom_multiplier, const uint8_t* alphabet, uint32_t window_bits,
                       int threads, char* err, size_t errlen) {
  if (!text) {
    set_err(err, errlen, "no targets");
    return nullptr;
  }
  if (window_bits == 0) window_bits = 16;   // the measured default
  if (window_bits != 4 && window_bits != 8 && window_bits != 16) {
    set_err(err, errlen, "window_bits: 4, 8 or 16");
    return nullptr;
  }
  khh_mini* m = new khh_mini();
  std::string e;
  if (!m->S.A.set(alphabet)) {
    set_err(err, errlen, "the alphabet is 58 distinct non-zero bytes");
    delete m;
    return nullptr;
  }
  if (!AddrTargets::load_text(text, bloom_multiplier, m->S.T, &e, kTargetsBtc)) {
    set_err(err, errlen, e);
    delete m;
    return nullptr;
  }
  if (threads <= 0) threads = (int)std::thread::hardware_concurrency();
  m->S.window_bits = window_bits;
  m->S.table = mini_table_be(window_bits, threads);
  return m;
}

void khh_mini_free(khh_mini* m) { delete m; }

const uint8_t* khh_mini_table(const khh_mini* m, uint64_t* n_points, uint32_t* window_bits) {
  if (n_points) *n_points = m ? m->S.table.size() / 64 : 0;
  if (window_bits) *window_bits = m ? m->S.window_bits : 0;
  return m ? m->S.table.data() : nullptr;
}

int khh_mini_string(const khh_mini* m, const char* first22, uint64_t offset, char* out22) {
  MiniDigits d;
  if (!m || !first22 || !out22 || !mini_parse(m->S.A, first22, kMiniLen, d, nullptr))
    return KHB_EINVAL;
  if (!mini_advance(d, offset)) return KHB_EINVAL;
  mini_string(m->S.A, d, out22);
  return KHB_OK;
}

int khh_mini_valid(const khh_mini* m, const char* minikey22) {
  MiniDigits d;
  if (!m || !minikey22 || !mini_parse(m->S.A, minikey22, kMiniLen, d, nullptr))
    return KHB_EINVAL;
  return mini_is_valid(minikey22) ? 1 : 0;
}

void khh_mini_key(const char* minikey22, uint8_t out32[32]) { mini_key_of(minikey22, out32); }

int khh_mini_set_queue_capacity(khh_mini* m, uint32_t cap) {
  if (!m) return KHB_EINVAL;
  m->queue_cap = cap;
  return KHB_OK;
}

int khh_mini_set_hit_capacity(khh_mini* m, uint32_t cap) {
  if (!m) return KHB_EINVAL;
  m->hit_cap = cap;
  return KHB_OK;
}

double khh_mini_cpu_scan(const khh_mini* m, const char* first22, uint64_t count, int threads, uint64_t* valid,
                         uint64_t* found) {
  MiniDigits first, last;
  if (!m || !first22 || count == 0 || !mini_parse(m->S.A, first22, kMiniLen, first, nullptr)) return -1.0;
  last = first;
  if (!mini_advance(last, count - 1)) return -1.0;
  return mini_cpu_scan(m->S, first, count, threads, valid, found);
}

int khh_mini_search(const khh_mini* m, const char* first22, size_t first_len, uint64_t count, const int* devices,
                    int n_devices, uint32_t lanes, uint64_t per_launch, char* minikeys, uint8_t* keys_be, uint8_t* rmd,
                    uint32_t cap, uint32_t* n_found, uint64_t* stats_out, uint32_t stats_len, char* err,
                    size_t errlen) {
  if (!m) return KHB_EINVAL;
  std::string e;
  MiniDigits first;
  if (!mini_parse(m->S.A, first22, first_len, first, &e)) {
    set_err(err, errlen, e);
    return KHB_EINVAL;
  }
  MiniConfig cfg;
  cfg.lanes = lanes;
  if (per_launch) cfg.per_launch = per_launch;
  cfg.queue_cap = m->queue_cap;
  cfg.hit_cap = m->hit_cap;
  cfg.devices.clear();
  for (int i = 0; i < n_devices; ++i) cfg.devices.push_back(devices[i]);
  if (cfg.devices.empty()) cfg.devices.push_back(0);
  uint32_t nf = 0;
  auto on_found = [&](const MiniFound& f) {
    if (nf < cap) {
      if (minikeys) memcpy(minikeys + (size_t)kMiniLen * nf, f.minikey, kMiniLen);
      if (keys_be) f.key.to_be(keys_be + 32 * (size_t)nf);
      if (rmd) memcpy(rmd + 20 * (size_t)nf, f.rmd.data(), 20);
    }
    ++nf;
  };
  MiniStats st;
  const int rc = mini_search(m->S, first, count, cfg, on_found, &st, &e);
  if (n_found) *n_found = nf;
  if (stats_out) {
    const uint64_t v[KHH_MINI_STATS] = {st.candidates, st.valid, st.bad_keys, st.hits, st.launches, st.rescans,
                                        (uint64_t)(st.filter_seconds * 1e6), (uint64_t)(st.keys_seconds * 1e6)};
    memcpy(stats_out, v, sizeof(uint64_t) * (stats_len < KHH_MINI_STATS ? stats_len : KHH_MINI_STATS));
  }
  if (rc) set_err(err, errlen, e);
  return rc;
}

// ---------------------------------------------------------------------------------- kangaroo interval search
khh_kang* khh_kang_new(const uint8_t pub_xy[64], const uint8_t start_be[32], const uint8_t end_be[32], int dp_bits,
                       uint64_t herd, uint64_t seed, uint64_t herd_cap, char* err, size_t errlen) {
  if (!pub_xy || !start_be || !end_be) {
    set_err(err, errlen, "no public key or interval");
    return nullptr;
  }
  if (herd_cap == 0) {
    herd_cap = khb_kang_full_herd(0);
    if (herd_cap == 0) herd_cap = (uint64_t)khb_kang_per_lane() << 18;      // an MI355X's 262,144 lanes
  }
  khh_kang* k = new khh_kang();
  std::string e;
  if (!kang_init(k->S, pt_from_be(pub_xy), U256::from_be(start_be), U256::from_be(end_be), dp_bits, herd, seed,
                 herd_cap, &e)) {
    set_err(err, errlen, e);
    delete k;
    return nullptr;
  }
  return k;
}

void khh_kang_free(khh_kang* k) { delete k; }

int khh_kang_params(const khh_kang* k, uint32_t* dp_bits, uint64_t* herd, uint32_t* width_bits) {
  if (!k) return KHB_EINVAL;
  if (dp_bits) *dp_bits = k->S.dp_bits;
  if (herd) *herd = k->S.herd;
  if (width_bits) *width_bits = (uint32_t)k->S.w_bits;
  return KHB_OK;
}

int khh_kang_jumps(const khh_kang* k, uint8_t* dist_be, uint8_t* xy) {
  if (!k || !dist_be || !xy) return KHB_EINVAL;
  for (int j = 0; j < kKangJumps; ++j) {
    k->S.jump_s[j].to_be(dist_be + 32 * j);
    pt_to_be(xy + 64 * j, k->S.jump_p[j]);
  }
  return KHB_OK;
}

static void roos_to_be(const KangRoo* r, uint64_t n, uint8_t* xy, uint8_t* dist_be) {
  for (uint64_t i = 0; i < n; ++i) {
    pt_to_be(xy + 64 * i, r[i].p);
    r[i].d.to_be(dist_be + 32 * i);
  }
}

static std::vector<KangRoo> roos_from_be(const uint8_t* xy, const uint8_t* dist_be, uint64_t n) {
  std::vector<KangRoo> r(n);
  for (uint64_t i = 0; i < n; ++i) {
    r[i].p = pt_from_be(xy + 64 * i);
    r[i].d = U256::from_be(dist_be + 32 * i);
  }
  return r;
}

int khh_kang_make_herd(const khh_kang* k, uint32_t stream, uint64_t n, uint8_t* xy, uint8_t* dist_be) {
  if (!k || !xy || !dist_be) return KHB_EINVAL;
  for (uint64_t i = 0; i < n; ++i) {
    const KangRoo r = kang_make(k->S, stream, i, 0);
    roos_to_be(&r, 1, xy + 64 * i, dist_be + 32 * i);
  }
  return KHB_OK;
}

int khh_kang_cpu_walk(const khh_kang* k, uint8_t* xy, uint8_t* dist_be, uint64_t n, uint32_t steps, uint32_t dp_bits,
                      uint32_t* dp_kangaroo, uint8_t* dp_x_be, uint8_t* dp_dist_be, uint64_t cap, uint64_t* n_dp,
                      uint64_t* second_choice) {
  if (!k || !xy || !dist_be || n == 0 || steps == 0 || dp_bits > 32) return KHB_EINVAL;
  std::vector<KangRoo> herd = roos_from_be(xy, dist_be, n);
  std::vector<KangDp> dps;
  kang_cpu_walk(k->S, herd.data(), n, steps, dp_bits, dps, second_choice);
  roos_to_be(herd.data(), n, xy, dist_be);
  if (n_dp) *n_dp = dps.size();
  for (uint64_t i = 0; i < dps.size() && i < cap; ++i) {
    if (dp_kangaroo) dp_kangaroo[i] = dps[i].i;
    if (dp_x_be) dps[i].x.to_be(dp_x_be + 32 * i);
    if (dp_dist_be) dps[i].d.to_be(dp_dist_be + 32 * i);
  }
  return KHB_OK;
}

int khh_kang_set_ring_capacity(khh_kang* k, uint32_t cap) {
  if (!k) return KHB_EINVAL;
  k->S.ring_cap = cap;
  return KHB_OK;
}

int khh_kang_plant(khh_kang* k, const uint8_t* xy, const uint8_t* dist_be, uint64_t n) {
  if (!k || (n && (!xy || !dist_be)) || n > k->S.herd) return KHB_EINVAL;
  k->S.planted = roos_from_be(xy, dist_be, n);
  return KHB_OK;
}

int khh_kang_keep_herd(khh_kang* k, int keep) {
  if (!k) return KHB_EINVAL;
  k->S.keep_herd = keep != 0;
  return KHB_OK;
}

int khh_kang_final_herd(const khh_kang* k, uint8_t* xy, uint8_t* dist_be, uint64_t cap, uint64_t* n) {
  if (!k || !n) return KHB_EINVAL;
  *n = k->S.final_herd.size();
  if (xy && dist_be) roos_to_be(k->S.final_herd.data(), *n < cap ? *n : cap, xy, dist_be);
  return KHB_OK;
}

int khh_kang_search(khh_kang* k, const int* devices, int n_devices, uint64_t max_steps, uint8_t key_be[32],
                    int* found, uint64_t* stats_out, uint32_t stats_len, char* err, size_t errlen) {
  if (!k || !found || (n_devices > 0 && !devices)) return KHB_EINVAL;
  std::vector<int> devs(devices, devices + (n_devices > 0 ? n_devices : 0));
  KangResult R;
  std::string e;
  const int rc = kang_search(k->S, devs, max_steps, R, &e);
  *found = R.found ? 1 : 0;
  if (R.found && key_be) R.key.to_be(key_be);
  if (stats_out) {
    const uint64_t v[KHH_KANG_STATS] = {R.steps, R.dps, R.dead, R.lost_dps, R.launches, (uint64_t)(R.seconds * 1e6)};
    memcpy(stats_out, v, sizeof(uint64_t) * (stats_len < KHH_KANG_STATS ? stats_len : KHH_KANG_STATS));
  }
  if (rc) set_err(err, errlen, e);
  return rc;
}

void khh_hash160(const uint8_t xy[64], int compressed, uint8_t out[20]) {
  hash160_pub(pt_from_be(xy), compressed != 0, out);
}

void khh_rmd_to_address(const uint8_t rmd[20], char* out_addr) {
  const std::string s = rmd_to_address(rmd);
  memcpy(out_addr, s.c_str(), s.size() + 1);
}

}  // extern "C"
