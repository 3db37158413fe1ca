#include "kang_host.hpp"

#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <mutex>
#include <thread>

#include "../../../include/khbsgs.h"
#include "../device/fe.hpp"
#include "mini_table.hpp"

namespace khb {

namespace {

// splitmix64: the seeded generator of jump distances and herd distances.
struct KangRng {
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  U256 bits(int n) {      // uniform below 2^n, n <= 256
    U256 r;
    for (int i = 0; i < 4; ++i) r.w[i] = next();
    return n >= 256 ? r : r.shr(256 - n);
  }
  U256 below(const U256& bound) {      // uniform in [0, bound), bound != 0
    const int n = bound.bit_length();
    for (;;) {
      const U256 r = bits(n);
      if (r < bound) return r;
    }
  }
};

uint64_t mix(uint64_t a, uint64_t b) {
  KangRng r{a ^ (b * 0xD6E8FEB86659FD93ull)};
  r.next();
  return r.next();
}

U256 pow2(int n) { return U256(1).shl(n); }

// The distance of kangaroo i of herd `stream`, generation gen: tame ones in [W/2, W/2 + W), wild ones in [1, W).
U256 draw_distance(const KangSearch& S, uint32_t stream, uint64_t i, uint32_t gen) {
  KangRng r{mix(mix(S.seed, 0x4B414E47ull + stream), mix(i, gen))};
  if (i & 1) {
    for (;;) {
      const U256 d = r.below(S.width);
      if (!d.is_zero()) return d;
    }
  }
  return r.below(S.width) + S.width.shr(1);
}

// d*G as the kangaroo's point: itself for a tame one, Q + d*G for a wild one.  false: d*G = +-Q (redraw).
bool roo_point(const KangSearch& S, uint64_t i, const Pt& dG, Pt& out) {
  if (!S.q_infinity && fe_eq(dG.x, S.Q.x)) return false;
  out = (i & 1) && !S.q_infinity ? add_direct(S.Q, dG) : dG;
  return true;
}

Fe fe32_of(const Fh& f) {
  Fe r;
  for (int k = 0; k < 4; ++k) {
    r.v[2 * k] = (uint32_t)f.w[k];
    r.v[2 * k + 1] = (uint32_t)(f.w[k] >> 32);
  }
  return r;
}
Fh fh_of(const Fe& f) {
  Fh r;
  for (int k = 0; k < 4; ++k) r.w[k] = f.v[2 * k] | ((uint64_t)f.v[2 * k + 1] << 32);
  return r;
}

struct Shared {
  Shared(KangSearch& s, uint64_t max, KangResult& r) : S(s), max_steps(max), R(r) {}
  KangSearch& S;
  const uint64_t max_steps;
  std::mutex mu;
  KangDpTable table;
  KangResult& R;
  uint64_t claimed = 0;            // jumps submitted, all devices
  std::atomic<bool> stop{false};
  int rc = 0;
  std::string err;
  std::vector<uint8_t> mini_table;      // the device's k*G window table, built once
  std::once_flag mini_once;
};

// What walks a herd: a device context, or the CPU.
struct Backend {
  virtual ~Backend() {}
  int depth = 1;
  uint32_t ring = 0;
  virtual int make_herd(const KangSearch& S, uint32_t stream, std::vector<KangRoo>& herd) = 0;
  virtual int store(uint32_t first, const KangRoo* r, uint32_t n) = 0;
  virtual int read(std::vector<KangRoo>& herd) = 0;
  virtual int submit(uint32_t steps) = 0;
  virtual int collect(std::vector<KangDp>& dps, uint64_t& walked, uint64_t& n_dp) = 0;
};

struct CpuBackend : Backend {
  const KangSearch& S;
  std::vector<KangRoo> herd;
  uint32_t pending = 0;
  explicit CpuBackend(const KangSearch& s) : S(s) { ring = s.ring_cap ? s.ring_cap : 1u << 18; }
  int make_herd(const KangSearch& s, uint32_t stream, std::vector<KangRoo>& h) override {
    h.resize(s.herd);
    for (uint64_t i = 0; i < s.herd; ++i) h[i] = kang_make(s, stream, i, 0);
    return 0;
  }
  int store(uint32_t first, const KangRoo* r, uint32_t n) override {
    if (herd.size() < (size_t)first + n) herd.resize((size_t)first + n);
    std::copy(r, r + n, herd.begin() + first);
    return 0;
  }
  int read(std::vector<KangRoo>& h) override {
    h = herd;
    return 0;
  }
  int submit(uint32_t steps) override {
    pending = steps;
    return 0;
  }
  int collect(std::vector<KangDp>& dps, uint64_t& walked, uint64_t& n_dp) override {
    dps.clear();
    kang_cpu_walk(S, herd.data(), herd.size(), pending, S.dp_bits, dps, nullptr);
    walked = (uint64_t)herd.size() * pending;
    n_dp = dps.size();
    if (dps.size() > ring) dps.resize(ring);      // as a full ring on the device
    return 0;
  }
};

struct DevBackend : Backend {
  Shared& H;
  khb_ctx* ctx = nullptr;
  std::vector<khb_kang_dp> raw;
  explicit DevBackend(Shared& h) : H(h) { depth = 2; }
  ~DevBackend() override { khb_close(ctx); }
  int open(int device) {
    int rc = khb_open(device, 0, &ctx);
    if (rc) return rc;
    const KangSearch& S = H.S;
    uint8_t dist[32 * kKangJumps], xy[64 * kKangJumps];
    for (int j = 0; j < kKangJumps; ++j) {
      S.jump_s[j].to_be(dist + 32 * j);
      pt_to_be(xy + 64 * j, S.jump_p[j]);
    }
    if ((rc = khb_kang_load_jumps(ctx, dist, xy))) return rc;
    // the ring: four times the points a one-step launch is expected to report, within [2^18, 2^24] entries
    uint64_t want = S.ring_cap;
    if (!want) {
      want = 1u << 18;
      const uint64_t per_step = S.dp_bits >= 63 ? 0 : S.herd >> S.dp_bits;
      while (want < 4 * per_step && want < (1u << 24)) want <<= 1;
    }
    ring = (uint32_t)want;
    raw.resize(ring);
    return khb_kang_set_ring_capacity(ctx, ring);
  }
  // d*G of the whole herd by the device's fixed-base multiplication, then Q added to the wild ones on the host with
  // one batch inversion.
  int make_herd(const KangSearch& S, uint32_t stream, std::vector<KangRoo>& herd) override {
    std::call_once(H.mini_once, [&] { H.mini_table = mini_table_be(8, 8); });
    int rc = khb_load_mini_table(ctx, H.mini_table.data(), 8);
    if (rc) return rc;
    const uint32_t n = (uint32_t)S.herd;
    herd.resize(n);
    std::vector<uint8_t> ks(32 * (size_t)n), xy(64 * (size_t)n), bad(n);
    for (uint32_t i = 0; i < n; ++i) {
      herd[i].d = draw_distance(S, stream, i, 0);
      herd[i].d.to_be(ks.data() + 32 * (size_t)i);
    }
    if ((rc = khb_mini_pubkey(ctx, ks.data(), xy.data(), bad.data(), n))) return rc;
    std::vector<Fh> dx(n), scratch(n);
    for (uint32_t i = 0; i < n; ++i) {
      herd[i].p = pt_from_be(xy.data() + 64 * (size_t)i);
      dx[i] = fh_small(0);
      if ((i & 1) && !S.q_infinity && !bad[i]) fe_sub(dx[i], herd[i].p.x, S.Q.x);
    }
    fe_batch_inv(dx.data(), n, scratch.data());
    for (uint32_t i = 0; i < n; ++i) {
      const Pt g = herd[i].p;
      if (bad[i] || (!S.q_infinity && fe_eq(g.x, S.Q.x))) {      // d*G = +-Q (or no point): a fresh draw on the host
        herd[i] = kang_make(S, stream, i, 1);
        continue;
      }
      if (!(i & 1) || S.q_infinity) continue;
      Fh s, x3, t;                                                // Q + g with 1 / (g.x - Q.x)
      fe_sub(s, g.y, S.Q.y);
      fe_mul(s, s, dx[i]);
      fe_sqr(x3, s);
      fe_sub(x3, x3, S.Q.x);
      fe_sub(x3, x3, g.x);
      fe_sub(t, S.Q.x, x3);
      fe_mul(t, t, s);
      fe_sub(t, t, S.Q.y);
      herd[i].p = Pt{x3, t};
    }
    return 0;
  }
  int store(uint32_t first, const KangRoo* r, uint32_t n) override {
    std::vector<uint8_t> xy(64 * (size_t)n), d(32 * (size_t)n);
    for (uint32_t i = 0; i < n; ++i) {
      pt_to_be(xy.data() + 64 * (size_t)i, r[i].p);
      r[i].d.to_be(d.data() + 32 * (size_t)i);
    }
    return khb_kang_store(ctx, first, n, xy.data(), d.data());
  }
  int read(std::vector<KangRoo>& herd) override {
    const uint32_t n = khb_kang_herd(ctx);
    std::vector<uint8_t> xy(64 * (size_t)n), d(32 * (size_t)n);
    const int rc = khb_kang_read(ctx, 0, n, xy.data(), d.data());
    herd.resize(rc ? 0 : n);
    for (size_t i = 0; i < herd.size(); ++i) {
      herd[i].p = pt_from_be(xy.data() + 64 * i);
      herd[i].d = U256::from_be(d.data() + 32 * i);
    }
    return rc;
  }
  int submit(uint32_t steps) override { return khb_kang_submit(ctx, steps, H.S.dp_bits); }
  int collect(std::vector<KangDp>& dps, uint64_t& walked, uint64_t& n_dp) override {
    khb_kang_stats st{};
    const int rc = khb_kang_collect(ctx, raw.data(), (uint32_t)raw.size(), &st);
    if (rc) return rc;
    walked = st.steps_walked;
    n_dp = st.n_dp;
    const size_t take = (size_t)std::min<uint64_t>(st.n_dp, raw.size());
    dps.resize(take);
    for (size_t i = 0; i < take; ++i) {
      dps[i].i = raw[i].kangaroo;
      dps[i].x = U256::from_be(raw[i].x_be);
      dps[i].d = U256::from_be(raw[i].dist_be);
    }
    return 0;
  }
};

// A tame and a wild kangaroo on one x: the two keys that explains, each verified.
bool solve(const KangSearch& S, const U256& d_tame, const U256& d_wild, U256& key) {
  const U256 cand[2] = {kang_sub_mod_n(d_tame, d_wild), kang_neg_mod_n(kang_add_mod_n(d_tame, d_wild))};
  for (const U256& c : cand) {
    const U256 k = kang_add_mod_n(S.start, c);
    if (k.is_zero()) continue;
    const Pt p = mul_g(k);
    if (fe_eq(p.x, S.pub.x) && fe_eq(p.y, S.pub.y)) {
      key = k;
      return true;
    }
  }
  return false;
}

void fail(Shared& H, int rc, const char* what) {
  std::lock_guard<std::mutex> lk(H.mu);
  if (!H.rc) {
    H.rc = rc;
    H.err = std::string(what) + ": " + khb_strerror(rc);
  }
  H.stop = true;
}

// One herd's loop: keep `depth` launches in flight, digest each launch's points into the shared table, replace the
// kangaroos that merged (behind the launches in flight, whose points of a replaced kangaroo are digested first), and
// halve the launch after one that overflowed its ring.
void herd_loop(Shared& H, Backend& B, uint32_t stream) {
  KangSearch& S = H.S;
  std::vector<KangRoo> herd;
  int rc = B.make_herd(S, stream, herd);
  if (rc) return fail(H, rc, "herd");
  if (stream == 0)
    for (size_t i = 0; i < S.planted.size() && i < herd.size(); ++i) herd[i] = S.planted[i];
  if ((rc = B.store(0, herd.data(), (uint32_t)herd.size()))) return fail(H, rc, "khb_kang_store");
  const uint64_t n = herd.size();
  herd = std::vector<KangRoo>();
  // expected points per launch at most a quarter of the ring; at most 2,048 steps, so the host looks in often
  uint64_t steps = S.dp_bits >= 40 ? 2048 : std::min<uint64_t>(2048, (((uint64_t)B.ring / 4) << S.dp_bits) / n);
  // and a launch at most an eighth of the 2 sqrt(W) jumps expected in all, so a short search is not one long launch
  steps = std::min<uint64_t>(steps, (1ull << std::min(62, std::max(0, S.w_bits / 2 - 2))) / n);
  if (steps == 0) steps = 1;
  std::vector<uint32_t> gen(n, 0), dead;
  std::vector<uint8_t> is_dead(n, 0);
  std::vector<KangDp> dps;
  int inflight = 0;
  auto claim = [&]() -> uint32_t {      // the next launch's steps within max_steps; 0 = none left
    std::lock_guard<std::mutex> lk(H.mu);
    uint64_t s = steps;
    if (H.max_steps) {
      const uint64_t left = H.max_steps > H.claimed ? H.max_steps - H.claimed : 0;
      s = std::min(s, left / n);
    }
    H.claimed += s * n;
    return (uint32_t)s;
  };
  auto digest = [&]() -> int {
    uint64_t walked = 0, n_dp = 0;
    const int crc = B.collect(dps, walked, n_dp);
    --inflight;
    if (crc) return crc;
    std::lock_guard<std::mutex> lk(H.mu);
    H.R.launches++;
    H.R.steps += walked;
    H.R.dps += dps.size();
    if (n_dp > dps.size()) {
      H.R.lost_dps += n_dp - dps.size();
      steps = std::max<uint64_t>(1, steps / 2);
    }
    for (const KangDp& p : dps) {
      const uint32_t kind = p.i & 1;
      const KangEntry* e = H.table.insert(p.x, p.d, kind);
      if (!e) continue;
      if (e->kind != kind) {
        U256 key;
        if (!H.R.found && solve(S, kind ? e->d : p.d, kind ? p.d : e->d, key)) {
          H.R.found = true;
          H.R.key = key;
          H.stop = true;
        }
      } else if (p.i < n && !is_dead[p.i]) {      // merged with an earlier kangaroo of its kind
        is_dead[p.i] = 1;
        dead.push_back(p.i);
      }
    }
    return 0;
  };
  bool out_of_steps = false;
  while (!H.stop && !out_of_steps) {
    while (inflight < B.depth && !H.stop) {
      const uint32_t s = claim();
      if (!s) {
        out_of_steps = true;
        break;
      }
      if ((rc = B.submit(s))) return fail(H, rc, "khb_kang_submit");
      ++inflight;
    }
    if (!inflight) break;
    if ((rc = digest())) return fail(H, rc, "khb_kang_collect");
    if (!dead.empty() && !H.stop) {
      while (inflight)
        if ((rc = digest())) return fail(H, rc, "khb_kang_collect");
      for (const uint32_t i : dead) {
        const KangRoo fresh = kang_make(S, stream, i, ++gen[i]);
        if ((rc = B.store(i, &fresh, 1))) return fail(H, rc, "khb_kang_store");
        is_dead[i] = 0;
      }
      std::lock_guard<std::mutex> lk(H.mu);
      H.R.dead += dead.size();
      dead.clear();
    }
  }
  while (inflight)
    if ((rc = digest())) return fail(H, rc, "khb_kang_collect");
  if (stream == 0 && S.keep_herd && (rc = B.read(S.final_herd))) fail(H, rc, "khb_kang_read");
}

}  // namespace

bool kang_init(KangSearch& S, const Pt& pub, const U256& start, const U256& end, int dp_bits, uint64_t herd,
               uint64_t seed, uint64_t herd_cap, std::string* err) {
  auto bad = [&](const char* m) {
    if (err) *err = m;
    return false;
  };
  if (!on_curve(pub)) return bad("the public key is not a point of the curve");
  if (!(start < end) || end > secp_order()) return bad("the interval is start < end <= n");
  S.pub = pub;
  S.start = start;
  S.end = end;
  S.width = end - start;
  S.w_bits = S.width.bit_length();
  if (S.width < pow2(kKangMinBits) || S.width > pow2(kKangMaxBits))
    return bad("the interval's width must be between 2^16 and 2^200");
  if (dp_bits > 32) return bad("dp_bits: 0 to 32");
  if (herd > (1ull << 30)) return bad("herd: at most 2^30 kangaroos per device");
  S.seed = seed;
  // Q = P - start*G
  S.q_infinity = false;
  if (start.is_zero()) {
    S.Q = pub;
  } else {
    const Pt sG = mul_g(start);
    if (fe_eq(sG.x, pub.x)) {
      if (!fe_eq(sG.y, pub.y)) return bad("the public key is the negative of start*G: its key is outside the interval");
      S.q_infinity = true;
      S.Q = pub;
    } else {
      S.Q = add_direct(pub, negation(sG));
    }
  }
  // the jumps: distances in [1, 2^(ceil(w / 2) + 1)), redrawn until the 32 x are distinct
  const int jbits = (S.w_bits + 1) / 2 + 1;
  KangRng r{mix(seed, 0x4A554D50ull)};
  for (int j = 0; j < kKangJumps;) {
    const U256 s = r.bits(jbits);
    if (s.is_zero()) continue;
    const Pt p = mul_g(s);
    bool dup = false;
    for (int i = 0; i < j; ++i) dup = dup || fe_eq(S.jump_p[i].x, p.x);
    if (dup) continue;
    S.jump_s[j] = s;
    S.jump_p[j] = p;
    ++j;
  }
  // defaults: herd * 2^dp <= 2^(floor(w / 2) - 2)
  const int budget = S.w_bits / 2 - 2;
  if (herd_cap == 0) herd_cap = 1;
  if (herd == 0) {
    herd = budget >= 40 ? herd_cap : std::min<uint64_t>(herd_cap, 1ull << budget);
    if (dp_bits >= 0 && budget - dp_bits < 40) herd = std::min<uint64_t>(herd, 1ull << std::max(budget - dp_bits, 1));
  }
  if (herd < 2) herd = 2;                        // a tame and a wild one
  if (dp_bits < 0) {
    int hb = 0;
    while ((1ull << hb) < herd) ++hb;
    dp_bits = std::min(32, std::max(0, budget - hb));
  }
  S.herd = herd;
  S.dp_bits = (uint32_t)dp_bits;
  return true;
}

KangRoo kang_make(const KangSearch& S, uint32_t stream, uint64_t i, uint32_t gen) {
  for (;; ++gen) {
    KangRoo r;
    r.d = draw_distance(S, stream, i, gen);
    if (roo_point(S, i, mul_g(r.d), r.p)) return r;
  }
}

void kang_cpu_walk(const KangSearch& S, KangRoo* herd, uint64_t n, uint32_t steps, uint32_t dp_bits,
                   std::vector<KangDp>& dps, uint64_t* second_choice) {
  Fe jx[kKangJumps], jy[kKangJumps];
  for (int j = 0; j < kKangJumps; ++j) {
    jx[j] = fe32_of(S.jump_p[j].x);
    jy[j] = fe32_of(S.jump_p[j].y);
  }
  const uint32_t dp_mask = dp_bits >= 32 ? 0xFFFFFFFFu : (1u << dp_bits) - 1u;
  std::vector<Fe> x(n), y(n), pre(n);
  std::vector<uint8_t> pick(n);
  for (uint64_t i = 0; i < n; ++i) {
    x[i] = fe32_of(herd[i].p.x);
    y[i] = fe32_of(herd[i].p.y);
  }
  uint64_t seconds = 0;
  for (uint32_t t = 0; t < steps; ++t) {
    Fe acc;
    for (uint64_t i = 0; i < n; ++i) {
      uint32_t j = x[i].v[0] & 31u;
      if (fe_eq(x[i], jx[j])) {
        j = (j + 1) & 31u;
        ++seconds;
      }
      pick[i] = (uint8_t)j;
      Fe dx;
      fe_sub(dx, jx[j], x[i]);
      if (i == 0) acc = dx; else fe_mul(acc, acc, dx);
      pre[i] = acc;
    }
    Fe inv;
    fe_inv(inv, acc);
    for (uint64_t i = n; i-- > 0;) {
      const uint32_t j = pick[i];
      Fe is = inv;
      if (i > 0) {
        Fe dx;
        fe_sub(dx, jx[j], x[i]);
        fe_mul(is, inv, pre[i - 1]);
        fe_mul(inv, inv, dx);
      }
      Fe s, x3, yy;
      fe_sub(s, jy[j], y[i]);
      fe_mul(s, s, is);
      fe_sqr(x3, s);
      fe_sub(x3, x3, x[i]);
      fe_sub(x3, x3, jx[j]);
      fe_sub(yy, jx[j], x3);
      fe_mul(yy, yy, s);
      fe_sub(yy, yy, jy[j]);
      x[i] = x3;
      y[i] = yy;
      herd[i].d = herd[i].d + S.jump_s[j];      // a plain 256-bit add
    }
    for (uint64_t i = 0; i < n; ++i)
      if ((x[i].v[1] & dp_mask) == 0) dps.push_back(KangDp{(uint32_t)i, u256_of(fh_of(x[i])), herd[i].d});
  }
  for (uint64_t i = 0; i < n; ++i) herd[i].p = Pt{fh_of(x[i]), fh_of(y[i])};
  if (second_choice) *second_choice = seconds;
}

int kang_search(KangSearch& S, const std::vector<int>& devices, uint64_t max_steps, KangResult& R, std::string* err) {
  R = KangResult();
  S.final_herd.clear();
  if (S.herd == 0) {
    if (err) *err = "no search";
    return KHB_EINVAL;
  }
  Shared H(S, max_steps, R);
  const auto t0 = std::chrono::steady_clock::now();
  if (devices.empty()) {
    CpuBackend B(S);
    herd_loop(H, B, 0);
  } else {
    std::vector<std::thread> th;
    for (size_t k = 0; k < devices.size(); ++k)
      th.emplace_back([&H, k, dev = devices[k]] {
        DevBackend B(H);
        const int rc = B.open(dev);
        if (rc) return fail(H, rc, "khb_open");
        herd_loop(H, B, (uint32_t)k);
      });
    for (auto& t : th) t.join();
  }
  R.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  if (H.rc && err) *err = H.err;
  return H.rc;
}

}  // namespace khb
