#include "mini_host.hpp"

#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <mutex>
#include <thread>

#include "../../../include/khbsgs.h"
#include "pipeline.hpp"

namespace khb {

const char kMiniDefaultAlphabet[59] = "123456789ABCDEFGHJKLMNPQRSTUVWXYZabcdefghijkmnopqrstuvwxyz";

bool MiniAlphabet::set(const uint8_t* a) {
  if (!a) a = (const uint8_t*)kMiniDefaultAlphabet;
  memset(digit, -1, sizeof digit);
  for (int i = 0; i < 58; ++i) {
    if (a[i] == 0 || digit[a[i]] >= 0) return false;
    digit[a[i]] = (int8_t)i;
    chars[i] = a[i];
  }
  return true;
}

bool mini_parse(const MiniAlphabet& A, const char* s, size_t len, MiniDigits& out, std::string* err) {
  auto bad = [&](const char* m) {
    if (err) *err = m;
    return false;
  };
  if (!s || len != (size_t)kMiniLen) return bad("a minikey has 22 characters");
  if (s[0] != 'S') return bad("a minikey begins with 'S'");
  for (int i = 0; i < kMiniDigitCount; ++i) {
    const int d = A.digit[(uint8_t)s[i + 1]];
    if (d < 0) return bad("a minikey character is outside the alphabet");
    out[i] = (uint8_t)d;
  }
  return true;
}

bool mini_advance(MiniDigits& d, uint64_t off) {
  uint64_t c = off;
  for (int i = kMiniDigitCount - 1; i >= 0 && c; --i) {
    uint64_t q = c / 58;
    uint32_t s = (uint32_t)(c % 58) + d[i];
    if (s >= 58) {
      s -= 58;
      q += 1;
    }
    d[i] = (uint8_t)s;
    c = q;
  }
  return c == 0;
}

void mini_string(const MiniAlphabet& A, const MiniDigits& d, char out[kMiniLen]) {
  out[0] = 'S';
  for (int i = 0; i < kMiniDigitCount; ++i) out[i + 1] = (char)A.chars[d[i]];
}

bool mini_is_valid(const char s[kMiniLen]) {
  uint8_t m[kMiniLen + 1], h[32];
  memcpy(m, s, kMiniLen);
  m[kMiniLen] = '?';
  sha256(m, sizeof m, h);
  return h[0] == 0;
}

void mini_key_of(const char s[kMiniLen], uint8_t out[32]) { sha256((const uint8_t*)s, kMiniLen, out); }

namespace {

struct MiniShared {
  const MiniSearch& M;
  const MiniDigits first;
  const uint64_t count;
  const MiniConfig& cfg;
  const std::function<void(const MiniFound&)>& on_found;
  MiniStats& stats;
  uint64_t cursor = 0;                 // offset of the next unclaimed candidate
  std::mutex mu;
  std::string err;
  int rc = 0;
};

// One launch: the candidates [off, off + n) of the span.  Its group fields are not used.
struct MBatch : BatchRange {
  uint64_t off = 0, n = 0;
  size_t jobs() const { return 1; }
  void slice(size_t, size_t, MBatch& o) const { o.off = off; o.n = n; }
};

// One device's side of the launch pipeline (pipeline.hpp run_pipeline) at depth 1: a context keeps one -m minikeys
// launch in flight.  A launch that overflowed the survivor queue or the hit ring is rescanned in two halves, ahead of
// new spans; only launches that did not overflow are counted, so every candidate is counted once.
struct MiniOps {
  MiniShared& S;
  khb_ctx* ctx;
  std::vector<khb_mini_hit> hits{};
  khb_mini_stats st{};
  static constexpr bool drop_on_stop = true;

  int fail(int code, const char* what) {
    std::lock_guard<std::mutex> lk(S.mu);
    if (!S.rc) {
      S.rc = code;
      S.err = std::string(what) + ": " + khb_strerror(code);
    }
    return code;
  }
  bool stopped() { return false; }
  bool fresh(MBatch& b) {
    std::lock_guard<std::mutex> lk(S.mu);
    if (S.rc || S.cursor >= S.count) return false;
    b.off = S.cursor;
    b.n = std::min<uint64_t>(S.cfg.per_launch, S.count - S.cursor);
    S.cursor += b.n;
    return true;
  }
  int submit(const MBatch& b) {
    MiniDigits d = S.first;
    if (!mini_advance(d, b.off)) return fail(KHB_EINVAL, "khb_mini_submit");
    const int rc = khb_mini_submit(ctx, d.data(), b.n, S.M.A.chars);
    return rc ? fail(rc, "khb_mini_submit") : 0;
  }
  int collect() {
    st = khb_mini_stats{};
    const int rc = khb_mini_collect(ctx, hits.data(), (uint32_t)hits.size(), &st);
    return rc ? fail(rc, "khb_mini_collect") : 0;
  }
  int done(const MBatch& b, MBatch& lo, MBatch& hi) {
    if (st.queue_overflow || st.hit_overflow || st.hits > hits.size()) {
      if (b.n < 2)
        return fail(-100, "a single candidate overflowed a queue (capacity 0?)");
      lo.off = b.off;
      lo.n = b.n / 2;
      hi.off = b.off + lo.n;
      hi.n = b.n - lo.n;
      lo.part = hi.part = true;
      std::lock_guard<std::mutex> lk(S.mu);
      S.stats.launches++;
      S.stats.rescans++;
      return kRescan;
    }
    const uint32_t nh = (uint32_t)st.hits;
    std::sort(hits.begin(), hits.begin() + nh,
              [](const khb_mini_hit& x, const khb_mini_hit& y) { return x.offset < y.offset; });
    std::vector<MiniFound> found;
    for (uint32_t h = 0; h < nh; ++h) {
      MiniDigits d = S.first;
      if (!mini_advance(d, b.off + hits[h].offset)) continue;
      MiniFound f;
      mini_string(S.M.A, d, f.minikey);
      if (!mini_is_valid(f.minikey)) continue;
      uint8_t kb[32];
      mini_key_of(f.minikey, kb);
      f.key = U256::from_be(kb);
      if (f.key.is_zero() || f.key >= secp_order()) continue;
      hash160_pub(mul_g(f.key), false, f.rmd.data());
      if (S.M.T.searchbinary(f.rmd.data())) found.push_back(f);     // else a bloom false positive
    }
    std::lock_guard<std::mutex> lk(S.mu);
    S.stats.launches++;
    S.stats.candidates += st.candidates;
    S.stats.valid += st.valid;
    S.stats.bad_keys += st.bad_keys;
    S.stats.hits += st.hits;
    if (st.filter_ms > 0) S.stats.filter_seconds += st.filter_ms * 1e-3;
    if (st.keys_ms > 0) S.stats.keys_seconds += st.keys_ms * 1e-3;
    S.stats.found += found.size();
    if (S.on_found)
      for (const MiniFound& f : found) S.on_found(f);
    return 0;
  }
};

void mini_device_loop(MiniShared& S, int device) {
  MiniOps ops{S, nullptr};
  khb_ctx*& ctx = ops.ctx;
  int rc = khb_open(device, S.cfg.lanes, &ctx);
  if (rc) { ops.fail(rc, "khb_open"); return; }
  const BloomGeom bg = S.M.T.bloom.geom();
  if ((S.cfg.hit_cap && (rc = khb_set_candidate_capacity(ctx, S.cfg.hit_cap))) ||
      (rc = khb_mini_set_queue_capacity(ctx, S.cfg.queue_cap)) ||
      (rc = khb_load_mini_table(ctx, S.M.table.data(), S.M.window_bits)) ||
      (rc = khb_load_addr_bloom(ctx, S.M.T.bloom.bf.data(), bg.bytes_per_sub, bg.bits, bg.hashes))) {
    ops.fail(rc, "table upload");
  } else {
    ops.hits.resize(khb_addr_hit_capacity(ctx));
    run_pipeline<MBatch>(ops, 1);
  }
  khb_close(ctx);
}

}  // namespace

int mini_search(const MiniSearch& M, const MiniDigits& first, uint64_t count, const MiniConfig& cfg,
                const std::function<void(const MiniFound&)>& on_found, MiniStats* stats, std::string* err) {
  MiniStats local;
  MiniStats& st = stats ? *stats : local;
  st = MiniStats();
  auto bad = [&](const char* m) {
    if (err) *err = m;
    return KHB_EINVAL;
  };
  if (M.T.kind != kTargetsBtc) return bad("minikeys are searched against BTC hash160 targets");
  if (M.table.empty()) return bad("no window table");
  if (count == 0) return bad("count must be positive");
  if (cfg.per_launch == 0 || cfg.per_launch > (1ull << 32)) return bad("per_launch: 1 to 2^32 candidates");
  for (int i = 0; i < kMiniDigitCount; ++i)
    if (first[i] >= 58) return bad("digits are below 58");
  MiniDigits last = first;
  if (!mini_advance(last, count - 1)) return bad("first + count exceeds 58^21: a span does not wrap");
  MiniShared S{M, first, count, cfg, on_found, st, 0, {}, {}, 0};
  std::vector<std::thread> th;
  for (int d : cfg.devices) th.emplace_back(mini_device_loop, std::ref(S), d);
  for (auto& t : th) t.join();
  if (S.rc && err) *err = S.err;
  return S.rc;
}

double mini_cpu_scan(const MiniSearch& M, const MiniDigits& first, uint64_t count, int threads, uint64_t* valid,
                     uint64_t* found) {
  if (threads < 1) threads = 1;
  std::atomic<uint64_t> nv{0}, nf{0};
  auto work = [&](uint64_t off, uint64_t n) {
    MiniDigits d = first;
    if (!mini_advance(d, off)) return;
    uint64_t v = 0, f = 0;
    uint8_t msg[kMiniLen + 1], h[32], rmd[20];
    msg[kMiniLen] = '?';
    for (uint64_t i = 0; i < n; ++i) {
      mini_string(M.A, d, (char*)msg);
      sha256(msg, sizeof msg, h);
      if (h[0] == 0) {
        ++v;
        sha256(msg, kMiniLen, h);
        const U256 k = U256::from_be(h);
        if (!k.is_zero() && k < secp_order()) {
          hash160_pub(mul_g(k), false, rmd);
          if (M.T.bloom.check20(rmd) && M.T.searchbinary(rmd)) ++f;
        }
      }
      mini_advance(d, 1);
    }
    nv += v;
    nf += f;
  };
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<std::thread> th;
  const uint64_t per = (count + threads - 1) / threads;
  for (int t = 0; t < threads; ++t) {
    const uint64_t off = per * t;
    if (off >= count) break;
    th.emplace_back(work, off, std::min(per, count - off));
  }
  for (auto& t : th) t.join();
  const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  if (valid) *valid = nv;
  if (found) *found = nf;
  return dt;
}

}  // namespace khb
