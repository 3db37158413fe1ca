#include "address_host.hpp"

#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <thread>

#include "../../../include/khbsgs.h"
#include "../device/hash160.hpp"
#include "../device/keccak.hpp"
#include "pipeline.hpp"

namespace khb {

using namespace khbk;   // SearchMode and its decoder (device/scan_modes.hpp)

// ------------------------------------------------------------------------------- hashing
void sha256(const uint8_t* msg, size_t len, uint8_t out[32]) {
  uint32_t s[8], w[16];
  sha256_init(s);
  uint8_t blk[128];
  size_t i = 0;
  auto load = [&](const uint8_t* b) {
    for (int k = 0; k < 16; ++k)
      w[k] = ((uint32_t)b[4 * k] << 24) | ((uint32_t)b[4 * k + 1] << 16) | ((uint32_t)b[4 * k + 2] << 8) | b[4 * k + 3];
  };
  for (; i + 64 <= len; i += 64) {
    load(msg + i);
    sha256_block(s, w);
  }
  const size_t rem = len - i;
  memset(blk, 0, sizeof blk);
  memcpy(blk, msg + i, rem);
  blk[rem] = 0x80;
  const size_t total = rem >= 56 ? 128 : 64;
  const uint64_t bits = (uint64_t)len * 8;
  for (int k = 0; k < 8; ++k) blk[total - 1 - k] = (uint8_t)(bits >> (8 * k));
  for (size_t o = 0; o < total; o += 64) {
    load(blk + o);
    sha256_block(s, w);
  }
  for (int k = 0; k < 8; ++k) {
    out[4 * k] = (uint8_t)(s[k] >> 24); out[4 * k + 1] = (uint8_t)(s[k] >> 16);
    out[4 * k + 2] = (uint8_t)(s[k] >> 8); out[4 * k + 3] = (uint8_t)s[k];
  }
}

static void fe_of_pt(Fe& x, Fe& y, const Pt& p) {
  uint8_t b[64];
  pt_to_be(b, p);
  fe_from_be(x, b);
  fe_from_be(y, b + 32);
}

static void bytes_of_words(uint8_t out[20], const uint32_t h[5]) {
  for (int k = 0; k < 5; ++k)
    for (int b = 0; b < 4; ++b) out[4 * k + b] = (uint8_t)(h[k] >> (8 * b));
}

void hash160_pub(const Pt& p, bool compressed, uint8_t out[20]) {
  Fe x, y;
  fe_of_pt(x, y, p);
  uint32_t h[5];
  if (compressed)
    hash160_compressed(h, (y.v[0] & 1) ? 3u : 2u, x);
  else
    hash160_uncompressed(h, x, y);
  bytes_of_words(out, h);
}

void hash160_x(uint8_t prefix, const Pt& p, uint8_t out[20]) {
  Fe x, y;
  fe_of_pt(x, y, p);
  uint32_t h[5];
  hash160_compressed(h, prefix, x);
  bytes_of_words(out, h);
}

void eth_address_xy(const uint8_t xy[64], uint8_t out[20]) {
  Fe x, y;
  fe_from_be(x, xy);
  fe_from_be(y, xy + 32);
  uint32_t h[5];
  eth_address(h, x, y);
  bytes_of_words(out, h);
}

void eth_address_pub(const Pt& p, uint8_t out[20]) {
  uint8_t b[64];
  pt_to_be(b, p);
  eth_address_xy(b, out);
}

// -------------------------------------------------------------------------------- base58
static const char kB58[] = "123456789ABCDEFGHJKLMNPQRSTUVWXYZabcdefghijkmnopqrstuvwxyz";

int b58_digit(unsigned char c) {
  if (!c || (c & 0x80)) return -1;
  const char* p = strchr(kB58, c);
  return p ? (int)(p - kB58) : -1;
}

bool b58decode25(const char* s, uint8_t out[25]) {
  const size_t n = strlen(s);
  size_t i = 0, zeros = 0;
  memset(out, 0, 25);
  for (; i < n && s[i] == '1'; ++i) ++zeros;
  for (; i < n; ++i) {
    const int v = b58_digit((unsigned char)s[i]);
    if (v < 0) return false;
    uint32_t carry = (uint32_t)v;
    for (int k = 24; k >= 0; --k) {
      const uint32_t t = (uint32_t)out[k] * 58u + carry;
      out[k] = (uint8_t)t;
      carry = t >> 8;
    }
    if (carry) return false;   // "Output number too big"
  }
  size_t lz = 0;
  while (lz < 25 && out[lz] == 0) ++lz;
  return 25 - lz + zeros == 25;  // keyhunt.cpp:6338: raw_value_length == 25
}

std::string rmd_to_address(const uint8_t rmd[20]) {
  uint8_t d[25], h1[32], h2[32];
  d[0] = 0x00;   // byte_encode_crypto (P2PKH)
  memcpy(d + 1, rmd, 20);
  sha256(d, 21, h1);
  sha256(h1, 32, h2);
  memcpy(d + 21, h2, 4);
  size_t zc = 0;
  while (zc < 25 && !d[zc]) ++zc;
  const size_t size = (25 - zc) * 138 / 100 + 1;   // b58enc (base58.c:145-189)
  std::vector<uint8_t> buf(size, 0);
  size_t high = size - 1, j = 0;
  for (size_t i = zc; i < 25; ++i, high = j) {
    int carry = d[i];
    for (j = size - 1; (j > high) || carry; --j) {
      carry += 256 * buf[j];
      buf[j] = (uint8_t)(carry % 58);
      carry /= 58;
      if (!j) break;
    }
  }
  for (j = 0; j < size && !buf[j]; ++j) {}
  std::string out(zc, '1');
  for (; j < size; ++j) out += kB58[buf[j]];
  return out;
}

// ------------------------------------------------------------------------------- targets
// The line as a C string (up to an embedded NUL) without its leading and trailing whitespace.
static std::string trimmed(const std::string& line) {
  const char* seps = " \t\n\r";
  const std::string s(line.c_str());
  const size_t b = s.find_first_not_of(seps);
  return b == std::string::npos ? std::string() : s.substr(b, s.find_last_not_of(seps) - b + 1);
}

static bool all_b58(const char* s) {
  for (; *s; ++s)
    if (b58_digit((unsigned char)*s) < 0) return false;
  return true;
}

static bool all_hex(const char* s) {
  for (; *s; ++s) {
    const char c = *s;
    if (!((c >= '0' && c <= '9') || (c >= 'a' && c <= 'f') || (c >= 'A' && c <= 'F'))) return false;
  }
  return true;
}

static int hexv(char c) { return c <= '9' ? c - '0' : (c | 32) - 'a' + 10; }

// Split like fgets(aux, size, f): a line longer than size - 1 characters continues in the next read.
static std::vector<std::string> fgets_lines(const std::string& text, size_t size) {
  std::vector<std::string> out;
  size_t p = 0;
  while (p < text.size()) {
    size_t e = text.find('\n', p);
    size_t len = (e == std::string::npos ? text.size() : e + 1) - p;
    if (len > size - 1) len = size - 1;
    out.push_back(text.substr(p, len));
    p += len;
  }
  return out;
}

static void hex20(const char* hex, H160& h) {
  for (int k = 0; k < 20; ++k) h[k] = (uint8_t)(hexv(hex[2 * k]) * 16 + hexv(hex[2 * k + 1]));
}

// One trimmed target line to its 20 bytes; false: "Ommiting invalid line".
static bool line_h160(TargetKind kind, const std::string& aux, H160& h) {
  const size_t r = aux.size();
  if (kind == kTargetsXpoint) {
    // stringtokenizer (util.c:67-84): trim "\t\n\r :", then the first strtok(" \t:") token: 64 hex = x, 66 hex = a
    // compressed key (prefix unchecked), 130 hex = 04 || x || y: x[0..19] for bloom and table (see address_host.hpp)
    const size_t t0 = std::min(aux.find_first_not_of(" \t:"), r);
    const std::string token = aux.substr(t0, aux.find_first_of(" \t:", t0) - t0);
    const size_t n = token.size();
    if ((n != 64 && n != 66 && n != 130) || !all_hex(token.c_str())) return false;
    hex20(token.c_str() + (n == 64 ? 0 : 2), h);
    return true;
  }
  if (kind == kTargetsEth) {
    // a 40-character line must be hex, a 42-character line hex from its third character (the two leading characters
    // are not looked at); hexs2bin takes either letter case
    const char* hex = r == 40 ? aux.c_str() : r == 42 ? aux.c_str() + 2 : nullptr;
    if (!hex || !all_hex(hex)) return false;
    hex20(hex, h);
    return true;
  }
  if (r == 40 && all_hex(aux.c_str())) {   // -m rmd160: the hash160 itself
    hex20(aux.c_str(), h);
    return true;
  }
  uint8_t raw[25];
  if (r == 0 || r >= 40 || !all_b58(aux.c_str()) || !b58decode25(aux.c_str(), raw)) return false;
  memcpy(h.data(), raw + 1, 20);
  return true;
}

// forceReadFileAddress (keyhunt.cpp:6300-6358), forceReadFileAddressEth (6374-6450), forceReadFileXPoint (6454-6552):
// the lines long enough to count size the bloom and give the number of lines read from the top of the file, valid
// or not (the reference's i < numberItems with numberItems-- per invalid line, or its i over lines: the same rule).
bool AddrTargets::load_text(const std::string& text, int bloom_multiplier, AddrTargets& T, std::string* err,
                            TargetKind kind) {
  T = AddrTargets();
  T.kind = kind;
  if (kind == kTargetsVanity) {          // no bloom and no table: the intervals of vanity_host.hpp
    T.van.load_text(text);
    T.skipped = T.van.skipped;
    T.counted = T.van.accepted.size();
    return true;
  }
  const std::vector<std::string> lines = fgets_lines(text, kind == kTargetsXpoint ? 1000 : 100);
  const size_t min_len = kind == kTargetsBtc ? 21 : 40;
  for (const std::string& l : lines)
    if (trimmed(l).size() >= min_len) ++T.counted;
  // initBloomFilter (keyhunt.cpp:6559-6576)
  const uint64_t entries = T.counted <= 10000 ? 10000 : (uint64_t)(bloom_multiplier > 0 ? bloom_multiplier : 1) * T.counted;
  if (T.bloom.init2(entries, 0.000001L) != 0) {
    if (err) *err = "bloom_init failed";
    return false;
  }
  for (size_t li = 0; li < T.counted && li < lines.size(); ++li) {
    const std::string aux = trimmed(lines[li]);
    H160 h;
    if (line_h160(kind, aux, h)) {
      T.bloom.add20(h.data());
      T.table.push_back(h);
    } else {
      T.skipped.push_back(aux);
    }
  }
  std::sort(T.table.begin(), T.table.end(),
            [](const H160& a, const H160& b) { return memcmp(a.data(), b.data(), 20) < 0; });
  return true;
}

bool AddrTargets::load_file(const char* path, int bloom_multiplier, AddrTargets& T, std::string* err, TargetKind kind) {
  FILE* f = fopen(path, "r");
  if (!f) {
    if (err) *err = std::string("Error opening the file ") + path;
    return false;
  }
  std::string text;
  char buf[65536];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, n);
  fclose(f);
  return load_text(text, bloom_multiplier, T, err, kind);
}

bool AddrTargets::searchbinary(const uint8_t data[20]) const {
  int64_t half, min = 0, max = (int64_t)table.size(), current = 0;
  bool r = false;
  half = max;
  while (!r && half >= 1) {
    half = (max - min) / 2;
    const int rcmp = memcmp(data, table[(size_t)(current + half)].data(), 20);
    if (rcmp == 0) {
      r = true;
    } else {
      if (rcmp < 0) max = max - half;
      else min = min + half;
      current = min;
    }
  }
  return r;
}

// ----------------------------------------------------------------------------- generator
void AddrGen::build(const U256& s, uint32_t groups_per_chunk, uint32_t g_per_lane, int threads) {
  stride = s;
  gpl = g_per_lane;
  gn.assign(513, Pt());
  const Pt G = mul_g(stride);
  gn[0] = G;
  gn[1] = double_direct(G);
  for (int i = 2; i < 512; ++i) gn[i] = add_direct(gn[i - 1], G);
  gn[512] = double_direct(gn[511]);
  const uint32_t n_off = (groups_per_chunk + gpl - 1) / gpl;
  offs.assign(n_off ? n_off : 1, Pt());
  std::atomic<uint32_t> next{1};
  auto work = [&] {
    for (;;) {
      const uint32_t m = next.fetch_add(1);
      if (m >= n_off) break;
      U256 k = stride * ((uint64_t)m * gpl * 1024u), r;
      U256::divmod(k, secp_order(), nullptr, &r);
      offs[m] = r.is_zero() ? Pt() : mul_g(r);
    }
  };
  std::vector<std::thread> th;
  for (int t = 1; t < threads; ++t) th.emplace_back(work);
  work();
  for (auto& t : th) t.join();
}

std::vector<uint8_t> AddrGen::table_be() const {
  std::vector<uint8_t> out(64 * gn.size());
  for (size_t i = 0; i < gn.size(); ++i) pt_to_be(out.data() + 64 * i, gn[i]);
  return out;
}

std::vector<uint8_t> AddrGen::offs_be() const {
  std::vector<uint8_t> out(64 * offs.size());
  for (size_t i = 0; i < offs.size(); ++i) pt_to_be(out.data() + 64 * i, offs[i]);
  return out;
}

// -------------------------------------------------------------------------------- search
const U256& endo_lambda(int e) {
  static const U256 L[2] = {[] { U256 v; U256::from_hex("5363ad4cc05c30e0a5261c028812645a122e22ea20816678df02967c1b23bd72", v); return v; }(),
                            [] { U256 v; U256::from_hex("ac9c52b33fa3cf1f5ad9e3fd77ed9ba4a880b9fc8ec739c2e0cfc810b51283ce", v); return v; }()};
  return L[e - 1];
}

// The value is recomputed from the key (independently of the GPU's): P = (lambda^e * k)*G has x = beta^e * x(k*G)
// and the same y.  Compressed forms 0/1: the x-only hit belongs to k' or to n - k' (keyhunt.cpp:2811-2822; with -e the
// reference decides by the parity of y, 2800-2860, which gives the same key).  Uncompressed form 2 is k' itself, form
// 3 (-e only) the negated point, n - k' (keyhunt.cpp:2876-2920).  -c eth and -m xpoint never negate (address_host.hpp).
bool confirm_hit(const AddrTargets& T, const U256& key, uint32_t kind, AddrFound* out) {
  const bool eth = kind == KHB_ADDR_KIND_ETH, xpoint = !eth && (kind & KHB_ADDR_KIND_X), btc = !eth && !xpoint;
  const uint32_t form = kind & 3u, e = eth ? 0 : (kind & ~(uint32_t)KHB_ADDR_KIND_X) >> 2;
  const bool fits = eth ? T.kind == kTargetsEth : xpoint ? T.kind == kTargetsXpoint
                                                         : T.kind == kTargetsBtc || T.kind == kTargetsVanity;
  if (!fits || e > 2 || (xpoint && form)) return false;
  U256 k;
  U256::divmod(key, secp_order(), nullptr, &k);
  if (e) k = mulmod(k, endo_lambda((int)e), secp_order());
  if (k.is_zero()) return false;
  const Pt P = mul_g(k);
  uint8_t h[64], hc[20];
  if (eth) eth_address_pub(P, h);
  else if (xpoint) pt_to_be(h, P);
  else if (form < 2) hash160_x((uint8_t)(2 + form), P, h);
  else hash160_pub(form == 2 ? P : negation(P), false, h);
  if (!T.is_target(h)) return false;
  bool negated = btc && form == 3;
  if (btc && form < 2) {
    hash160_pub(P, true, hc);
    negated = memcmp(h, hc, 20) != 0;
  }
  // without -e the reported key is the scanned key itself (key, not key mod n), as the reference's keyfound
  out->key = negated ? secp_order() - k : e ? k : key;
  out->compressed = btc && form < 2;
  memcpy(out->rmd.data(), h, 20);
  return true;
}

namespace {

struct AddrShared {
  const AddrTargets& T;
  const AddrGen& G;
  const AddrConfig& cfg;
  const AddrCallbacks& cb;
  const SearchMode sm;                 // cfg.search decoded, with the targets' vanity flag
  U256 cursor;
  uint64_t claimed = 0;
  std::mutex mu;
  AddrStats& stats;
  std::string err;
  int rc = 0;
};

struct ABatch : BatchRange {
  std::vector<U256> bases;
  std::vector<uint8_t> centres;
  size_t jobs() const { return bases.size(); }
  void slice(size_t j0, size_t j1, ABatch& o) const {
    o.bases.assign(bases.begin() + j0, bases.begin() + j1);
    o.centres.assign(centres.begin() + 64 * j0, centres.begin() + 64 * j1);
  }
};

// One device's side of the launch pipeline (pipeline.hpp run_pipeline): chunk claiming, the khb_addr_submit /
// khb_addr_collect calls and their buffer, the confirmation of the hits and the statistics.  A batch whose bloom
// hits overflowed the ring is rescanned in two parts (by chunks, or one chunk by a gpl-aligned group range), queued
// ahead of new chunks: every hit reaches confirm_hit, as every hit reaches searchbinary in the reference
// (keyhunt.cpp:2716-2937).
struct AddrOps {
  AddrShared& S;
  khb_ctx* ctx;
  const int device;
  const uint32_t groups;               // of a whole chunk
  uint64_t per_batch = 1;              // chunks claimed per launch
  std::vector<khb_addr_hit> hits{};
  uint32_t acap = 0;                   // hits a launch keeps: the ring's capacity, at most hits.size()
  khb_stats st{};                      // the launch collected last
  // after a stop (the caller's stop) the prepared batch is dropped instead of queued, so the exit waits for at most
  // the one launch still in flight
  static constexpr bool drop_on_stop = true;

  int fail(int code, const char* what) {
    std::lock_guard<std::mutex> lk(S.mu);
    if (!S.rc) {
      S.rc = code;
      S.err = std::string(what) + ": " + khb_strerror(code);
    }
    return code;
  }
  bool stopped() { return S.cb.stop && S.cb.stop(); }
  bool fresh(ABatch& b) {
    b.bases.clear();
    {
      std::lock_guard<std::mutex> lk(S.mu);
      if (S.rc) return false;
      while (b.bases.size() < per_batch) {
        if (S.cfg.max_chunks && S.claimed >= S.cfg.max_chunks) break;
        if (S.cfg.random) {
          b.bases.push_back(random_in(S.cfg.start, S.cfg.end));
        } else {
          if (!(S.cursor < S.cfg.end)) break;
          b.bases.push_back(S.cursor);
          S.cursor = S.cursor + U256(S.cfg.n_seq);
        }
        ++S.claimed;
      }
    }
    if (b.bases.empty()) return false;
    if (S.cb.on_chunk)
      for (const U256& c : b.bases) S.cb.on_chunk(c, device);
    const U256 half = S.G.stride * 512u;
    b.centres.resize(64 * b.bases.size());
    for (size_t k = 0; k < b.bases.size(); ++k) {
      U256 c = b.bases[k] + half, r;   // startP = ComputePublicKey(key_mpz + 512*stride)
      U256::divmod(c, secp_order(), nullptr, &r);
      pt_to_be(b.centres.data() + 64 * k, mul_g(r));
    }
    return true;
  }
  int submit(const ABatch& b) {
    const int rc = khb_addr_submit(ctx, b.centres.data(), (uint32_t)b.bases.size(), b.group_begin,
                                   b.group_count ? b.group_count : groups, encode_search(S.sm));
    return rc ? fail(rc, "khb_addr_submit") : 0;
  }
  int collect() {
    st = khb_stats{};
    const int rc = khb_addr_collect(ctx, hits.data(), (uint32_t)hits.size(), &st);
    return rc ? fail(rc, "khb_addr_collect") : 0;
  }
  int done(const ABatch& b, ABatch& lo, ABatch& hi) {
    if (st.n_cand > acap) {              // the ring kept only acap hits: rescan the batch in parts
      if (!split_batch(b, groups, S.G.gpl, lo, hi))
        return fail(-100, "bloom hit ring overflow on a single work item (target bloom too full)");
      std::lock_guard<std::mutex> lk(S.mu);
      S.stats.launches++;
      S.stats.rescans++;
      S.stats.kernel_seconds += st.kernel_ms * 1e-3;
      if (!b.part) S.stats.chunks += b.bases.size();
      return kRescan;
    }
    const uint32_t nh = st.n_cand;
    std::sort(hits.begin(), hits.begin() + nh, [](const khb_addr_hit& x, const khb_addr_hit& y) {
      if (x.job != y.job) return x.job < y.job;
      if (x.group != y.group) return x.group < y.group;
      if (x.t != y.t) return x.t < y.t;
      return x.kind < y.kind;
    });
    std::vector<AddrFound> found;
    for (uint32_t h = 0; h < nh; ++h) {
      const khb_addr_hit& ht = hits[h];
      const U256 key = b.bases[ht.job] + S.G.stride * ((uint64_t)ht.group * 1024u + ht.t);
      AddrFound f;
      if (confirm_hit(S.T, key, ht.kind, &f)) found.push_back(f);
    }
    std::lock_guard<std::mutex> lk(S.mu);
    S.stats.launches++;
    if (!b.part) S.stats.chunks += b.bases.size();
    S.stats.keys += st.giant_steps;
    S.stats.hits += st.n_cand;
    S.stats.degenerate += st.n_degenerate;
    S.stats.kernel_seconds += st.kernel_ms * 1e-3;
    if (st.shader_mhz > 0) {
      S.stats.shader_mhz_sum += st.shader_mhz;
      S.stats.shader_mhz_n++;
    }
    S.stats.found += found.size();
    if (S.cb.on_found)
      for (const AddrFound& f : found) S.cb.on_found(f);
    return 0;
  }
};

void device_loop(AddrShared& S, int device) {
  AddrOps ops{S, nullptr, device, (uint32_t)(S.cfg.n_seq / 1024)};
  khb_ctx*& ctx = ops.ctx;
  int rc = khb_open(device, S.cfg.lanes, &ctx);
  if (rc) { ops.fail(rc, "khb_open"); return; }
  const std::vector<uint8_t> gtab = S.G.table_be(), offs = S.G.offs_be();
  const bool vanity = S.sm.vanity;
  const BloomGeom bg = vanity ? BloomGeom{} : S.T.bloom.geom();
  const std::vector<uint8_t> iv = S.T.van.merged_bytes();   // lo || hi per interval
  std::vector<uint8_t> van_lo(iv.size() / 2), van_hi(iv.size() / 2);
  for (size_t i = 0; i < iv.size() / 40; ++i) {
    memcpy(van_lo.data() + 20 * i, iv.data() + 40 * i, 20);
    memcpy(van_hi.data() + 20 * i, iv.data() + 40 * i + 20, 20);
  }
  int depth = 2;
  if ((S.cfg.hit_cap && (rc = khb_set_candidate_capacity(ctx, S.cfg.hit_cap))) ||
      (rc = khb_load_giant_table(ctx, gtab.data())) ||
      (rc = khb_load_lane_offsets(ctx, offs.data(), (uint32_t)S.G.offs.size(), S.G.gpl)) ||
      (rc = vanity ? khb_load_vanity(ctx, van_lo.data(), van_hi.data(), (uint32_t)(iv.size() / 40))
                   : khb_load_addr_bloom(ctx, S.T.bloom.bf.data(), bg.bytes_per_sub, bg.bits, bg.hashes))) {
    ops.fail(rc, "table upload");
  } else if ((rc = reserve_depth(depth, KHB_ENOMEM, [&](int n) { return khb_reserve_slots(ctx, n); },
                                 [&](const char* m) {   // large targets or many devices' worth of scratch
                                   std::lock_guard<std::mutex> lk(S.mu);
                                   if (S.cb.on_warning) S.cb.on_warning(m);
                                 }))) {
    ops.fail(rc, "khb_reserve_slots");
  } else {
    // about eight work items per lane (the kernel's waves take items dynamically, so a deep launch keeps every SIMD
    // full until its last items), and two launches queued (the context's two submission slots): the next launch
    // fills the CUs the current one's tail leaves idle
    const uint64_t lanes_per_job = (ops.groups + S.G.gpl - 1) / S.G.gpl;
    ops.per_batch = std::min<uint64_t>(4096, std::max<uint64_t>(1, (8ull * khb_lanes(ctx) + lanes_per_job - 1) / lanes_per_job));
    ops.hits.resize(1u << 18);
    ops.acap = std::min<uint32_t>(khb_addr_hit_capacity(ctx), (uint32_t)ops.hits.size());
    if (vanity) {
      // every hash inside the table is a hit, so a launch is sized to keep its expected hits (keys x hashes per key x
      // the table's share of all hashes) at or below a quarter of the ring; more than that in one chunk overflows
      // and is rescanned in parts like any other overflow
      // hashes per key: 1 uncompressed, 2 compressed (02 and 03), 3 for both; with -e 6, 6 and 12
      const int hashes[2][3] = {{1, 2, 3}, {6, 6, 12}};
      const double forms = hashes[S.sm.endo ? 1 : 0][S.sm.forms];
      const double per_chunk = (double)S.cfg.n_seq * forms * S.T.van.covered();
      const double fit = per_chunk > 0 ? 0.25 * ops.acap / per_chunk : (double)ops.per_batch;
      ops.per_batch = fit < 1 ? 1 : std::min<uint64_t>(ops.per_batch, (uint64_t)fit);
    }
    run_pipeline<ABatch>(ops, depth);
  }
  khb_close(ctx);
}

}  // namespace

int addr_search(const AddrTargets& T, const AddrGen& G, const AddrConfig& cfg, const AddrCallbacks& cb,
                AddrStats* stats, std::string* err) {
  AddrStats local;
  AddrStats& st = stats ? *stats : local;
  st = AddrStats();
  if (cfg.n_seq < 1024 || cfg.n_seq % 1024 || cfg.n_seq / 1024 > 0xFFFFFFFFull) {
    if (err) *err = "n must be a positive multiple of 1024";
    return -100;
  }
  SearchMode sm;
  const bool ok = decode_search(cfg.search, sm) && !sm.vanity;   // the search sets KHB_SEARCH_VANITY, not the caller
  sm.vanity = T.kind == kTargetsVanity;
  if (sm.vanity && (!ok || sm.family != kFamilyBtc || T.van.merged.empty())) {
    if (err)
      *err = T.van.merged.empty() ? "there are no vanity targets"
                                  : "vanity targets are searched with search 0, 1 or 2 (-l), optionally with -e";
    return KHB_EINVAL;
  }
  const bool eth = sm.family == kFamilyEth, xpoint = sm.family == kFamilyXpoint;
  if (!ok || (sm.vanity ? kTargetsVanity : eth ? kTargetsEth : xpoint ? kTargetsXpoint : kTargetsBtc) != T.kind) {
    if (err)
      *err = T.kind == kTargetsEth ? "targets loaded for -c eth are searched with KHB_SEARCH_ETH alone (no -l bits, no -e)"
             : T.kind == kTargetsXpoint
                 ? "targets loaded for -m xpoint are searched with KHB_SEARCH_XPOINT, optionally with -e (no -l bits)"
             : eth    ? "KHB_SEARCH_ETH needs targets loaded for -c eth (these are BTC hash160 targets)"
             : xpoint ? "KHB_SEARCH_XPOINT needs targets loaded for -m xpoint (these are BTC hash160 targets)"
                      : "search must be 0, 1 or 2 (-l), optionally with -e";
    return KHB_EINVAL;
  }
  if ((cfg.n_seq / 1024 + G.gpl - 1) / G.gpl > G.offs.size()) {
    if (err) *err = "generator lane offsets do not cover a chunk";
    return -100;
  }
  AddrShared S{T, G, cfg, cb, sm, cfg.start, 0, {}, st, {}, 0};
  std::vector<std::thread> th;
  for (int d : cfg.devices) th.emplace_back(device_loop, std::ref(S), d);
  for (auto& t : th) t.join();
  if (S.rc && err) *err = S.err;
  return S.rc;
}

}  // namespace khb
