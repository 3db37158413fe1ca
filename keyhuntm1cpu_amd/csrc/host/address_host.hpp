// Host side of keyhunt's -m address / -m rmd160 (BTC P2PKH, with or without -e; -c eth), -m xpoint and -m vanity modes on
// libkhbsgs: target loading (forceReadFileAddress, keyhunt.cpp:6300-6358; forceReadFileAddressEth, 6374-6450;
// forceReadFileXPoint, 6454-6552), the generator table
// (init_generator, keyhunt.cpp:4386-4399), chunk claiming (thread_process, keyhunt.cpp:2546-2567),
// and the confirmation of GPU bloom hits (searchbinary + key recovery, keyhunt.cpp:2789-2937).
#pragma once
#include <stdint.h>

#include <array>
#include <functional>
#include <string>
#include <vector>

#include "../device/scan_modes.hpp"
#include "bloom_host.hpp"
#include "secp_host.hpp"
#include "u256.hpp"
#include "vanity_host.hpp"

namespace khb {

using H160 = std::array<uint8_t, 20>;

// The value of a Base58 digit, -1 for any other character.
int b58_digit(unsigned char c);
// b58tobin into 25 bytes with keyhunt's acceptance rule (decoded size == 25, base58.c:39-112).
bool b58decode25(const char* s, uint8_t out[25]);
// rmd160toaddress_dst (keyhunt.cpp:2274-2284): base58check of 0x00 || rmd.
std::string rmd_to_address(const uint8_t rmd[20]);
void sha256(const uint8_t* msg, size_t len, uint8_t out[32]);
// GetHash160(P2PKH, compressed, P) (SECP256K1.cpp:671-705) / GetHash160_fromX (:707-789)
void hash160_pub(const Pt& p, bool compressed, uint8_t out[20]);
void hash160_x(uint8_t prefix, const Pt& p, uint8_t out[20]);
// generate_binaddress_eth (keyhunt.cpp:4783-4789): bytes 12..31 of Keccak-256(x || y)
void eth_address_xy(const uint8_t xy[64], uint8_t out[20]);
void eth_address_pub(const Pt& p, uint8_t out[20]);

// What a target file's lines are (the khh_addr_new* entry points of include/khhost.h choose one)
enum TargetKind {
  kTargetsBtc = 0,      // -m address / -m rmd160: base58 P2PKH addresses or 40-hex hash160 (forceReadFileAddress)
  kTargetsEth = 1,      // -c eth: 40-hex lines, with or without a two-character prefix (forceReadFileAddressEth)
  kTargetsXpoint = 2,   // -m xpoint: public keys or x coordinates (forceReadFileXPoint)
  kTargetsVanity = 3,   // -m vanity: address prefixes, one per line (vanity_host.hpp)
};

struct AddrTargets {
  std::vector<H160> table;             // sorted (memcmp), the reference's addressTable after _sort
  BloomFilter bloom;                   // initBloomFilter(counted lines)
  uint64_t counted = 0;                // lines long enough to count (sizes the bloom)
  std::vector<std::string> skipped;    // "[I] Ommiting invalid line": the trimmed lines
  TargetKind kind = kTargetsBtc;       // what the table holds: hash160s, ETH addresses or the first 20 bytes of x;
                                       // kTargetsVanity: `van` holds the targets, table and bloom stay empty
  VanityTargets van;

  // text: the target file's contents.  Returns false with *err on an unusable bloom.  counted = lines of more than 20
  // characters (BTC) or of 40 or more (ETH, xpoint), and that many lines are read from the top of the file.
  // BTC: a valid base58 line of under 40 characters, or a 40-hex line.
  // ETH: a 40-hex line, or a 42-character line whose last 40 are hex (its first two characters are not looked at).
  // xpoint (keyhunt.cpp:6454-6552): the first token (separators: space, tab, ':') decides: 64 hex = x, 66 hex = a
  // compressed key whose two prefix characters are dropped unchecked, 130 hex = an uncompressed key; anything else
  // goes to `skipped` and not into the table (the reference keeps a zero entry for it).  Table and bloom hold the
  // first 20 bytes of x.  Deviation: for a 130-hex line the reference adds 04 || x[0..18] to the bloom and stores
  // x[1..20] in the table (6524-6528), so such a line can never be found there; here both take x[0..19].
  static bool load_text(const std::string& text, int bloom_multiplier, AddrTargets& out, std::string* err,
                        TargetKind kind = kTargetsBtc);
  static bool load_file(const char* path, int bloom_multiplier, AddrTargets& out, std::string* err,
                        TargetKind kind = kTargetsBtc);
  bool searchbinary(const uint8_t h[20]) const;   // keyhunt.cpp:2311-2335, literal
  // h is wanted: searchbinary, or for -m vanity the address of h begins with a target (VanityTargets::matches)
  bool is_target(const uint8_t h[20]) const { return kind == kTargetsVanity ? van.matches(h) : searchbinary(h); }
};

struct AddrGen {
  U256 stride{1};
  std::vector<Pt> gn;                  // Gn[0..511] = (i+1)*stride*G, gn[512] = _2Gn = 1024*stride*G
  std::vector<Pt> offs;                // offs[m] = m*gpl*_2Gn  (lane starts within a chunk)
  uint32_t gpl = 0;
  void build(const U256& stride, uint32_t groups_per_chunk, uint32_t gpl, int threads);
  std::vector<uint8_t> table_be() const;
  std::vector<uint8_t> offs_be() const;
};

struct AddrConfig {
  int search = 2;                      // khb_addr_submit's `search` (encode_search) without KHB_SEARCH_VANITY, which
                                       // the search adds for kTargetsVanity targets: -l 0, 1 or 2 (keyhunt.cpp:59-61,
                                       // 300), KHB_SEARCH_ETH or _XPOINT for targets of that kind, and
                                       // KHB_SEARCH_ENDOMORPHISM for -e (keyhunt.cpp:579-585)
  U256 start{1}, end{1};               // [start, end): n_range_start / n_range_end
  uint64_t n_seq = 1ull << 32;         // keys per claimed chunk (-n, N_SEQUENTIAL_MAX)
  bool random = false;                 // -R: each chunk starts at a random key in [start, end)
  std::vector<int> devices{0};
  uint32_t lanes = 0;                  // 0 = library default
  uint32_t gpl = 16;                   // groups per GPU lane
  uint64_t max_chunks = 0;             // 0 = until the range is exhausted
  uint32_t hit_cap = 0;                // tests: the launch's bloom-hit capacity (0 = library default)
};

struct AddrFound {
  U256 key;
  bool compressed;
  H160 rmd;                            // the hash160, the ETH address (-c eth) or the matched 20 bytes of x (-m xpoint)
};

struct AddrStats {
  uint64_t launches = 0, chunks = 0, keys = 0, hits = 0, found = 0, degenerate = 0;
  uint64_t rescans = 0;            // launches whose bloom hits overflowed the ring (rescanned in parts)
  double kernel_seconds = 0;
  double shader_mhz_sum = 0;       // sum of the launches' average shader clocks (khb_stats.shader_mhz)
  uint64_t shader_mhz_n = 0;
};

struct AddrCallbacks {
  std::function<void(const AddrFound&)> on_found;             // called in range order per batch
  std::function<void(const U256& base, int device)> on_chunk;  // "Base key: ..." progress
  std::function<bool()> stop;                                  // polled between batches
  std::function<void(const std::string&)> on_warning;          // e.g. the depth-1 fallback
};

// Confirm one GPU bloom hit (khb_addr_hit.kind = form | e << 2) of the point whose key is `key`: searchbinary of the
// hash the kind names, then the reference's key recovery (keyhunt.cpp:2789-2937): lambda^e * key, negated when the
// hit is the other point of the pair.  False when the hash is not a target (a bloom false positive).  With -m vanity
// targets the same kinds and recovery, and the hash is a target iff its address begins with one of them.
// kind KHB_ADDR_KIND_ETH (-c eth, keyhunt.cpp:2989-3002): the ETH address of key*G, the key returned unchanged.
// kind KHB_ADDR_KIND_X | e << 2 (-m xpoint, keyhunt.cpp:3005-3062): the first 20 bytes of beta^e * x(key*G); the key
// returned is lambda^e * key mod n (the walked key itself for e = 0), never negated; compressed = false.
bool confirm_hit(const AddrTargets& T, const U256& key, uint32_t kind, AddrFound* out);
// lambda and lambda^2 mod n (keyhunt.cpp:582-583)
const U256& endo_lambda(int e);

// Sequential (or -R random) search over the range; returns 0 or a KHB_E* / -100 code with *err.
int addr_search(const AddrTargets& T, const AddrGen& G, const AddrConfig& cfg, const AddrCallbacks& cb,
                AddrStats* stats, std::string* err);

}  // namespace khb
