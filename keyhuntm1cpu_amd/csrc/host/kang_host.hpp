// Pollard's kangaroo (lambda) interval search with distinguished points: the host side of DESIGN.md §2g.
//
// Target P with key in [start, end), W = end - start, Q = P - start*G.  Kangaroo i is tame when i is even (its point
// is d*G) and wild when odd (Q + d*G); all of them jump by the rule of device/kangaroo.hpp.  A tame and a wild
// kangaroo that report the same distinguished x give key' = d_tame - d_wild (mod n), or -(d_tame + d_wild) when the
// points are each other's negatives; key = start + key'.  Every candidate is verified (key*G == P) before it is
// reported.  Two kangaroos of the same kind on the same x have merged: the later one is replaced by a fresh one.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "secp_host.hpp"
#include "u256.hpp"

namespace khb {

// ---- distances mod n (a, b < n) ----
inline U256 kang_add_mod_n(const U256& a, const U256& b) {
  U256 r;
  const uint64_t c = U256::add(r, a, b);
  if (c || r >= secp_order()) r = r - secp_order();
  return r;
}
inline U256 kang_sub_mod_n(const U256& a, const U256& b) {
  U256 r;
  if (U256::sub(r, a, b)) r = r + secp_order();
  return r;
}
inline U256 kang_neg_mod_n(const U256& a) { return a.is_zero() ? a : secp_order() - a; }

// ---- the distinguished-point table: open addressing keyed by x, linear probing, doubled at half full ----
struct KangEntry {
  U256 x, d;
  uint32_t kind = 0;      // 0 tame, 1 wild
  uint32_t used = 0;
};

class KangDpTable {
 public:
  explicit KangDpTable(uint32_t log2_slots = 10) : slots_((size_t)1 << log2_slots) {}
  // The entry already stored for x, or nullptr after storing {x, d, kind}.  Nothing is ever dropped.
  const KangEntry* insert(const U256& x, const U256& d, uint32_t kind) {
    if (2 * (count_ + 1) > slots_.size()) grow();
    KangEntry& e = slots_[find(slots_, x, &probes_)];
    if (e.used) return &e;
    e.x = x;
    e.d = d;
    e.kind = kind;
    e.used = 1;
    ++count_;
    return nullptr;
  }
  const KangEntry* lookup(const U256& x) const {
    const KangEntry& e = slots_[find(slots_, x, nullptr)];
    return e.used ? &e : nullptr;
  }
  size_t size() const { return count_; }
  size_t slots() const { return slots_.size(); }
  uint64_t probes() const { return probes_; }     // slots passed over by insert: collisions met
  uint32_t grown() const { return grown_; }

 private:
  // A distinguished x has zero bits where the DP test looks, so every word is mixed in.
  static uint64_t hash(const U256& x) {
    uint64_t h = x.w[0] ^ (x.w[1] * 0x9E3779B97F4A7C15ull) ^ (x.w[2] * 0xC2B2AE3D27D4EB4Full) ^ (x.w[3] * 0x165667B19E3779F9ull);
    h ^= h >> 32;
    h *= 0xD6E8FEB86659FD93ull;
    h ^= h >> 29;
    return h;
  }
  // The slot that holds x, or the free one where it belongs.
  static size_t find(const std::vector<KangEntry>& s, const U256& x, uint64_t* probes) {
    const size_t mask = s.size() - 1;
    size_t i = (size_t)hash(x) & mask;
    while (s[i].used && s[i].x != x) {
      i = (i + 1) & mask;
      if (probes) ++*probes;
    }
    return i;
  }
  void grow() {
    std::vector<KangEntry> bigger(slots_.size() * 2);
    for (const KangEntry& e : slots_)
      if (e.used) bigger[find(bigger, e.x, nullptr)] = e;
    slots_.swap(bigger);
    ++grown_;
  }
  std::vector<KangEntry> slots_;
  size_t count_ = 0;
  uint64_t probes_ = 0;
  uint32_t grown_ = 0;
};

// ---- the search ----
constexpr int kKangJumps = 32;
constexpr int kKangMinBits = 16, kKangMaxBits = 200;      // accepted widths: 2^16 <= W <= 2^200

struct KangRoo {
  Pt p;
  U256 d;
};

struct KangDp {
  uint32_t i;
  U256 x, d;
};

struct KangResult {
  bool found = false;
  U256 key;
  uint64_t steps = 0;        // jumps made, all devices
  uint64_t dps = 0;          // distinguished points digested
  uint64_t dead = 0;         // merged kangaroos replaced
  uint64_t lost_dps = 0;     // points a full ring dropped
  uint64_t launches = 0;
  double seconds = 0;
};

struct KangSearch {
  Pt pub, Q;
  bool q_infinity = false;   // the key is `start` itself: Q has no affine form
  U256 start, end, width;
  int w_bits = 0;            // bit length of the width
  uint32_t dp_bits = 0;
  uint64_t herd = 0;         // kangaroos per device
  uint64_t seed = 0;
  U256 jump_s[kKangJumps];
  Pt jump_p[kKangJumps];
  uint32_t ring_cap = 0;     // tests: ring entries per launch (0 = sized from the herd)
  std::vector<KangRoo> planted;      // tests: the first kangaroos of the first device's herd
  bool keep_herd = false;            // keep the first device's herd as the search leaves it
  std::vector<KangRoo> final_herd;
};

// herd_cap: the most kangaroos per device the defaults choose (one full residency x slots per lane).  dp_bits < 0 and
// herd == 0 ask for the defaults: the largest herd and dp_bits with herd * 2^dp_bits <= 2^(w_bits / 2 - 2).
bool kang_init(KangSearch& S, const Pt& pub, const U256& start, const U256& end, int dp_bits, uint64_t herd,
               uint64_t seed, uint64_t herd_cap, std::string* err);
// Kangaroo i of herd `stream` (a device's index), generation g (0 at first, then one per replacement): its distance
// from the seeded generator and its point, through the host's own k*G.
KangRoo kang_make(const KangSearch& S, uint32_t stream, uint64_t i, uint32_t gen);
// `steps` jumps of each of the n kangaroos on the portable field of device/fe.hpp, one batch inversion per step; the
// distinguished points in the order they are met (step by step, ascending kangaroo).
void kang_cpu_walk(const KangSearch& S, KangRoo* herd, uint64_t n, uint32_t steps, uint32_t dp_bits,
                   std::vector<KangDp>& dps, uint64_t* second_choice);
// devices empty: the herd walks on the CPU (kang_cpu_walk), which is how the host logic is tested without a GPU.
// max_steps: jumps in all (0 = no limit); reaching it is "not found", not an error.
int kang_search(KangSearch& S, const std::vector<int>& devices, uint64_t max_steps, KangResult& R, std::string* err);

}  // namespace khb
