#include "vanity_host.hpp"

#include <math.h>
#include <string.h>

#include <algorithm>

#include "address_host.hpp"
#include "u256.hpp"

namespace khb {

namespace {

struct Range {
  U256 lo, hi;
};

H160 low160(const U256& v) {
  uint8_t b[32];
  v.to_be(b);
  H160 h;
  memcpy(h.data(), b + 12, 20);
  return h;
}

U256 of160(const H160& h) {
  uint8_t b[32] = {0};
  memcpy(b + 12, h.data(), 20);
  return U256::from_be(b);
}

U256 pow2(int n) { return U256(1).shl(n); }

// The ranges of hash160 values for s (see vanity_host.hpp); empty when s is not accepted.
std::vector<Range> ranges_of(const std::string& s) {
  std::vector<Range> out;
  if (s.empty() || s.size() > 29 || s[0] != '1') return out;
  for (const char c : s)
    if (b58_digit((unsigned char)c) < 0) return out;
  size_t z = 0;
  while (z < s.size() && s[z] == '1') ++z;
  const size_t nr = s.size() - z;                // digits behind the '1's; the first of them is not '1'
  if (z > 25 || (nr && z > 24)) return out;      // no 25-byte value prints with that many '1's
  const U256 top = pow2(8 * (25 - (int)z)) - U256(1);
  if (nr == 0) {
    out.push_back(Range{U256(0), top.shr(32)});
    return out;
  }
  const U256 bottom = pow2(8 * (24 - (int)z));
  U256 rv(0);
  for (size_t i = z; i < s.size(); ++i) rv = rv * 58u + U256((uint64_t)b58_digit((unsigned char)s[i]));
  // n digits in all: s padded with n - nr characters.  58^35 > 2^200, so 35 digits cover every 25-byte value and
  // every product below stays under 2^256.
  U256 span(1);                                  // 58^(n - nr)
  for (size_t n = nr; n <= 35; ++n, span = span * 58u) {
    U256 lo = rv * span, hi = lo + (span - U256(1));
    if (lo > top) break;
    if (lo < bottom) lo = bottom;
    if (hi > top) hi = top;
    if (lo <= hi) out.push_back(Range{lo.shr(32), hi.shr(32)});
  }
  return out;
}

}  // namespace

bool VanityTargets::intervals_of(const std::string& s, std::vector<VanityInterval>& out) {
  out.clear();
  for (const Range& r : ranges_of(s)) out.push_back(VanityInterval{low160(r.lo), low160(r.hi)});
  return !out.empty();
}

bool VanityTargets::add(const std::string& s, bool merge) {
  std::vector<VanityInterval> iv;
  if (!intervals_of(s, iv)) return false;
  if (!seen.insert(s).second) return true;
  accepted.push_back(s);
  per_target.push_back(iv);
  if (merge) merge_all();
  return true;
}

void VanityTargets::merge_all() {
  merged.clear();
  if (per_target.empty()) return;
  std::vector<Range> all;
  for (const auto& t : per_target)
    for (const VanityInterval& v : t) all.push_back(Range{of160(v.lo), of160(v.hi)});
  std::sort(all.begin(), all.end(), [](const Range& a, const Range& b) { return a.lo < b.lo; });
  Range cur = all[0];
  for (size_t i = 1; i < all.size(); ++i) {
    if (all[i].lo <= cur.hi + U256(1)) {         // overlapping or touching (160-bit values: no wrap in 256 bits)
      if (all[i].hi > cur.hi) cur.hi = all[i].hi;
    } else {
      merged.push_back(VanityInterval{low160(cur.lo), low160(cur.hi)});
      cur = all[i];
    }
  }
  merged.push_back(VanityInterval{low160(cur.lo), low160(cur.hi)});
}

void VanityTargets::load_text(const std::string& text) {
  const char* seps = " \t\n\r";
  size_t p = 0;
  while (p < text.size()) {
    size_t e = text.find('\n', p);
    if (e == std::string::npos) e = text.size();
    const std::string line(text.substr(p, e - p).c_str());
    p = e + 1;
    const size_t b = line.find_first_not_of(seps);
    if (b == std::string::npos) continue;
    const std::string s = line.substr(b, line.find_last_not_of(seps) - b + 1);
    if (s.size() > 35 || !add(s, false)) skipped.push_back(s);   // the reference reads lines of 1 to 35 characters
  }
  merge_all();
}

bool VanityTargets::in_table(const uint8_t h[20]) const {
  // the last interval with lo <= h
  auto it = std::upper_bound(merged.begin(), merged.end(), h, [](const uint8_t* v, const VanityInterval& i) {
    return memcmp(v, i.lo.data(), 20) < 0;
  });
  return it != merged.begin() && memcmp(h, (it - 1)->hi.data(), 20) <= 0;
}

bool VanityTargets::matches(const uint8_t h[20]) const {
  const std::string a = rmd_to_address(h);
  for (const std::string& t : accepted)
    if (a.compare(0, t.size(), t) == 0) return true;
  return false;
}

double VanityTargets::covered() const {
  double sum = 0;
  for (const VanityInterval& v : merged) {
    const U256 d = of160(v.hi) - of160(v.lo) + U256(1);
    sum += ldexp((double)d.w[0], -160) + ldexp((double)d.w[1], -96) + ldexp((double)d.w[2], -32);
  }
  return sum;
}

std::vector<uint8_t> VanityTargets::merged_bytes() const {
  std::vector<uint8_t> out(40 * merged.size());
  for (size_t i = 0; i < merged.size(); ++i) {
    memcpy(out.data() + 40 * i, merged[i].lo.data(), 20);
    memcpy(out.data() + 40 * i + 20, merged[i].hi.data(), 20);
  }
  return out;
}

}  // namespace khb
