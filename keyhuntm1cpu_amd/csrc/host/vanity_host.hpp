// Host side of keyhunt's -m vanity on libkhbsgs: address prefixes as ranges of hash160 values (the table
// khb_load_vanity takes) and the exact confirmation of a hit by the printed address.
//
// Match rule: a hash160 h matches the target string s iff the Base58Check P2PKH address of 0x00 || h begins with s.
//
// Intervals.  A 25-byte value (version, hash, checksum) with exactly z leading zero bytes prints as z '1' characters
// followed by the base-58 digits of its value, the first of them not '1'.  So for a target of z >= 1 '1' characters
// followed by the digits r, and for every address length L, the matching values are those from s padded to length L
// with '1' to s padded to length L with 'z' that have exactly z leading zero bytes: [2^(8(24-z)), 2^(8(25-z)) - 1].
// Both ends are shifted right by 32 bits to drop the checksum, and a non-empty interval is kept.  A target of '1'
// characters alone (r empty) is also the prefix of every address with more leading '1's, so its range is every value
// with at least z leading zero bytes, [0, 2^(8(25-z)) - 1].  The hashes inside the shifted intervals are a superset of
// the matches that can be wrong only at an interval's two ends, where the checksum decides; matches() is exact.
//
// Two deliberate deviations from the reference's addvanity (keyhunt.cpp:5837-5958).  It pads s with '1' and with 'z'
// to every length that decodes to 25 bytes and pairs the j-th lower bound with the j-th upper bound, but the two lists
// can differ in length or start at different lengths, which yields empty or missing ranges: for "1Q" the
// 34-character addresses 1Q1... to 1QLbz7... are never matched, because 1Qzz... overflows 25 bytes at that length.
// The intervals here are exact per length.  And it accepts targets such as "3abc", then matches P2PKH hashes whose
// printed address does not carry the prefix; here a target must begin with '1'.
#pragma once
#include <stdint.h>

#include <array>
#include <set>
#include <string>
#include <vector>

namespace khb {

using H160 = std::array<uint8_t, 20>;

struct VanityInterval {
  H160 lo, hi;                         // closed, big-endian
};

struct VanityTargets {
  std::vector<std::string> accepted;                      // distinct, in the order given
  std::vector<std::vector<VanityInterval>> per_target;    // accepted[i]'s intervals, ascending
  std::vector<VanityInterval> merged;                     // all of them sorted, disjoint, touching ones joined
  std::vector<std::string> skipped;                       // load_text: the lines not accepted
  std::set<std::string> seen;                             // the accepted targets, for the repeated-target test

  // The intervals of one target; false (and none) when it is not accepted: not valid Base58, not 1 to 29 characters
  // (the reference's targetsize >= 30 limit), not beginning with '1', or without a non-empty interval.
  static bool intervals_of(const std::string& s, std::vector<VanityInterval>& out);
  // Accept one target (a repeated one is accepted once) and rebuild `merged`; false: it is not accepted.
  bool add(const std::string& s) { return add(s, true); }
  // One target per line, trimmed; blank lines are passed over, a line that is not accepted goes to `skipped`.
  void load_text(const std::string& text);
  // h lies in a merged interval: what the device reports, a superset of matches().
  bool in_table(const uint8_t h[20]) const;
  // The address of 0x00 || h begins with an accepted target.
  bool matches(const uint8_t h[20]) const;
  // The merged table's share of all 2^160 hashes: sum(hi - lo + 1) / 2^160.
  double covered() const;
  // lo || hi of every merged interval, 40 bytes each
  std::vector<uint8_t> merged_bytes() const;

 private:
  bool add(const std::string& s, bool merge);   // load_text merges once, after its last line
  void merge_all();                             // `merged` from per_target
};

}  // namespace khb
