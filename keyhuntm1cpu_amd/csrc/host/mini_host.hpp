// Host side of keyhunt's -m minikeys (thread_process_minikeys, keyhunt.cpp:2338-2505) on libkhbsgs: the candidate
// strings and their counter, the window table of the device's k*G, launches of a bounded size through the launch
// pipeline (pipeline.hpp) with the rescan of an overflowed launch in halves, and the confirmation of every device hit
// by recomputing minikey -> key -> mul_g -> hash160 and a lookup in the sorted target table.
//
// A minikey is 'S' and 21 characters of a 58-character alphabet (the reference's Ccoinbuffer_default unless the caller
// gives another, as -8 does); the 21 digits count in [0, 58^21).  It is valid iff byte 0 of SHA-256(minikey || '?') is
// zero, its key is SHA-256(minikey) read big-endian, and it matches iff the hash160 of the key's uncompressed public
// key is a target.
//
// Two deliberate deviations from the reference.  It steps its base by 253 N candidates per cycle and runs each cycle
// until N valid keys were seen (keyhunt.cpp:897-917, 2430-2501), so consecutive cycles overlap or leave gaps at
// random; here a span [first, first + count) is examined exactly once per candidate.  And it increments before its
// first test, so the base it prints is never tested; here `first` is tested.
#pragma once
#include <stdint.h>

#include <array>
#include <functional>
#include <string>
#include <vector>

#include "address_host.hpp"
#include "mini_table.hpp"

namespace khb {

constexpr int kMiniLen = 22;                     // characters of a minikey
constexpr int kMiniDigitCount = 21;
extern const char kMiniDefaultAlphabet[59];      // Ccoinbuffer_default

struct MiniAlphabet {
  uint8_t chars[58];
  int8_t digit[256];                             // -1: not in the alphabet
  // 58 distinct bytes, none of them NUL; null = the default.  False otherwise.
  bool set(const uint8_t* a);
};

using MiniDigits = std::array<uint8_t, kMiniDigitCount>;

// The digits of a 22-character minikey; false with *err for another length, a first character other than 'S' or a
// character outside the alphabet.
bool mini_parse(const MiniAlphabet& A, const char* s, size_t len, MiniDigits& out, std::string* err);
// d + off; false when the sum is 58^21 or more.
bool mini_advance(MiniDigits& d, uint64_t off);
void mini_string(const MiniAlphabet& A, const MiniDigits& d, char out[kMiniLen]);
bool mini_is_valid(const char s[kMiniLen]);             // byte 0 of SHA-256(s || '?') is zero
void mini_key_of(const char s[kMiniLen], uint8_t out[32]);   // SHA-256(s)

struct MiniFound {
  char minikey[kMiniLen];
  U256 key;
  H160 rmd;
};

struct MiniStats {
  uint64_t candidates = 0, valid = 0, bad_keys = 0, hits = 0, found = 0;
  uint64_t launches = 0, rescans = 0;
  double filter_seconds = 0, keys_seconds = 0;
};

struct MiniConfig {
  std::vector<int> devices{0};
  uint32_t lanes = 0;                  // 0 = library default
  uint64_t per_launch = 1ull << 30;    // candidates per launch (at most 2^32)
  uint32_t queue_cap = 0;              // tests: survivor-queue capacity (0 = sized from the launch)
  uint32_t hit_cap = 0;                // tests: bloom-hit ring capacity (0 = library default)
};

struct MiniSearch {
  AddrTargets T;                       // kTargetsBtc: the bloom and the sorted table of -m address
  MiniAlphabet A;
  uint32_t window_bits = 16;
  std::vector<uint8_t> table;          // mini_table_be(window_bits)
};

// Examine first, first + 1, ..., first + count - 1.  0, or a KHB_E* / -100 code with *err; first + count > 58^21 is
// KHB_EINVAL and launches nothing.  on_found is called in offset order within a launch, launches in the order they
// are collected (the halves of a rescanned launch may follow a launch queued before the split).
int mini_search(const MiniSearch& M, const MiniDigits& first, uint64_t count, const MiniConfig& cfg,
                const std::function<void(const MiniFound&)>& on_found, MiniStats* stats, std::string* err);


// The reference's loop on the CPU over the same span (a measurement's baseline): `threads` threads, each a contiguous
// part.  Returns the seconds taken; valid and found as the loop counted them.
double mini_cpu_scan(const MiniSearch& M, const MiniDigits& first, uint64_t count, int threads, uint64_t* valid,
                     uint64_t* found);

}  // namespace khb
