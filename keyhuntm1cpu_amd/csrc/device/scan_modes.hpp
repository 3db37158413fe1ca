// The modes of k_giant_scan, each described once (kModeTraits), the predicates the device code reads them through,
// and the decoder of the public `search` value of khb_addr_submit (include/khbsgs.h) that both libraries use.  No HIP
// in here: a host compiler takes this header alone (tests/native/test_search_mode.cpp).
#pragma once
#include <stdint.h>
#include "../../../include/khbsgs.h"

namespace khbk {

// Kernel modes (template argument of k_giant_scan, scan_batch / scan_group and the walks).  The numbers do not move:
// the profiles and tools/ name the kernels by them, k_giant_scan<N>.
enum : int {
  kScan = 0,       // -m bsgs: level-1 bloom probe of every x
  kDump = 1,       // -m bsgs parity: write every x
  kAddrU = 2,      // -m address, -l uncompress   (2 + keyhunt SEARCH_UNCOMPRESS, keyhunt.cpp:59-61)
  kAddrC = 3,      // -m address, -l compress
  kAddrB = 4,      // -m address, -l both (the reference default, keyhunt.cpp:300)
  kAddrDump = 5,   // -m address parity: write every x||y
  kBaby = 6,       // baby-step table build: bloom_add of every x into L1/L2/L3 + bPtable records
  kScanG = 7,      // -m bsgs with a level-0 gate (walk_gated, entered as walk_group_g_half / walk_group_g)
  kScanG1 = 8,     // kScanG with the gate's stage-1 fold in front (khb_set_gate_stage1)
  kScanG2 = 9,     // kScanG1 with the stage-0 filter in front of the fold (khb_set_gate_stage0; k >= 4)
  kAddrUE = 10,    // kAddrU / kAddrC / kAddrB with -e (KHB_SEARCH_ENDOMORPHISM: beta*x, beta^2*x, negated y;
  kAddrCE = 11,    //   keyhunt.cpp:2646-2763)
  kAddrBE = 12,
  kAddrEth = 13,   // -m address -c eth: Keccak-256 of x || y (keyhunt.cpp:2776-2780; device/keccak.hpp)
  kAddrX = 14,     // -m xpoint: the first 20 bytes of x probed as they are (keyhunt.cpp:3005-3062; device/xpoint.hpp)
  kAddrXE = 15,    // kAddrX with -e: x, beta*x and beta^2*x (keyhunt.cpp:3013-3043)
  kVanU = 16,      // -m vanity: kAddrU / kAddrC / kAddrB with the interval match of device/vanity.hpp in the place of
  kVanC = 17,      //   the target bloom (KHB_SEARCH_VANITY)
  kVanB = 18,
  kVanUE = 19,     // -m vanity -e: kAddrUE / kAddrCE / kAddrBE likewise
  kVanCE = 20,
  kVanBE = 21,
  kModeCount = 22,
};

// What a mode does with a walked point
enum Work : uint8_t {
  kProbe,       // -m bsgs: level-1 bloom probe of x
  kGated,       // the same behind the level-0 gate, `stages` filter stages in front of the full gate
  kDumpX,       // write x
  kDumpXY,      // write x || y
  kBabyBuild,   // add x to the baby-step tables
  kHash160,     // BTC: hash160 of the forms `unc` / `comp`, with `endo` also of beta*x, beta^2*x and the negated points
  kEth,         // ETH address of x || y
  kXpoint,      // the first 20 bytes of x, with `endo` also of beta*x and beta^2*x
};
// Which occupancy target a mode is compiled for (scan_args.hpp: the KHB_*_WAVES_PER_SIMD macro of each)
enum Occupancy : uint8_t { kOccScan, kOccAddr, kOccAddrE, kOccEth, kOccX, kOccVanity, kOccCount };

struct ModeTraits {
  Work work;
  uint8_t stages;       // kGated: 0 (kScanG), 1 (the fold, kScanG1), 2 (filter + fold, kScanG2)
  bool unc, comp;       // kHash160: the forms hashed (-l)
  bool endo, vanity;    // -e; the match: the vanity intervals in the place of the target bloom
  Occupancy occ;
};

constexpr ModeTraits kModeTraits[kModeCount] = {
    /* kScan    */ {kProbe, 0, false, false, false, false, kOccScan},
    /* kDump    */ {kDumpX, 0, false, false, false, false, kOccScan},
    /* kAddrU   */ {kHash160, 0, true, false, false, false, kOccAddr},
    /* kAddrC   */ {kHash160, 0, false, true, false, false, kOccAddr},
    /* kAddrB   */ {kHash160, 0, true, true, false, false, kOccAddr},
    /* kAddrDump*/ {kDumpXY, 0, false, false, false, false, kOccAddr},
    /* kBaby    */ {kBabyBuild, 0, false, false, false, false, kOccScan},
    /* kScanG   */ {kGated, 0, false, false, false, false, kOccScan},
    /* kScanG1  */ {kGated, 1, false, false, false, false, kOccScan},
    /* kScanG2  */ {kGated, 2, false, false, false, false, kOccScan},
    /* kAddrUE  */ {kHash160, 0, true, false, true, false, kOccAddrE},
    /* kAddrCE  */ {kHash160, 0, false, true, true, false, kOccAddrE},
    /* kAddrBE  */ {kHash160, 0, true, true, true, false, kOccAddrE},
    /* kAddrEth */ {kEth, 0, false, false, false, false, kOccEth},
    /* kAddrX   */ {kXpoint, 0, false, false, false, false, kOccX},
    /* kAddrXE  */ {kXpoint, 0, false, false, true, false, kOccX},
    /* kVanU    */ {kHash160, 0, true, false, false, true, kOccVanity},
    /* kVanC    */ {kHash160, 0, false, true, false, true, kOccVanity},
    /* kVanB    */ {kHash160, 0, true, true, false, true, kOccVanity},
    /* kVanUE   */ {kHash160, 0, true, false, true, true, kOccVanity},
    /* kVanCE   */ {kHash160, 0, false, true, true, true, kOccVanity},
    /* kVanBE   */ {kHash160, 0, true, true, true, true, kOccVanity},
};
constexpr const ModeTraits& traits(int m) { return kModeTraits[m]; }

constexpr bool is_gated(int m) { return traits(m).work == kGated; }
constexpr int gate_stages(int m) { return traits(m).stages; }   // filter stages in front of the full gate
constexpr bool is_scan(int m) { return traits(m).work == kProbe || traits(m).work == kGated; }
constexpr bool is_vanity(int m) { return traits(m).vanity; }
constexpr bool is_endo(int m) { return traits(m).work == kHash160 && traits(m).endo; }   // BTC -e (kAddrXE: is_xpoint)
constexpr bool is_xpoint(int m) { return traits(m).work == kXpoint; }
constexpr bool is_search(int m) { return traits(m).work == kHash160 || traits(m).work == kEth || is_xpoint(m); }
constexpr bool is_addr(int m) { return is_search(m) || traits(m).work == kDumpXY; }
constexpr bool addr_compressed(int m) { return traits(m).comp; }
constexpr bool addr_uncompressed(int m) { return traits(m).unc; }
constexpr bool needs_y(int m) { return traits(m).unc || traits(m).work == kDumpXY || traits(m).work == kEth; }
constexpr bool is_baby(int m) { return traits(m).work == kBabyBuild; }
constexpr bool is_dump(int m) { return traits(m).work == kDumpX || traits(m).work == kDumpXY || is_baby(m); }
constexpr bool is_batched(int m) { return is_scan(m) || traits(m).work == kDumpX; }   // x only, kBatch groups per item
constexpr bool is_xy(int m) { return is_addr(m) || is_baby(m); }                      // x and y, group by group

// ------------------------------------------------------------------------------- the `search` value of khbsgs.h
enum Family : uint8_t { kFamilyBtc, kFamilyEth, kFamilyXpoint };

struct SearchMode {
  Family family = kFamilyBtc;
  int forms = 0;          // the -l value: 0 uncompress, 1 compress, 2 both (kFamilyBtc; 0 otherwise)
  bool endo = false;      // KHB_SEARCH_ENDOMORPHISM
  bool vanity = false;    // KHB_SEARCH_VANITY
};

constexpr int encode_search(const SearchMode& sm) {
  return sm.forms | (sm.endo ? KHB_SEARCH_ENDOMORPHISM : 0) | (sm.vanity ? KHB_SEARCH_VANITY : 0) |
         (sm.family == kFamilyEth ? KHB_SEARCH_ETH : sm.family == kFamilyXpoint ? KHB_SEARCH_XPOINT : 0);
}

// The fields of `search`; false where khbsgs.h says KHB_EINVAL.  -l 0/1/2, -e and vanity go with BTC, -e alone with
// xpoint, nothing with ETH.  A refused value of known bits still leaves its fields in sm (the host's error texts name
// the family asked for); any other leaves sm empty.
constexpr bool decode_search(int search, SearchMode& sm) {
  sm = SearchMode{};
  constexpr int known = 3 | KHB_SEARCH_ENDOMORPHISM | KHB_SEARCH_ETH | KHB_SEARCH_XPOINT | KHB_SEARCH_VANITY;
  const bool eth = search & KHB_SEARCH_ETH, xpoint = search & KHB_SEARCH_XPOINT;
  if (search < 0 || (search & ~known) || (search & 3) == 3 || (eth && xpoint)) return false;
  sm = {eth ? kFamilyEth : xpoint ? kFamilyXpoint : kFamilyBtc, search & 3, (search & KHB_SEARCH_ENDOMORPHISM) != 0,
        (search & KHB_SEARCH_VANITY) != 0};
  return sm.family == kFamilyBtc || (sm.forms == 0 && !sm.vanity && !(eth && sm.endo));
}

// What the traits of a search instance (is_search: a mode khb_addr_submit's `search` selects) say in terms of `search`
constexpr SearchMode search_of_mode(int m) {
  const ModeTraits& t = traits(m);
  return {t.work == kEth ? kFamilyEth : t.work == kXpoint ? kFamilyXpoint : kFamilyBtc,
          t.work != kHash160 ? 0 : t.unc && t.comp ? 2 : t.comp ? 1 : 0, t.endo, t.vanity};
}

// The kernel mode of a decoded search: the instance whose traits say the same; -1 if there is none
constexpr int scan_mode_of(const SearchMode& sm) {
  for (int m = 0; m < kModeCount; ++m)
    if (is_search(m) && encode_search(search_of_mode(m)) == encode_search(sm)) return m;
  return -1;
}

// how many search instances are reached from their own traits, by a value decode_search accepts: all 15
constexpr int search_instances_inverted() {
  int n = 0;
  SearchMode sm;
  for (int m = 0; m < kModeCount; ++m)
    n += is_search(m) && decode_search(encode_search(search_of_mode(m)), sm) && scan_mode_of(sm) == m;
  return n;
}
static_assert(search_instances_inverted() == 15, "scan_mode_of inverts the traits of the 15 search instances");

}  // namespace khbk
