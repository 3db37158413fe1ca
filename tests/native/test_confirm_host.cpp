// Host-compiled check of device/confirm.hpp (the GPU's bsgs_secondcheck / bsgs_thirdcheck, khb_check)
// against the oracle's restatement (oracle/ora_bsgs.c secondcheck, keyhunt.cpp:4271-4368).  Test
// infrastructure: the oracle is the checker.
//   1. real tables of a small geometry: planted keys around each candidate's window (found / not found,
//      both signs of the third check's +-(j+1)), the AddDirect(P, -P) special case of the third check,
//      and random candidates;
//   2. the same candidates with every level-2 and level-3 bloom bit set in both implementations, so each
//      candidate runs 32 third checks, 1024 level-3 probes and bPtable searches;
//   3. the directed classes of tests/check_cases.py, built here from the same formulas: Z (dx == 0 inside a
//      batch: Q == -+AMP2[i2], Q' == +AMP3[i], the other 31 x of the batch pinned through the blooms), K (start = 0
//      with a = 0, target == base*G), C (sums that carry through several limbs, a base that wraps past 2^256), D
//      (runs of three equal 6-byte keys in the bPtable: the reference's probe sequence decides which key is
//      found), blooms that hold exactly the 32 + 32 x 32 x of four candidates, the U8 helpers against the
//      oracle's 256-bit integers on operands that carry and borrow through every limb, and search_bp against
//      the oracle's bsgs_searchbinary on tables of 1 to 300 entries with runs of equal keys.
#include "../../keyhuntm1cpu_amd/csrc/device/confirm.hpp"
extern "C" {
#include "../../oracle/ora.h"
}
#include <cstdio>
#include <cstring>
#include <vector>
using namespace khb;

static uint64_t sm = 0x636f6e6669726dull;
static uint64_t splitmix() {
  uint64_t z = (sm += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

static Fe fe_of(const ora_u256& a) {
  Fe f;
  for (int k = 0; k < 4; ++k) {
    f.v[2 * k] = (uint32_t)a.w[k];
    f.v[2 * k + 1] = (uint32_t)(a.w[k] >> 32);
  }
  return f;
}
static U8 u8_of(const ora_u256& a) {
  Fe f = fe_of(a);
  U8 r;
  memcpy(r.v, f.v, sizeof r.v);
  return r;
}
static ora_u256 ora_of(const U8& a) {
  ora_u256 r;
  for (int k = 0; k < 4; ++k) r.w[k] = a.v[2 * k] | ((uint64_t)a.v[2 * k + 1] << 32);
  return r;
}
static CPt cpt_of(const ora_point& p) { return CPt{fe_of(p.x), fe_of(p.y)}; }
static CPt cpt_be(const uint8_t* b) {
  CPt p;
  fe_from_be(p.x, b);
  fe_from_be(p.y, b + 32);
  return p;
}
static ora_u256 u64v(uint64_t v) {
  ora_u256 r;
  ora_u256_set64(&r, v);
  return r;
}
static ora_u256 add(ora_u256 a, const ora_u256& b) {
  ora_u256 r;
  ora_u256_add(&r, &a, &b);
  return r;
}
static ora_u256 mul(ora_u256 a, uint64_t m) {
  ora_u256 r;
  ora_u256_mul64(&r, &a, m);
  return r;
}

struct Case {
  ora_u256 base;
  uint32_t a;
  ora_point target;
  const char* kind;
};

int main() {
  ora_secp_init();
  char err[256];
  ora_bsgs* B = ora_bsgs_new("0x1000000000", 1, 8, err, sizeof err);   // N = 2^36: m = 2^18, m2 = 2^13, m3 = 2^8
  if (!B) {
    printf("FAIL oracle tables: %s\n", err);
    return 1;
  }
  uint64_t par[10];
  ora_bsgs_params(B, par);
  const uint64_t m = par[0], m2 = par[1], m3 = par[2];
  // tables in the device layout
  std::vector<CPt> gtab(32 * 256);
  for (int i = 0; i < 32; ++i)
    for (int b = 1; b < 256; ++b) {
      ora_u256 k = {{0, 0, 0, 0}};
      k.w[i / 8] = (uint64_t)b << (8 * (i % 8));
      ora_point P;
      ora_compute_pubkey(&P, &k);
      gtab[256 * i + b - 1] = cpt_of(P);
    }
  uint8_t a2b[32 * 64], a3b[32 * 64];
  ora_bsgs_amp_table(B, 2, a2b);
  ora_bsgs_amp_table(B, 3, a3b);
  std::vector<CPt> amp2(32), amp3(32);
  for (int i = 0; i < 32; ++i) {
    amp2[i] = cpt_be(a2b + 64 * i);
    amp3[i] = cpt_be(a3b + 64 * i);
  }
  std::vector<uint8_t> l2, l3, bp(16 * m3);
  const ora_bloom* b2 = ora_bsgs_bloom(B, 2, 0);
  const ora_bloom* b3 = ora_bsgs_bloom(B, 3, 0);
  for (int s = 0; s < 256; ++s) {
    const ora_bloom* x = ora_bsgs_bloom(B, 2, s);
    l2.insert(l2.end(), x->bf, x->bf + x->bytes);
    x = ora_bsgs_bloom(B, 3, s);
    l3.insert(l3.end(), x->bf, x->bf + x->bytes);
  }
  memcpy(bp.data(), ora_bsgs_bptable(B), 16 * m3);
  auto geom = [](const ora_bloom* b) {
    BloomGeom g;
    g.bytes_per_sub = b->bytes;
    g.bits = b->bits;
    g.magic = (uint64_t)(((unsigned __int128)1 << 64) / b->bits);
    g.wrap = (uint64_t)(((unsigned __int128)1 << 64) % b->bits);
    g.hashes = b->hashes;
    return g;
  };
  CheckTables T;
  T.gtab = gtab.data();
  T.amp2 = amp2.data();
  T.amp3 = amp3.data();
  T.l2 = l2.data();
  T.l3 = l3.data();
  T.bp = bp.data();
  T.g2 = geom(b2);
  T.g3 = geom(b3);
  T.n_bp = m3;
  T.m_double = u8_of(u64v(2 * m));
  T.m2_double = u8_of(u64v(2 * m2));
  T.m3 = u8_of(u64v(m3));
  T.m3_double = u8_of(u64v(2 * m3));

  // candidates
  std::vector<Case> cases;
  for (int c = 0; c < 48; ++c) {             // planted: key = base + a*2m + off, off across the window
    Case x;
    x.base = {{splitmix(), splitmix() & 0xffff, 0, 0}};
    x.a = (uint32_t)(splitmix() % 4096);
    const uint64_t off = splitmix() % (2 * m + 64);
    ora_u256 key = add(add(x.base, mul(u64v(2 * m), x.a)), u64v(off));
    ora_compute_pubkey(&x.target, &key);
    x.kind = "planted";
    cases.push_back(x);
  }
  for (int c = 0; c < 16; ++c) {             // the third check's AddDirect(P, -P) special case
    Case x;
    x.base = {{splitmix(), 0, 0, 0}};
    x.a = (uint32_t)(splitmix() % 4096);
    const uint32_t i2 = (uint32_t)(splitmix() % 32), i = (uint32_t)(splitmix() % 32);
    ora_u256 key = add(add(x.base, mul(u64v(2 * m), x.a)), mul(u64v(2 * m2), i2));
    key = add(key, add(mul(u64v(2 * m3), i), u64v(m3)));
    ora_compute_pubkey(&x.target, &key);
    x.kind = "special";
    cases.push_back(x);
  }
  for (int c = 0; c < 32; ++c) {             // random: nothing to find
    Case x;
    x.base = {{splitmix(), splitmix(), splitmix() >> 8, 0}};
    x.a = (uint32_t)splitmix();
    ora_u256 key = {{splitmix(), splitmix(), splitmix(), splitmix() >> 4}};
    ora_compute_pubkey(&x.target, &key);
    x.kind = "random";
    cases.push_back(x);
  }

  int fails = 0, found = 0, l2h = 0, l3h = 0, bph = 0, special_found = 0;
  std::vector<CheckResult> results;
  std::vector<int> founds;
  auto run_on = [&](const char* phase, const std::vector<Case>& cs, size_t ncases) {
    results.clear();
    founds.clear();
    for (size_t c = 0; c < ncases; ++c) {
      const Case& x = cs[c];
      ora_u256 okey = {{0, 0, 0, 0}};
      const int ofound = ora_bsgs_secondcheck(B, &x.base, x.a, &x.target, &okey);
      CheckResult r{};
      const bool gfound = second_check(T, u8_of(x.base), x.a, cpt_of(x.target), r);
      results.push_back(r);
      founds.push_back(ofound);
      found += gfound;
      l2h += r.l2_hits;
      l3h += r.l3_hits;
      bph += r.bp_hits;
      if (gfound && !strcmp(x.kind, "special")) special_found++;
      const ora_u256 gk = ora_of(r.key);
      if (ofound != (int)gfound || (ofound && ora_u256_cmp(&okey, &gk) != 0)) {
        char h1[65], h2[65];
        ora_u256_to_hex(&okey, h1);
        ora_u256_to_hex(&gk, h2);
        printf("FAIL %s case %zu (%s): oracle %d %s, device code %d %s\n", phase, c, x.kind, ofound, h1, (int)gfound, h2);
        fails++;
      }
    }
  };
  auto run = [&](const char* phase, size_t ncases) { run_on(phase, cases, ncases); };
  run("real", cases.size());
  printf("real tables: %zu candidates, %d found (%d special), l2 hits %d, l3 hits %d, bPtable hits %d\n", cases.size(),
         found, special_found, l2h, l3h, bph);
  if (found < 16 || special_found < 8 || bph == 0) {
    printf("FAIL too few paths exercised\n");
    fails++;
  }

  // ---- directed classes (tests/check_cases.py) --------------------------------------------------------------
  const std::vector<uint8_t> l2_real = l2, l3_real = l3, bp_real = bp;
  std::vector<ora_point> oamp2(32), oamp3(32);
  for (int i = 0; i < 32; ++i) {
    ora_u256_from_be(&oamp2[i].x, a2b + 64 * i);
    ora_u256_from_be(&oamp2[i].y, a2b + 64 * i + 32);
    ora_u256_set64(&oamp2[i].z, 1);
    ora_u256_from_be(&oamp3[i].x, a3b + 64 * i);
    ora_u256_from_be(&oamp3[i].y, a3b + 64 * i + 32);
    ora_u256_set64(&oamp3[i].z, 1);
  }
  auto blooms_to_device = [&]() {             // the oracle's sub-blooms as they stand -> the tables under test
    size_t o2 = 0, o3 = 0;
    for (int s = 0; s < 256; ++s) {
      const ora_bloom* x = ora_bsgs_bloom(B, 2, s);
      memcpy(l2.data() + o2, x->bf, x->bytes);
      o2 += x->bytes;
      x = ora_bsgs_bloom(B, 3, s);
      memcpy(l3.data() + o3, x->bf, x->bytes);
      o3 += x->bytes;
    }
  };
  auto blooms_set = [&](const std::vector<uint8_t>* v2, const std::vector<uint8_t>* v3, int fill) {
    size_t o2 = 0, o3 = 0;
    for (int s = 0; s < 256; ++s) {
      ora_bloom* x = const_cast<ora_bloom*>(ora_bsgs_bloom(B, 2, s));
      if (v2) memcpy(x->bf, v2->data() + o2, x->bytes); else memset(x->bf, fill, x->bytes);
      o2 += x->bytes;
      x = const_cast<ora_bloom*>(ora_bsgs_bloom(B, 3, s));
      if (v3) memcpy(x->bf, v3->data() + o3, x->bytes); else memset(x->bf, fill, x->bytes);
      o3 += x->bytes;
    }
    blooms_to_device();
  };
  auto bloom_add = [&](int level, const ora_u256& x) {
    uint8_t xb[32];
    ora_u256_to_be(&x, xb);
    ora_bloom_add(const_cast<ora_bloom*>(ora_bsgs_bloom(B, level, xb[0])), xb, 32);
  };
  // Q = target - base*G and the 32 x of Q + amp[i], by the oracle's own calls
  auto batch_x = [&](const ora_u256& base, const ora_point& target, const std::vector<ora_point>& amp, ora_u256* xs) {
    ora_point bpnt, aux, Q, QA;
    ora_compute_pubkey(&bpnt, &base);
    ora_negation(&aux, &bpnt);
    ora_add_direct(&Q, &target, &aux);
    for (int i = 0; i < 32; ++i) {
      ora_add_direct(&QA, &Q, &amp[i]);
      xs[i] = QA.x;
    }
    return Q;
  };
  auto base_of = [&](const Case& x) { return add(x.base, mul(u64v(2 * m), x.a)); };
  auto sub = [](ora_u256 a, const ora_u256& b) {
    ora_u256 r;
    ora_u256_sub(&r, &a, &b);
    return r;
  };
  auto shl = [](unsigned k) {                 // 2^k
    ora_u256 r = {{0, 0, 0, 0}};
    r.w[k / 64] = 1ull << (k % 64);
    return r;
  };
  auto planted = [&](const ora_u256& start, uint32_t a, const ora_u256& key, const char* kind) {
    Case x;
    x.base = start;
    x.a = a;
    ora_compute_pubkey(&x.target, &key);
    x.kind = kind;
    return x;
  };
  auto reset_counts = [&]() { found = l2h = l3h = bph = special_found = 0; };
  const int slots3[3] = {0, 1, 31};

  // Z: dx == 0 inside a batch.  The blooms hold, besides the geometry's, the other 31 x of each aimed batch and of
  // every third check it enters, so a slot next to the zero one with a wrong inverse lowers a count.
  {
    std::vector<Case> z;
    std::vector<int> zlevel, zslot;
    for (int sign = 0; sign < 2; ++sign)
      for (int s = 0; s < 3; ++s) {
        const ora_u256 start = {{splitmix(), (splitmix() & 0x3f) | 0x100, 0, 0}};
        const uint32_t a = (uint32_t)(splitmix() % 4096);
        const ora_u256 off = mul(u64v(m2), 2 * slots3[s] + 1), base = add(start, mul(u64v(2 * m), a));
        z.push_back(planted(start, a, sign == 0 ? add(base, off) : sub(base, off), sign == 0 ? "Z2-amp2" : "Z2+amp2"));
        zlevel.push_back(2);
        zslot.push_back(slots3[s]);
      }
    for (int s = 0; s < 3; ++s) {             // Q' == +AMP3[i] in the third check of i2 = 0 (base2 = base)
      const ora_u256 start = {{splitmix(), (splitmix() & 0x3f) | 0x100, 0, 0}};
      const uint32_t a = (uint32_t)(splitmix() % 4096);
      const ora_u256 base = add(start, mul(u64v(2 * m), a));
      z.push_back(planted(start, a, sub(base, mul(u64v(m3), 2 * slots3[s] + 1)), "Z3+amp3"));
      zlevel.push_back(3);
      zslot.push_back(slots3[s]);
    }
    for (size_t c = 0; c < z.size(); ++c) {
      ora_u256 xs2[32], xs3[32];
      const ora_u256 base = base_of(z[c]);
      const ora_point Q = batch_x(base, z[c].target, oamp2, xs2);
      const std::vector<ora_point>& amp = zlevel[c] == 2 ? oamp2 : oamp3;
      int zeros = 0;
      for (int i = 0; i < 32; ++i) zeros += ora_u256_cmp(&Q.x, &amp[i].x) == 0;
      if (zeros != 1 || ora_u256_cmp(&Q.x, &amp[zslot[c]].x) != 0) {     // the case reaches its slot, and that one alone
        printf("FAIL Z case %zu (%s[%d]) does not put dx == 0 into its slot\n", c, z[c].kind, zslot[c]);
        fails++;
      }
      if (zlevel[c] == 2) {
        for (int i2 = 0; i2 < 32; ++i2) {
          if (i2 == zslot[c]) continue;
          bloom_add(2, xs2[i2]);
          batch_x(add(base, mul(u64v(2 * m2), i2)), z[c].target, oamp3, xs3);
          for (int i = 0; i < 32; ++i) bloom_add(3, xs3[i]);
        }
      } else {
        bloom_add(2, xs2[0]);                 // slot 0's x: a level-2 false positive placed by hand, the key lies below the window
        batch_x(base, z[c].target, oamp3, xs3);
        for (int i = 0; i < 32; ++i)
          if (i != zslot[c]) bloom_add(3, xs3[i]);
      }
    }
    blooms_to_device();
    reset_counts();
    run_on("Z", z, z.size());
    for (size_t c = 0; c < z.size(); ++c) {
      const CheckResult& r = results[c];
      const bool ok = zlevel[c] == 2 ? (!founds[c] && r.l2_hits == 31 && r.l3_hits == 31 * 32)
                                     : (founds[c] && r.l2_hits == 1 && r.l3_hits == (uint32_t)zslot[c]);
      if (!ok) {
        printf("FAIL Z case %zu (%s[%d]): oracle found %d, l2 hits %u, l3 hits %u\n", c, z[c].kind, zslot[c], founds[c],
               r.l2_hits, r.l3_hits);
        fails++;
      }
    }
    printf("Z (dx == 0 in a batch): %zu candidates, %d found, l2 hits %d, l3 hits %d\n", z.size(), found, l2h, l3h);
    blooms_set(&l2_real, &l3_real, 0);
  }

  // K: degenerate bases;  C: carries through several limbs, and a base that wraps past 2^256
  {
    std::vector<Case> k;
    const uint64_t small[3] = {1, 5, 2 * m + 3};
    for (int s = 0; s < 3; ++s) k.push_back(planted(u64v(0), 0, u64v(small[s]), "K-zero"));
    for (int s = 0; s < 2; ++s) {
      const ora_u256 start = {{splitmix(), splitmix() | 1, splitmix() & 0xffffffff, 0}};
      const uint32_t a = s ? 4095 : 0;
      k.push_back(planted(start, a, add(start, mul(u64v(2 * m), a)), "K-target-is-base"));
    }
    reset_counts();
    run_on("K", k, k.size());
    if (found != 0) {
      printf("FAIL K: %d found\n", found);
      fails++;
    }
    printf("K (degenerate bases): %zu candidates, %d found\n", k.size(), found);
    std::vector<Case> cc;
    for (unsigned kk = 32; kk <= 224; kk += 32)
      for (int s = 0; s < 2; ++s) {
        const uint32_t a = s ? 4095 : 1;
        const ora_u256 start = sub(sub(shl(kk), u64v(1)), u64v(splitmix() % (2 * m)));
        cc.push_back(planted(start, a, add(add(start, mul(u64v(2 * m), a)), u64v(splitmix() % (2 * m))), "C-start-below-2^k"));
      }
    const unsigned below[4] = {64, 96, 160, 224};
    for (int s = 0; s < 4; ++s) {             // the candidate's base just below 2^k: base2 and the key sum carry
      const uint32_t a = 4095;
      const uint64_t d = splitmix() % (2 * m - 4 * m2);
      const ora_u256 start = sub(sub(sub(shl(below[s]), u64v(1)), u64v(d)), mul(u64v(2 * m), a));
      cc.push_back(planted(start, a, add(shl(below[s]), u64v(splitmix() % (2 * m - d - 1))), "C-base-below-2^k"));
    }
    reset_counts();
    run_on("C", cc, cc.size());
    if (found != (int)cc.size() || bph < found) {
      printf("FAIL C: %d of %zu found\n", found, cc.size());
      fails++;
    }
    printf("C (carries): %zu candidates, %d found, bPtable hits %d\n", cc.size(), found, bph);
    std::vector<Case> w;
    ora_u256 top = {{~0ull, ~0ull, ~0ull, ~0ull}};
    w.push_back(planted(sub(top, u64v(splitmix() % (2 * m))), 3, {{splitmix(), splitmix(), splitmix(), splitmix() >> 8}}, "C-wrap"));
    reset_counts();
    run_on("C-wrap", w, 1);
    if (found != 0) {
      printf("FAIL C-wrap: found\n");
      fails++;
    }
  }

  // D: runs of three equal 6-byte keys.  Entries p - 1 and p + 1 take entry p's value and keep their index.
  {
    const int centres[18] = {1, 254, 12, 25, 38, 51, 64, 77, 90, 103, 108, 121, 134, 147, 160, 173, 186, 199};
    ora_xvalue* ot = const_cast<ora_xvalue*>(ora_bsgs_bptable(B));
    std::vector<Case> d;
    for (int c = 0; c < 18; ++c)
      for (int sign = 0; sign < 2; ++sign) {
        const uint64_t j = ot[centres[c]].index;
        const ora_u256 start = {{splitmix(), (splitmix() & 0xffff) | 0x100, 0, 0}};
        const uint32_t a = (uint32_t)(splitmix() % 4096);
        const uint64_t i2 = splitmix() % 32, i = splitmix() % 32;
        ora_u256 key = add(add(start, mul(u64v(2 * m), a)), u64v(i2 * 2 * m2 + (2 * i + 1) * m3));
        key = sign ? sub(key, u64v(j + 1)) : add(key, u64v(j + 1));
        d.push_back(planted(start, a, key, sign ? "D-" : "D+"));
      }
    for (int c = 0; c < 18; ++c) {
      memcpy(ot[centres[c] - 1].value, ot[centres[c]].value, 6);
      memcpy(ot[centres[c] + 1].value, ot[centres[c]].value, 6);
    }
    memcpy(bp.data(), ot, 16 * m3);
    reset_counts();
    run_on("D", d, d.size());
    int even_found = 0, odd_found = 0;
    for (size_t c = 0; c < d.size(); ++c) (centres[c / 2] % 2 ? odd_found : even_found) += founds[c];
    printf("D (equal bPtable keys): %zu candidates, oracle finds %d at even centres, %d at odd ones, bPtable hits %d\n",
           d.size(), even_found, odd_found, bph);
    if (even_found != 18 || odd_found != 0 || bph != 36) {     // both outcomes: the probe sequence is observable
      printf("FAIL D: expected the 18 keys at even centres found and the 18 at odd centres lost\n");
      fails++;
    }
    memcpy(ot, bp_real.data(), 16 * m3);
    bp = bp_real;
  }

  // Every x of every batch: blooms that hold exactly the 32 + 32 x 32 x of four nothing-to-find candidates
  {
    std::vector<Case> n;
    for (int c = 0; c < 8; ++c) {
      Case x;
      x.base = {{splitmix(), splitmix(), splitmix() >> 2, 0}};
      x.a = (uint32_t)splitmix();
      ora_u256 key = {{splitmix(), splitmix(), splitmix(), splitmix() >> 6}};
      ora_compute_pubkey(&x.target, &key);
      x.kind = c < 4 ? "pinned" : "unrelated";
      n.push_back(x);
    }
    blooms_set(nullptr, nullptr, 0);
    for (int c = 0; c < 4; ++c) {
      ora_u256 xs2[32], xs3[32];
      const ora_u256 base = base_of(n[c]);
      batch_x(base, n[c].target, oamp2, xs2);
      for (int i2 = 0; i2 < 32; ++i2) {
        bloom_add(2, xs2[i2]);
        batch_x(add(base, mul(u64v(2 * m2), i2)), n[c].target, oamp3, xs3);
        for (int i = 0; i < 32; ++i) bloom_add(3, xs3[i]);
      }
    }
    blooms_to_device();
    reset_counts();
    run_on("pinned", n, n.size());
    for (size_t c = 0; c < n.size(); ++c) {
      const CheckResult& r = results[c];
      const uint32_t e2 = c < 4 ? 32 : 0, e3 = c < 4 ? 1024 : 0;
      if (founds[c] || r.found || r.l2_hits != e2 || r.l3_hits != e3) {
        printf("FAIL pinned case %zu (%s): l2 hits %u of %u, l3 hits %u of %u\n", c, n[c].kind, r.l2_hits, e2, r.l3_hits, e3);
        fails++;
      }
    }
    printf("pinned blooms: 8 candidates, l2 hits %d, l3 hits %d, bPtable hits %d\n", l2h, l3h, bph);
    blooms_set(&l2_real, &l3_real, 0);
  }

  // The U8 helpers against the oracle's integers: runs of all-ones and all-zero limbs, every k and s
  {
    int bad = 0;
    for (int c = 0; c < 4000; ++c) {
      ora_u256 a, mm;
      for (int w = 0; w < 4; ++w) {
        const uint64_t sel = splitmix();
        a.w[w] = (sel & 3) == 0 ? 0 : (sel & 3) == 1 ? ~0ull : (sel & 3) == 2 ? (~0ull << 32) | (uint32_t)splitmix() : splitmix();
        mm.w[w] = (sel & 12) == 0 ? 0 : (sel & 12) == 4 ? ~0ull : splitmix();
      }
      const uint64_t sel = splitmix();
      const uint32_t k = (sel & 3) == 0 ? 0xffffffffu : (sel & 3) == 1 ? 1u : (uint32_t)splitmix();
      const uint64_t s = (sel & 12) == 0 ? ~0ull : (sel & 12) == 4 ? 1ull : (sel & 12) == 8 ? (uint32_t)splitmix() : splitmix();
      U8 r;
      u8_mul32_add(r, u8_of(mm), k, u8_of(a));
      ora_u256 e = add(mul(mm, k), a), g = ora_of(r);
      bad += ora_u256_cmp(&e, &g) != 0;
      u8_addsub64(r, u8_of(a), s, false);
      e = add(a, u64v(s));
      g = ora_of(r);
      bad += ora_u256_cmp(&e, &g) != 0;
      u8_addsub64(r, u8_of(a), s, true);
      e = sub(a, u64v(s));
      g = ora_of(r);
      bad += ora_u256_cmp(&e, &g) != 0;
    }
    if (bad) {
      printf("FAIL U8 helpers: %d of 12000 results differ from the oracle's integers\n", bad);
      fails++;
    }
  }

  // search_bp against the oracle's bsgs_searchbinary at every table size from 1 to 300, runs of equal keys included:
  // the landed index.  At 256 entries every interval the search halves is a power of two; elsewhere `half` rounds.
  {
    int bad = 0, searches = 0, hits = 0;
    for (int n = 1; n <= 300; ++n) {
      std::vector<uint64_t> keys(n);
      uint64_t k = 1 + splitmix() % 1000;
      for (int i = 0; i < n; ++i) {
        keys[i] = k;
        if (splitmix() % 4) k += 1 + splitmix() % 100000;       // one step in four repeats the key
      }
      std::vector<ora_xvalue> tab(n);
      for (int i = 0; i < n; ++i) {
        for (int b = 0; b < 6; ++b) tab[i].value[b] = (uint8_t)(keys[i] >> (8 * (5 - b)));
        tab[i].pad[0] = tab[i].pad[1] = 0;
        tab[i].index = (uint64_t)(n - 1 - i);
      }
      for (int i = 0; i < n; ++i)
        for (int dlt = -1; dlt <= 1; ++dlt) {
          const uint64_t q = keys[i] + dlt;
          uint8_t xb[32] = {0};
          for (int b = 0; b < 6; ++b) xb[16 + b] = (uint8_t)(q >> (8 * (5 - b)));
          uint64_t oi = 0, gi = 0;
          const int of = ora_bsgs_searchbinary(tab.data(), xb, n, &oi);
          const bool gf = search_bp((const uint8_t*)tab.data(), n, xb, gi);
          bad += of != (int)gf || (of && oi != gi);
          hits += of;
          searches++;
        }
    }
    if (bad || hits < searches / 4) {
      printf("FAIL search_bp: %d of %d searches differ from the oracle's bsgs_searchbinary (%d hits)\n", bad, searches, hits);
      fails++;
    }
    printf("search_bp at 1..300 entries: %d searches, %d hits\n", searches, hits);
  }

  // dense blooms: every level-2/3 bit set in both implementations
  for (int s = 0; s < 256; ++s) {
    ora_bloom* x = const_cast<ora_bloom*>(ora_bsgs_bloom(B, 2, s));
    memset(x->bf, 0xff, x->bytes);
    x = const_cast<ora_bloom*>(ora_bsgs_bloom(B, 3, s));
    memset(x->bf, 0xff, x->bytes);
  }
  memset(l2.data(), 0xff, l2.size());
  memset(l3.data(), 0xff, l3.size());
  found = l2h = l3h = bph = special_found = 0;
  run("dense", 24);
  printf("dense blooms: 24 candidates, %d found, l2 hits %d, l3 hits %d, bPtable hits %d\n", found, l2h, l3h, bph);
  ora_bsgs_free(B);
  printf(fails ? "FAIL %d\n" : "ok\n", fails);
  return fails ? 1 : 0;
}
