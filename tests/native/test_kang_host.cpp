// The kangaroo search's host pieces that need no device (host/kang_host.hpp), as a stand-alone program for the
// sanitizers:
//   table <n> <log2_slots>   n distinguished points into a table of 2^log2_slots slots, against std::map: first
//                            inserts, repeated x (the stored entry comes back unchanged), growth and probing; prints
//                            "size slots grown probes"
//   modn <file>              pairs a, b (32 bytes BE each, both < n): prints a + b, a - b and -a mod n as hex
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <vector>

#include "../../keyhuntm1cpu_amd/csrc/host/kang_host.hpp"

using namespace khb;

static uint64_t rng_state = 0x1234567;
static uint64_t rnd() {
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
      return 1;                                               \
    }                                                         \
  } while (0)

static int table_mode(size_t n, uint32_t log2_slots) {
  KangDpTable T(log2_slots);
  std::map<std::vector<uint64_t>, std::pair<uint64_t, uint32_t>> ref;
  std::vector<U256> xs;
  for (size_t i = 0; i < n; ++i) {
    U256 x, d;
    for (int k = 0; k < 4; ++k) x.w[k] = rnd();
    x.w[0] &= ~0xFFFF00000000ull;          // a distinguished x: 16 zero bits where the DP test looks
    if (i % 7 == 3 && !xs.empty()) x = xs[rnd() % xs.size()];      // an x already stored
    if (i % 11 == 5) {                     // x that differ only in the top word
      x = U256(42);
      x.w[3] = rnd() % 64;
    }
    d.w[0] = i;
    d.w[3] = rnd();
    const uint32_t kind = (uint32_t)(rnd() & 1);
    const std::vector<uint64_t> key(x.w, x.w + 4);
    const KangEntry* e = T.insert(x, d, kind);
    auto it = ref.find(key);
    if (it == ref.end()) {
      CHECK(e == nullptr);
      ref[key] = {i, kind};
      xs.push_back(x);
    } else {
      CHECK(e != nullptr && e->x == x && e->d.w[0] == it->second.first && e->kind == it->second.second);
    }
    CHECK(T.size() == ref.size());
    CHECK(2 * T.size() <= T.slots());
  }
  for (const U256& x : xs) {
    const KangEntry* e = T.lookup(x);
    CHECK(e && e->x == x && e->d.w[0] == ref[std::vector<uint64_t>(x.w, x.w + 4)].first);
  }
  U256 absent(7);
  absent.w[2] = 99;
  CHECK(T.lookup(absent) == nullptr);
  printf("%zu %zu %u %llu\n", T.size(), T.slots(), T.grown(), (unsigned long long)T.probes());
  return 0;
}

static int modn_mode(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) return 2;
  uint8_t buf[64];
  while (fread(buf, 1, 64, f) == 64) {
    const U256 a = U256::from_be(buf), b = U256::from_be(buf + 32);
    printf("%s %s %s\n", kang_add_mod_n(a, b).hex().c_str(), kang_sub_mod_n(a, b).hex().c_str(),
           kang_neg_mod_n(a).hex().c_str());
  }
  fclose(f);
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 4 && !strcmp(argv[1], "table")) return table_mode(strtoull(argv[2], nullptr, 10), atoi(argv[3]));
  if (argc >= 3 && !strcmp(argv[1], "modn")) return modn_mode(argv[2]);
  fprintf(stderr, "usage: %s table <n> <log2_slots> | modn <file>\n", argv[0]);
  return 2;
}
