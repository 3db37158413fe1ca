// Host-side run of device/minikey.hpp (compiled for the CPU, with the address and undefined-behaviour sanitizers by
// tests/test_native_mini.py), the code the -m minikeys kernels run.  Test infrastructure.  Modes (argv[1]), each
// reading the file argv[2] and printing one line per record for the Python side to compare with its own big integers,
// hashlib and the oracle:
//   add   records of 21 digit bytes, u64 offset, u32 steps:
//           "<ok> <digits hex> <ok2> <digits hex>": mini_add(d, offset), then `steps` times mini_carry(d, 20) on it
//   pack  58 alphabet bytes, then records of 21 digit bytes:
//           "<digest of the 23-byte shape> <digest of the 22-byte shape> <mini_valid> <mini_key hex>"
//   mul   argv[3] = window width; records of 32-byte big-endian scalars; the table is host/mini_table.cpp's:
//           "1" for a bad key, else "0 <x||y hex>" of mini_mul_g; exits 1 if that differs from the host's mul_g
#include "../../keyhuntm1cpu_amd/csrc/device/minikey.hpp"
#include "../../keyhuntm1cpu_amd/csrc/host/mini_table.hpp"
#include "../../keyhuntm1cpu_amd/csrc/host/secp_host.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
using namespace khb;

static std::vector<uint8_t> slurp(const char* path) {
  std::vector<uint8_t> v;
  FILE* f = fopen(path, "rb");
  if (!f) exit(2);
  uint8_t buf[4096];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
  fclose(f);
  return v;
}

static void hex(const uint8_t* p, size_t n) {
  for (size_t i = 0; i < n; ++i) printf("%02x", p[i]);
}

static void digest(const uint32_t s[8]) {
  for (int i = 0; i < 8; ++i) printf("%08x", s[i]);
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const std::vector<uint8_t> in = slurp(argv[2]);
  const std::string mode = argv[1];
  if (mode == "add") {
    const size_t rec = 21 + 8 + 4;
    for (size_t o = 0; o + rec <= in.size(); o += rec) {
      std::vector<uint8_t> d(in.begin() + o, in.begin() + o + 21);     // exactly 21 bytes on the heap
      uint64_t off;
      uint32_t steps;
      memcpy(&off, &in[o + 21], 8);
      memcpy(&steps, &in[o + 29], 4);
      const bool ok = mini_add(d.data(), off);
      printf("%d ", ok ? 1 : 0);
      hex(d.data(), 21);
      bool ok2 = true;
      for (uint32_t t = 0; t < steps; ++t) ok2 = mini_carry(d.data(), 20) && ok2;
      printf(" %d ", ok2 ? 1 : 0);
      hex(d.data(), 21);
      printf("\n");
    }
  } else if (mode == "pack") {
    if (in.size() < 58) return 2;
    std::vector<uint8_t> alpha(in.begin(), in.begin() + 58);
    for (size_t o = 58; o + 21 <= in.size(); o += 21) {
      std::vector<uint8_t> d(in.begin() + o, in.begin() + o + 21);
      for (int check = 1; check >= 0; --check) {
        uint32_t w[16], s[8];
        mini_pack(w, alpha.data(), d.data(), check != 0);
        sha256_init(s);
        sha256_block(s, w);
        digest(s);
        printf(" ");
      }
      // the filter's own path: the head words and what a run shares (mini_pre), then word 0 from w[5] alone
      uint32_t head[5], s[8];
      MiniPre pre;
      mini_pack_head(head, alpha.data(), d.data());
      mini_pre(pre, head, 0xB8u);
      mini_sha(s, head, mini_w5_check(alpha[d[19]], alpha[d[20]]), 0xB8u);
      if (mini_sha_word0(pre, mini_w5_check(alpha[d[19]], alpha[d[20]]), 0xB8u) != s[0]) return 1;
      if (((s[0] >> 24) == 0) != mini_valid(alpha.data(), d.data())) return 1;
      printf("%d ", mini_valid(alpha.data(), d.data()) ? 1 : 0);
      U8 k;
      mini_key(k, alpha.data(), d.data());
      for (int i = 7; i >= 0; --i) printf("%08x", k.v[i]);
      printf("\n");
    }
  } else if (mode == "mul") {
    if (argc < 4) return 2;
    const uint32_t w = (uint32_t)atoi(argv[3]);
    const std::vector<uint8_t> tb = mini_table_be(w, 4);
    if (tb.size() != 64 * mini_table_points(w)) return 2;
    std::vector<CPt> tab(tb.size() / 64);                             // exactly the table: a read past it is reported
    for (size_t i = 0; i < tab.size(); ++i) {
      fe_from_be(tab[i].x, tb.data() + 64 * i);
      fe_from_be(tab[i].y, tb.data() + 64 * i + 32);
    }
    int bad = 0;
    for (size_t o = 0; o + 32 <= in.size(); o += 32) {
      Fe f;
      fe_from_be(f, &in[o]);
      U8 k;
      memcpy(k.v, f.v, sizeof k.v);
      CPt r;
      mini_mul_g(r, k, tab.data(), w);     // run for bad keys too: it must stay inside the table
      if (!mini_scalar_ok(k)) {
        printf("1\n");
        continue;
      }
      uint8_t xy[64], want[64];
      fe_to_be(xy, r.x);
      fe_to_be(xy + 32, r.y);
      pt_to_be(want, mul_g(U256::from_be(&in[o])));
      if (memcmp(xy, want, 64) != 0 && !bad++) {
        fprintf(stderr, "w = %u, scalar ", w);
        for (int i = 0; i < 32; ++i) fprintf(stderr, "%02x", in[o + i]);
        fprintf(stderr, ": mini_mul_g differs from mul_g\n");
      }
      printf("0 ");
      hex(xy, 64);
      printf("\n");
    }
    return bad ? 1 : 0;
  } else {
    return 2;
  }
  return 0;
}
