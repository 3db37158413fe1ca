// keyhunt_amd -m address / -m rmd160 / -m xpoint: keyhunt.cpp main() (800-960 setup and prints, 2145-2252 stats)
// and thread_process's output (writekey, keyhunt.cpp:5989-6030; writekeyeth, 6023-6051) over the libkhbsgs address scan.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <mutex>

#include "../../../include/khbsgs.h"
#include "address_host.hpp"
#include "cli.hpp"

namespace khb {

using namespace khbk;   // SearchMode (device/scan_modes.hpp)

namespace {

// writekey (keyhunt.cpp:5989-6030).  xpoint: f.rmd holds the matched bytes of x, not a hash160, and the reference's
// writekey(false, key) prints the hash160 of the uncompressed key (keyhunt.cpp:5996-6000).
void writekey(const AddrFound& f, std::mutex& mu, bool xpoint = false) {
  const Pt pub = mul_g(f.key);
  const std::string hexkey = f.key.hex();
  const std::string pubhex = pubkey_hex(pub, f.compressed);
  H160 rmd = f.rmd;
  if (xpoint) hash160_pub(pub, false, rmd.data());
  const std::string addr = rmd_to_address(rmd.data());
  char rmdhex[41];
  for (int i = 0; i < 20; ++i) snprintf(rmdhex + 2 * i, 3, "%02x", rmd[i]);
  const std::string text =
      "Private Key: " + hexkey + "\npubkey: " + pubhex + "\nAddress " + addr + "\nrmd160 " + rmdhex + "\n";
  append_found(mu, text, "\nHit! " + text);
}

// writekeyeth (keyhunt.cpp:6023-6051)
void writekeyeth(const AddrFound& f, std::mutex& mu) {
  const std::string hexkey = f.key.hex();
  char address[43] = "0x";
  for (int i = 0; i < 20; ++i) snprintf(address + 2 + 2 * i, 3, "%02x", f.rmd[i]);
  const std::string text = "Private Key: " + hexkey + "\naddress: " + address + "\n";
  append_found(mu, text, "\n Hit!!!! " + text);
}

}  // namespace

int run_address_mode(const CliOptions& o) {
  const bool xpoint = o.mode == kModeXpoint;
  if (o.eth && o.mode != kModeAddress) {   // -c is "valid only w/ -m address"
    fprintf(stderr, "[E] -c eth is valid only with -m address (-m %s)\n",
            xpoint ? "xpoint searches public-key x values" : "rmd160 searches BTC hash160 values");
    return EXIT_FAILURE;
  }
  if (o.eth && o.endomorphism) {
    // keyhunt.cpp:2772 hashes beta*x a second time where beta^2*x was meant and recovers that slot with
    // lambda^2, so the reference's -c eth -e can print a key that does not own the address
    fprintf(stderr, "[E] -c eth does not work with -e: the reference's ETH endomorphism path hashes beta*x twice "
                    "(beta^2*x is never hashed) and can report a key that does not own the address; it is not "
                    "reproduced\n");
    return EXIT_FAILURE;
  }
  const CliRange range = resolve_range(o);   // keyhunt.cpp:816-838
  if (!o.crypto_set && o.mode == kModeAddress) printf("[+] Setting search for btc adddress\n");   // keyhunt.cpp:812-815
  U256 stride(1);
  if (o.stride) {   // keyhunt.cpp:790-797
    const bool ok = (o.stride[0] == '0' && o.stride[1] == 'x') ? U256::from_hex(o.stride + 2, stride)
                                                                : U256::from_dec(o.stride, stride);
    if (!ok || stride.is_zero()) {
      fprintf(stderr, "[E] invalid stride %s\n", o.stride);
      return EXIT_FAILURE;
    }
    printf("[+] Stride : %s\n", stride.dec().c_str());
  }
  const char* file = o.file ? o.file : "addresses.txt";   // default_fileName
  // range (keyhunt.cpp:844-864)
  U256 start(1), end = secp_order();
  if (range.have) {
    start = range.start;
    end = range.end;
  } else if (o.flag_bits) {
    U256::from_hex(o.bits_min.c_str(), start);
    U256::from_hex(o.bits_max.c_str(), end);
  }
  // -n (keyhunt.cpp:866-887)
  uint64_t n_seq = 0x100000000ull;
  if (o.str_n) {
    const uint64_t v = (o.str_n[0] == '0' && o.str_n[1] == 'x') ? strtoull(o.str_n, nullptr, 16)
                                                                 : strtoull(o.str_n, nullptr, 10);
    if (v < 1024) {
      fprintf(stderr, "[I] n value need to be equal or great than 1024, back to defaults\n");
    } else if (v % 1024 != 0) {
      fprintf(stderr, "[I] n value need to be multiplier of  1024\n");
    } else {
      n_seq = v;
    }
  }
  printf("[+] N = %p\n", (void*)n_seq);
  if (o.flag_bits) printf("[+] Bit Range %i\n", o.bitrange);
  else printf("[+] Range \n");
  printf("[+] -- from : 0x%s\n", start.hex().c_str());
  printf("[+] -- to   : 0x%s\n", end.hex().c_str());
  // targets (keyhunt.cpp:6300-6358, 6559-6576)
  AddrTargets T;
  std::string err;
  if (!AddrTargets::load_file(file, o.bloom_multiplier, T, &err,
                              xpoint ? kTargetsXpoint : o.eth ? kTargetsEth : kTargetsBtc)) {
    fprintf(stderr, "[E] %s\n[E] Unenexpected error\n", err.c_str());
    return EXIT_FAILURE;
  }
  printf("[+] Allocating memory for %llu elements: %.2f MB\n", (unsigned long long)T.counted,
         (double)(20.0 * (double)T.counted / 1048576.0));
  printf("[+] Bloom filter for %llu elements.\n", (unsigned long long)T.counted);
  printf("[+] Loading data to the bloomfilter total: %.2f MB\n", (double)T.bloom.bytes / 1048576.0);
  for (const std::string& s : T.skipped)
    fprintf(stderr, xpoint ? "[E] Omiting line : %s\n" : "[I] Ommiting invalid line %s\n", s.c_str());
  printf("[+] Sorting data ...");
  printf(" done! %llu values were loaded and sorted\n", (unsigned long long)T.table.size());
  // generator + lane offsets for one chunk of n_seq keys
  AddrGen G;
  const uint32_t gpl = 16;
  G.build(stride, (uint32_t)(n_seq / 1024), gpl, o.threads > 0 ? o.threads : 1);
  AddrConfig cfg;
  // -c eth: one hash per point whatever -l says; -m xpoint: -l is accepted and not used
  cfg.search = encode_search({xpoint ? kFamilyXpoint : o.eth ? kFamilyEth : kFamilyBtc, xpoint || o.eth ? 0 : o.search,
                              o.endomorphism, false});
  cfg.start = start;
  cfg.end = end;
  cfg.n_seq = n_seq;
  cfg.random = o.bsgs_mode == kBsgsRandom;   // -R
  cfg.devices = o.devices;
  cfg.lanes = o.gpu_blocks * 256u;
  cfg.gpl = gpl;
  cfg.max_chunks = o.max_chunks;
  std::mutex out_mu;
  AddrStats stats;
  std::atomic<uint64_t> keys_done{0};
  AddrCallbacks cb;
  cb.on_found = [&](const AddrFound& f) { o.eth ? writekeyeth(f, out_mu) : writekey(f, out_mu, xpoint); };
  cb.on_warning = [&](const std::string& m) {
    std::lock_guard<std::mutex> lk(out_mu);
    fprintf(stderr, "%s\n", m.c_str());
  };
  cb.on_chunk = [&](const U256& base, int device) {
    if (o.quiet) return;
    std::lock_guard<std::mutex> lk(out_mu);
    printf("\rBase key: %s     \r", base.hex().c_str());
    fflush(stdout);
  };
  // stats line every -s seconds (keyhunt.cpp:2145-2252): keys = groups * 1024, x6 with -e (keyhunt.cpp:2175-2180:
  // every -l mode; x3 for -m xpoint), else x2 for -l compress
  StatsTicker ticker(o.out_seconds, false, out_mu, [&](uint64_t seconds) {
    U256 total(keys_done.load());
    if (o.endomorphism) total = total * (xpoint ? 3u : 6u);   // keyhunt.cpp:2175-2181
    else if (o.search == 1) total = total * 2u;   // also with -c eth, as the reference (keyhunt.cpp:2183-2186)
    return speed_line(total, seconds);
  });
  AddrCallbacks cb2 = cb;
  cb2.on_chunk = [&](const U256& base, int device) {
    cb.on_chunk(base, device);
    keys_done.fetch_add(n_seq);
  };
  const int rc = addr_search(T, G, cfg, cb2, &stats, &err);
  ticker.stop();
  if (rc) {
    fprintf(stderr, "[E] %s\n", err.c_str());
    return EXIT_FAILURE;
  }
  printf("\nEnd\n");
  return 0;
}

}  // namespace khb
