// keyhunt_amd — keyhunt-compatible CLI on MI355X: the mode table, main() and the `-m bsgs` run.
//
// Options are parsed by cli.cpp.  The -m bsgs run follows keyhunt.cpp main(): -n (665-668, 1052-1067), target
// file (962-1044), geometry/bloom prints (1045-1303), found-key output (3950-3981), stats line (2145-2252).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/random.h>
#include <unistd.h>

#include <mutex>
#include <string>
#include <vector>

#include "../../../include/khbsgs.h"
#include "bsgs_host.hpp"
#include "cli.hpp"
#include "engine.hpp"

using namespace khb;

namespace {

const char* kVersion = "1.0.0 keyhunt_amd (MI355X BSGS engine)";

int run_bsgs_mode(const CliOptions& o);

// Adding a mode: its row here and its word in the -m line of menu(); the refusal in main() names the rows still
// without a runner.
const CliMode kModes[] = {{"xpoint", run_address_mode}, {"address", run_address_mode}, {"bsgs", run_bsgs_mode},
                          {"rmd160", run_address_mode}, {"pub2rmd", nullptr},          {"minikeys", nullptr},
                          {"vanity", nullptr}};

void menu() {
  printf("\nUsage:\n");
  printf("-h          show this help\n");
  printf("-B Mode     BSGS now have some modes <sequential, backward, both, random, dance>\n");
  printf("-b bits     For some puzzles you only need some numbers of bits in the test keys.\n");
  printf("-c crypto   Search for specific crypto. <btc, eth> valid only w/ -m address\n");
  printf("-f file     Specify file name with public keys (02/03 compressed or 04 uncompressed hex)\n");
  printf("-k value    Use this only with bsgs mode, k value is factor for M, more speed but more RAM use wisely\n");
  printf("-m mode     mode of search for cryptos. (bsgs, address, rmd160, xpoint) default: bsgs\n");
  printf("            -m xpoint: -f holds public keys or x values (64, 66 or 130 hex), searched by x\n");
  printf("-M          Matrix screen, feel like a h4x0r, but performance will dropped\n");
  printf("-n number   Use -n to set the N for the BSGS process. Bigger N more RAM needed\n");
  printf("-q          Quiet the thread output\n");
  printf("-r SR:EN    StarRange:EndRange, the end range can be omitted for search from start range to N-1 ECC value\n");
  printf("-R          Random, this is the default behavior\n");
  printf("-s ns       Number of seconds for the stats output, 0 to omit output.\n");
  printf("-t tn       CPU threads for table build and candidate confirmation\n");
  printf("--cpu-build build the baby-step tables on the CPU (default: on the first GPU)\n");
  printf("--resident  -m bsgs, large -k: build the level-1 bloom and its gate on every GPU and keep them there\n");
  printf("            (never in host memory; not with -S or --cpu-build)\n");
  printf("-6          to skip sha256 Checksum on data files\n");
  printf("--gpu       use the GPU path (always on: keyhunt_amd has no CPU giant-step path)\n");
  printf("-g ids      GPU device ids, comma separated (default 0)\n");
  printf("--gpu-blocks n   persistent workgroups per GPU (256 lanes each)\n");
  printf("--check where    confirm candidates (second/third check) on the host, the gpu, or auto (default host)\n");
  printf("--no-gate   probe every giant step in the level-1 bloom (no level-0 gate; same keys, more candidates)\n");
  printf("\nExample:\n\n./keyhunt_amd -m bsgs -f tests/63.pub -b 63 -q -g 0\n\n");
  exit(EXIT_FAILURE);
}

U256 rand_range(const U256& lo, const U256& hi) {
  uint8_t b[32];
  if (getrandom(b, sizeof b, 0) != (ssize_t)sizeof b) {
    fprintf(stderr, "[E] Error getrandom() ?\n");
    exit(EXIT_FAILURE);
  }
  U256 v = U256::from_be(b), r;
  U256 span = hi - lo;
  if (span.is_zero()) return lo;
  U256::divmod(v, span, nullptr, &r);
  return lo + r;
}

int run_bsgs_mode(const CliOptions& o) {
  // -e / -I outside the sub-mode "both" are ignored by -m bsgs, as there (keyhunt.cpp:780-789)
  check_resident_conflict(o);
  printf("[+] Mode BSGS %s\n", kBsgsModes[o.bsgs_mode]);
  const char* file = o.file ? o.file : "addresses.txt";   // default_fileName, keyhunt.cpp:231
  SearchConfig cfg;
  cfg.devices = o.devices;
  if (o.gpu_blocks) cfg.lanes = o.gpu_blocks * 256u;
  cfg.max_chunks = o.max_chunks;
  cfg.check_mode = o.check_mode;
  cfg.use_gate = o.use_gate;
  cfg.chunk_mode = o.bsgs_mode;                     // sequential, backward, both, random, dance
  cfg.random_chunks = o.bsgs_mode == kBsgsRandom;
  cfg.check_threads = o.threads;
  CliRange range = resolve_range(o);                // keyhunt.cpp:816-838, 1089-1119

  // ---- target file (keyhunt.cpp:962-1044)
  printf("[+] Opening file %s\n", file);
  FILE* fd = fopen(file, "rb");
  if (!fd) { fprintf(stderr, "[E] Can't open file %s\n", file); exit(EXIT_FAILURE); }
  std::vector<Target> targets;
  int counted = 0;
  char line[1024];
  while (fgets(line, 1022, fd)) {
    trim(line);
    if (strlen(line) >= 66) counted++;
  }
  if (counted == 0) { fprintf(stderr, "[E] There is no valid data in the file\n"); exit(EXIT_FAILURE); }
  fseek(fd, 0, SEEK_SET);
  while (fgets(line, 1022, fd)) {
    trim(line);
    if (strlen(line) < 66) continue;
    std::vector<std::string> t = tokens(line);
    if (t.empty()) continue;
    const std::string& tok = t[0];
    if (tok.size() == 66 || tok.size() == 130) {
      Target tg;
      std::string e;
      if (parse_pubkey_hex(tok.c_str(), tg.p, tg.compressed, &e)) targets.push_back(tg);
      else printf("%s\n", e.c_str());
    } else {
      printf("Invalid length: %s\n", tok.c_str());
    }
  }
  fclose(fd);
  if (targets.empty()) { fprintf(stderr, "[E] The file don't have any valid publickeys\n"); exit(EXIT_FAILURE); }
  printf("[+] Added %u points from file\n", (unsigned)targets.size());

  // ---- geometry (keyhunt.cpp:1045-1213)
  Geometry geo;
  std::string err;
  if (!make_geometry(o.str_n, o.kfactor, geo, err)) { fprintf(stderr, "%s\n", err.c_str()); exit(EXIT_FAILURE); }
  if (o.flag_bits && !range.have) {
    U256::from_hex(o.bits_min.c_str(), range.start);
    U256::from_hex(o.bits_max.c_str(), range.end);
    printf("[+] Bit Range %i\n", o.bitrange);
    printf("[+] -- from : 0x%s\n", o.bits_min.c_str());
    printf("[+] -- to   : 0x%s\n", o.bits_max.c_str());
    range.have = true;
  } else if (range.have) {
    printf("[+] Range \n");
    printf("[+] -- from : 0x%s\n", o.range_start.c_str());
    printf("[+] -- to   : 0x%s\n", o.range_end.c_str());
  }
  if (!range.have) {   // random start, keyhunt.cpp:1106-1112
    range.start = rand_range(U256(1), secp_order());
    range.end = secp_order();
  }
  if (range.end - range.start < geo.N) { fprintf(stderr, "[E] the given range is small\n"); exit(EXIT_FAILURE); }
  printf("[+] N = 0x%s\n", geo.N.hex().c_str());

  // ---- tables; -S: the reference's table files in the working directory (keyhunt.cpp:1373-1613, 1881-2025)
  print_table_sizes(geo);
  Tables T;
  TableSource src;
  src.dir = o.save_read_file ? "." : nullptr;
  src.skip_checksum = o.skip_checksum;
  src.threads = o.threads;
  src.device = o.cpu_build ? -1 : cfg.devices[0];   // baby steps on the first GPU (identical tables; tests/test_gpu_tables.py)
  src.resident = o.resident;
  src.say = [](const std::string& m) { printf("%s", m.c_str()); fflush(stdout); };
  src.progress = [](uint64_t d, uint64_t tot) {
    printf("\r[+] processing %llu/%llu bP points : %i%%\r", (unsigned long long)d, (unsigned long long)tot,
           (int)((double)d / (double)tot * 100));
    fflush(stdout);
  };
  src.after_load = [](uint32_t have) {
    if (have && have != kFileAll && (have & kFileL1))
      printf("[I] We need to recalculate some files, don't worry this is only 3%% of the previous work\n");
  };
  src.after_build = [&](uint32_t have) {
    const uint64_t ext = ((have & kFileL1) || o.resident) ? geo.m2 : geo.l1ext;
    printf("\r[+] processing %llu/%llu bP points : 100%%     \n", (unsigned long long)ext, (unsigned long long)ext);
    if (!(have & kFileBp)) printf("[+] Sorting %llu elements... Done!\n", (unsigned long long)geo.m3);
  };
  if (!T.obtain(geo, src, nullptr, err)) { fprintf(stderr, "%s\n", err.c_str()); exit(EXIT_FAILURE); }

  // ---- search
  std::mutex out_mu;
  SearchCallbacks cb;
  cb.on_found = [&](int k, const U256& key) {   // keyhunt.cpp:3950-3971
    const std::string kh = key.hex(), ph = pubkey_hex(mul_g(key), targets[k].compressed);
    append_found(out_mu, "Key found privkey " + kh + "\nPublickey " + ph + "\n",
                 "[+] Thread Key found privkey " + kh + "   \n[+] Publickey " + ph + "\n");
  };
  cb.on_chunk = [&](const U256& base) {             // keyhunt.cpp:3846-3860
    if (o.quiet) return;
    std::lock_guard<std::mutex> lk(out_mu);
    if (o.matrix) printf("[+] Thread 0x%s \n", base.hex().c_str());
    else { printf("\r[+] Thread 0x%s   \r", base.hex().c_str()); fflush(stdout); }
  };
  cb.on_warning = [&](const std::string& m) {
    std::lock_guard<std::mutex> lk(out_mu);
    fprintf(stderr, "%s\n", m.c_str());
  };
  std::vector<int> found;
  std::vector<U256> keys;
  SearchStats stats;
  Session session;
  StatsTicker ticker(o.out_seconds, o.matrix, out_mu, [&](uint64_t seconds) {
    // steps += 2 per chunk, keys = steps * N
    const U256 total = geo.N_double * __atomic_load_n(&stats.chunks, __ATOMIC_RELAXED);
    char gs[64];
    snprintf(gs, sizeof gs, " [%.3f G giant-steps/s]",
             (double)__atomic_load_n(&stats.giant_steps, __ATOMIC_RELAXED) / seconds / 1e9);
    return speed_line(total, seconds) + gs;
  });
  int rc = session.open(T, cfg, err);
  if (!rc) {
    print_resident_lines(session);
    rc = session.run(targets, range.start, range.end, cb, found, keys, stats, err, cfg.max_chunks, cfg.random_chunks);
  }
  ticker.stop();
  if (rc) { fprintf(stderr, "%s\n", err.c_str()); exit(EXIT_FAILURE); }
  int all = 1;
  for (int f : found) all &= f;
  if (all) {
    printf("All points were found\n");
    exit(EXIT_FAILURE);   // the reference exits with status 1 on success (keyhunt.cpp:3979-3980)
  }
  printf("\nEnd\n");
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  setvbuf(stdout, nullptr, _IOLBF, 0);
  printf("[+] Version %s\n", kVersion);
  CliOptions o;
  parse_keyhunt_args(argc, argv, o, {kModes, (int)(sizeof kModes / sizeof kModes[0]), menu});
  // keyhunt.cpp:780-789: compared with MODE_BSGS (2), i.e. the -B sub-mode "both", whatever -m is
  if (o.bsgs_mode == kBsgsBoth && o.endomorphism) {
    fprintf(stderr, "[E] Endomorphism doesn't work with BSGS\n");
    exit(EXIT_FAILURE);
  }
  if (o.bsgs_mode == kBsgsBoth && o.stride) {
    fprintf(stderr, "[E] Stride doesn't work with BSGS\n");
    exit(EXIT_FAILURE);
  }
  const CliMode& m = kModes[o.mode];
  if (!m.run) {
    fprintf(stderr, "[E] keyhunt_amd implements -m bsgs, -m address, -m rmd160 and -m xpoint; -m minikeys and -m vanity "
                    "remain (mode %s is not available)\n",
            m.name);
    exit(EXIT_FAILURE);
  }
  return m.run(o);
}
