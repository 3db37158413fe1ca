// The front end shared by keyhunt_amd and bsgsd_amd (cli.hpp).  Flags and messages follow keyhunt.cpp main()
// (415-2259): getopt string (489), -b (508-527), -r (678-712, 816-838), -k (595-601), -t, -q, -s, -R/-B (498-507,
// 673-677), found-key output (3950-3981) and the stats line (2145-2252).  GPU selection follows the reference
// README's documented interface (README.md:115-122): --gpu, -g <ids>, --gpu-blocks.
#include "cli.hpp"

#include <ctype.h>
#include <getopt.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>

#include "engine.hpp"   // Session's resident info, Geometry, BloomFilter sizes, kCheck* (headers only)
#include "secp_host.hpp"

namespace khb {

const char* const kBsgsModes[5] = {"sequential", "backward", "both", "random", "dance"};   // keyhunt.cpp:227

namespace {

const char* kLimitPrefix[7] = {"Mkeys/s", "Gkeys/s", "Tkeys/s", "Pkeys/s", "Ekeys/s", "Zkeys/s", "Ykeys/s"};

int index_of(const char* s, const char* const* arr, int n) {
  for (int i = 0; i < n; ++i)
    if (strcmp(s, arr[i]) == 0) return i;
  return -1;
}

}  // namespace

int default_threads() {
  const int n = (int)std::thread::hardware_concurrency();
  return n > 16 ? 16 : n;
}

void trim(char* s) {
  size_t n = strlen(s);
  while (n && strchr(" \t\n\r", s[n - 1])) s[--n] = 0;
  size_t i = 0;
  while (s[i] && strchr(" \t\n\r", s[i])) ++i;
  if (i) memmove(s, s + i, strlen(s + i) + 1);
}

std::vector<std::string> tokens(const char* s) {
  std::string t(s);
  const size_t b = t.find_first_not_of("\t\n\r :"), e = t.find_last_not_of("\t\n\r :");
  std::vector<std::string> out;
  if (b == std::string::npos) return out;
  std::string cur;
  for (size_t i = b; i <= e; ++i) {
    if (strchr(" \t:", t[i])) {
      if (!cur.empty()) out.push_back(cur);
      cur.clear();
    } else {
      cur.push_back(t[i]);
    }
  }
  out.push_back(cur);   // t[e] is no separator
  return out;
}

bool valid_hex(const char* s) {
  for (; *s; ++s)
    if (!isxdigit((unsigned char)*s)) return false;
  return true;
}

std::vector<int> parse_devices(const char* arg) {
  std::vector<int> out;
  for (const std::string& s : tokens(arg)) {
    std::string part;
    for (char ch : s + ",") {
      if (ch == ',') { if (!part.empty()) out.push_back(atoi(part.c_str())); part.clear(); }
      else part.push_back(ch);
    }
  }
  if (out.empty()) out.push_back(0);
  return out;
}

int parse_check_mode(const char* s) {
  if (!strcmp(s, "host")) return kCheckHost;
  if (!strcmp(s, "gpu")) return kCheckDevice;
  if (!strcmp(s, "auto")) return kCheckAuto;
  return -1;
}

bool parse_shared_option(int c, const char* arg, CliOptions& o) {
  switch (c) {
    case '6': o.skip_checksum = true; fprintf(stderr, "[W] Skipping checksums on files\n"); return true;
    case 'k':
      o.kfactor = (int)strtol(arg, nullptr, 10);
      if (o.kfactor <= 0) o.kfactor = 1;
      printf("[+] K factor %i\n", o.kfactor);
      return true;
    case 't':
      o.threads = (int)strtol(arg, nullptr, 10);
      if (o.threads <= 0) o.threads = 1;
      printf(o.threads > 1 ? "[+] Threads : %u\n" : "[+] Thread : %u\n", o.threads);
      return true;
    case 'g': o.devices = parse_devices(arg); return true;
    case kOptCpuBuild: o.cpu_build = true; return true;
    case kOptCheck:                                 // where candidates are confirmed (engine.hpp check_mode)
      if ((o.check_mode = parse_check_mode(arg)) < 0) {
        fprintf(stderr, "[E] --check: host, gpu or auto\n");
        exit(EXIT_FAILURE);
      }
      return true;
    case kOptResident: o.resident = true; return true;   // large -k: level-1 bloom and gate built and kept on each GPU
  }
  return false;
}

void check_resident_conflict(const CliOptions& o) {
  if (!o.resident || !(o.save_read_file || o.cpu_build)) return;
  fprintf(stderr, "[E] --resident builds the level-1 bloom on the GPU and keeps it there: it cannot be combined with %s\n",
          o.save_read_file ? "-S" : "--cpu-build");
  exit(EXIT_FAILURE);
}

void parse_keyhunt_args(int argc, char** argv, CliOptions& o, const CliProgram& prog) {
  static const char* const kSearch[3] = {"uncompress", "compress", "both"};   // keyhunt.cpp:230
  static const char* const kCryptos[2] = {"btc", "eth"};
  static struct option longopts[] = {{"gpu", no_argument, nullptr, 1000},
                                     {"gpu-threads", required_argument, nullptr, 1001},
                                     {"gpu-blocks", required_argument, nullptr, 1002},
                                     {"max-chunks", required_argument, nullptr, 1003},
                                     {"cpu-build", no_argument, nullptr, kOptCpuBuild},
                                     {"check", required_argument, nullptr, kOptCheck},
                                     {"no-gate", no_argument, nullptr, 1006},
                                     {"resident", no_argument, nullptr, kOptResident},
                                     {nullptr, 0, nullptr, 0}};
  optind = 0;   // a fresh scan for every argv
  int c;
  while ((c = getopt_long(argc, argv, "deh6MqRSB:b:c:C:E:f:I:k:l:m:N:n:p:r:s:t:v:G:8:z:g:", longopts, nullptr)) != -1) {
    if (parse_shared_option(c, optarg, o)) continue;
    switch (c) {
      case 'h': prog.menu(); break;
      case 'B': {
        const int v = index_of(optarg, kBsgsModes, 5);
        if (v >= 0) o.bsgs_mode = v; else fprintf(stderr, "[W] Ignoring unknow bsgs mode %s\n", optarg);
        break;
      }
      case 'b':
        o.bitrange = (int)strtol(optarg, nullptr, 10);
        if (o.bitrange > 0 && o.bitrange <= 256) {
          U256 mn = U256(1).shl(o.bitrange - 1), mx = U256(1).shl(o.bitrange);
          if (o.bitrange == 256 || mx > secp_order()) mx = secp_order();
          o.bits_min = mn.hex();
          o.bits_max = mx.hex();
          o.flag_bits = true;
        } else {
          fprintf(stderr, "[E] invalid bits param: %s.\n", optarg);
        }
        break;
      case 'd': printf("[+] Flag DEBUG enabled\n"); break;
      case 'e': o.endomorphism = true; printf("[+] Endomorphism enabled\n"); break;
      case 'c': {
        const int v = index_of(optarg, kCryptos, 2);
        if (v == 1) { o.eth = true; printf("[+] Setting search for ETH adddress.\n"); }
        if (v >= 0) o.crypto_set = true;
        break;
      }
      case 'I': o.stride = optarg; break;
      case 'l':
        switch (index_of(optarg, kSearch, 3)) {
          case 0: o.search = 0; printf("[+] Search uncompress only\n"); break;
          case 1: o.search = 1; printf("[+] Search compress only\n"); break;
          case 2: o.search = 2; printf("[+] Search both compress and uncompress\n"); break;
        }
        break;
      case 'f': o.file = optarg; break;
      case 'M': o.matrix = true; printf("[+] Matrix screen\n"); break;
      case 'm':
        o.mode = -1;
        for (int i = 0; i < prog.mode_count; ++i)
          if (strcmp(optarg, prog.modes[i].name) == 0) o.mode = i;
        if (o.mode < 0) { fprintf(stderr, "[E] Unknow mode value %s\n", optarg); exit(EXIT_FAILURE); }
        // every available mode but bsgs announces itself here; bsgs does with its -B mode, once that is known
        if (o.mode != kModeBsgs && prog.modes[o.mode].run) printf("[+] Mode %s\n", prog.modes[o.mode].name);
        break;
      case 'n': o.str_n = optarg; break;
      case 'q': o.quiet = true; printf("[+] Quiet thread output\n"); break;
      case 'R': printf("[+] Random mode\n"); o.bsgs_mode = kBsgsRandom; break;
      case 'r': {
        const std::vector<std::string> t = tokens(optarg);
        if (t.size() == 1) {
          if (valid_hex(t[0].c_str())) { o.flag_range = true; o.range_start = t[0]; o.range_end = secp_order().hex(); }
          else fprintf(stderr, "[E] Invalid hexstring : %s.\n", t[0].c_str());
        } else if (t.size() == 2) {
          if (valid_hex(t[0].c_str()) && valid_hex(t[1].c_str())) { o.flag_range = true; o.range_start = t[0]; o.range_end = t[1]; }
          else fprintf(stderr, "[E] Invalid hexstring : %s\n", valid_hex(t[0].c_str()) ? t[1].c_str() : t[0].c_str());
        } else {
          printf("[E] Unknow number of Range Params: %i\n", (int)t.size());
        }
        break;
      }
      case 's':
        o.out_seconds = strtoull(optarg, nullptr, 10);
        if (o.out_seconds == 0) printf("[+] Turn off stats output\n");
        else printf("[+] Stats output every %llu seconds\n", (unsigned long long)o.out_seconds);
        break;
      case 'S': o.save_read_file = true; break;
      case 1000: break;                             // --gpu: the only path
      case 1001: break;                             // --gpu-threads: fixed 256-lane workgroups
      case 1002: o.gpu_blocks = (uint32_t)strtoul(optarg, nullptr, 10); break;
      case 1003: o.max_chunks = strtoull(optarg, nullptr, 10); break;
      case 1006: o.use_gate = false; break;         // the reference's exact level-1 candidate stream
      case 'z':                                     // keyhunt.cpp:766-772 (used by initBloomFilter, 6559-6576)
        o.bloom_multiplier = (int)strtol(optarg, nullptr, 10);
        if (o.bloom_multiplier <= 0) o.bloom_multiplier = 1;
        printf("[+] Bloom Size Multiplier %i\n", o.bloom_multiplier);
        break;
      case 'C': case 'E': case 'N': case 'p': case 'v': case 'G': case '8':
        break;   // options of the other search modes
      default:
        fprintf(stderr, "[E] Unknow opcion -%c\n", c);
        exit(EXIT_FAILURE);
    }
  }
}

CliRange resolve_range(const CliOptions& o) {
  CliRange r;
  if (!o.flag_range) return r;
  U256::from_hex(o.range_start.c_str(), r.start);
  if (r.start.is_zero()) r.start = U256(1);
  U256::from_hex(o.range_end.c_str(), r.end);
  if (r.start == r.end) {
    fprintf(stderr, "[E] Start and End range can't be the same\nFallback to random mode!\n");
  } else if (r.start < secp_order() && r.end <= secp_order()) {
    if (r.start > r.end) {
      fprintf(stderr, "[W] Opps, start range can't be great than end range. Swapping them\n");
      std::swap(r.start, r.end);
    }
    r.have = true;
  } else {
    fprintf(stderr, "[E] Start and End range can't be great than N\nFallback to random mode!\n");
  }
  return r;
}

std::string speed_line(const U256& total, uint64_t seconds) {
  U256 per = total, q;
  U256::divmod(total, U256(seconds ? seconds : 1), &per, nullptr);
  U256 lim[7];
  const char* ls[7] = {"1000000", "1000000000", "1000000000000", "1000000000000000", "1000000000000000000",
                       "1000000000000000000000", "1000000000000000000000000"};
  for (int j = 0; j < 7; ++j) U256::from_dec(ls[j], lim[j]);
  char buf[512];
  if (per < lim[0]) {
    snprintf(buf, sizeof buf, "[+] Total %s keys in %llu seconds: %s keys/s", total.dec().c_str(),
             (unsigned long long)seconds, per.dec().c_str());
  } else {
    int i = 0;
    bool salir = false;
    while (i < 6 && !salir) {
      if (per < lim[i + 1]) salir = true; else i++;
    }
    const int idx = salir ? i : i - 1;
    U256::divmod(per, lim[idx], &q, nullptr);
    snprintf(buf, sizeof buf, "[+] Total %s keys in %llu seconds: ~%s %s (%s keys/s)", total.dec().c_str(),
             (unsigned long long)seconds, q.dec().c_str(), kLimitPrefix[idx], per.dec().c_str());
  }
  return buf;
}

StatsTicker::StatsTicker(uint64_t every, bool matrix, std::mutex& mu, std::function<std::string(uint64_t)> line) {
  th_ = std::thread([this, every, matrix, &mu, line] {
    const auto t0 = std::chrono::steady_clock::now();
    uint64_t seconds = 0;
    while (!done_.load()) {
      std::this_thread::sleep_for(std::chrono::milliseconds(100));
      const uint64_t el = (uint64_t)std::chrono::duration_cast<std::chrono::seconds>(
                              std::chrono::steady_clock::now() - t0).count();
      if (el <= seconds) continue;
      seconds = el;
      if (every == 0 || seconds % every) continue;
      std::lock_guard<std::mutex> lk(mu);
      if (matrix) printf("%s\n", line(seconds).c_str());
      else { printf("\r%s\r", line(seconds).c_str()); fflush(stdout); }
    }
  });
}

void StatsTicker::stop() {
  done_ = true;
  if (th_.joinable()) th_.join();
}

void append_found(std::mutex& mu, const std::string& file_text, const std::string& stdout_text) {
  std::lock_guard<std::mutex> lk(mu);
  FILE* keys = fopen("KEYFOUNDKEYFOUND.txt", "a");
  if (keys) {
    fputs(file_text.c_str(), keys);
    fclose(keys);
  }
  fputs(stdout_text.c_str(), stdout);
  fflush(stdout);
}

void print_table_sizes(const Geometry& geo) {
  const uint64_t items[3] = {geo.items1, geo.items2, geo.items3}, elements[3] = {geo.m, geo.m2, geo.m3};
  for (int i = 0; i < 3; ++i) {
    BloomFilter b;
    b.init2(items[i], 0.000001, false);
    printf("[+] Bloom filter for %llu elements : %.2f MB\n", (unsigned long long)elements[i],
           (float)(b.bytes * 256) / 1048576.0f);
  }
  printf("[+] Allocating %.2f MB for %llu bP Points\n", (double)(geo.m3 * 16 / 1048576), (unsigned long long)geo.m3);
}

void print_resident_lines(const Session& s) {
  const std::vector<Session::ResidentInfo>& v = s.resident_info();
  for (size_t i = 0; i < v.size(); ++i) {
    const double mb = 1.0 / 1048576.0;
    char gate[96] = "no gate";
    if (v[i].gate_log2)
      snprintf(gate, sizeof gate, "gate 2^%u bits (%.2f MB, %u probes)", v[i].gate_log2,
               (double)(1ull << (v[i].gate_log2 - 3)) * mb, v[i].gate_probes);
    printf("[+] GPU %d resident: L1 bloom %.2f MB, %s, build %.1f ms\n", s.config().devices[i],
           (double)v[i].l1_bytes * mb, gate, v[i].build_ms);
  }
  fflush(stdout);
}

}  // namespace khb
