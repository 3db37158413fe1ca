// The front end shared by keyhunt_amd and bsgsd_amd (cli.cpp): the options struct and its parser, the -r rule, and
// the pieces of output both programs or several modes print (stats line, found file, table sizes, resident lines).
// keyhunt_main.cpp: mode table, main() and -m bsgs; keyhunt_address.cpp: -m address / -m rmd160 / -m xpoint;
// bsgsd_main.cpp: the daemon.  cli.cpp links against u256 and secp_host only.
#pragma once
#include <stdint.h>

#include <atomic>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "u256.hpp"

namespace khb {

struct Geometry;
class Session;

// -m values the front end tests by name, numbered as the reference's MODE_* (keyhunt.cpp:51-57)
enum : int { kModeXpoint = 0, kModeAddress = 1, kModeBsgs = 2, kModeRmd160 = 3 };
enum : int { kBsgsBoth = 2, kBsgsRandom = 3 };   // -B values (keyhunt.cpp:227)
extern const char* const kBsgsModes[5];

int default_threads();                // the hardware's threads, 16 at the most

// Every flag of keyhunt_amd; bsgsd_amd fills the ones it shares (-6 -k -n -t -g --check --cpu-build --resident).
struct CliOptions {
  int mode = kModeBsgs;               // -m: row of the mode table
  int bsgs_mode = 0;                  // -B (index into kBsgsModes); -R selects random
  int kfactor = 1;                    // -k
  int threads = default_threads();    // -t
  bool quiet = false, matrix = false; // -q, -M
  bool flag_range = false;            // -r accepted by the parser (resolve_range applies the rule)
  std::string range_start, range_end; // as typed
  bool flag_bits = false;             // -b
  int bitrange = 0;
  std::string bits_min, bits_max;
  const char* file = nullptr;         // -f
  const char* str_n = nullptr;        // -n
  const char* stride = nullptr;       // -I
  uint64_t out_seconds = 30;          // -s
  std::vector<int> devices{0};        // -g
  uint32_t gpu_blocks = 0;            // --gpu-blocks
  uint64_t max_chunks = 0;            // --max-chunks
  int check_mode = 0;                 // --check (engine.hpp kCheck*)
  bool use_gate = true;               // --no-gate clears it
  bool save_read_file = false, skip_checksum = false, cpu_build = false, resident = false;   // -S -6 --cpu-build --resident
  bool endomorphism = false;          // -e (keyhunt.cpp:579-585)
  bool crypto_set = false;            // -c given
  bool eth = false;                   // -c eth: ETH addresses (-l is then not used for hashing)
  int search = 2;                     // -l (keyhunt.cpp:300: both); accepted and not used by -m xpoint
  int bloom_multiplier = 1;           // -z
};

// One row per -m value, in the reference's order (keyhunt.cpp:228); run == nullptr: not available.  The table and
// the usage text are keyhunt_amd's (keyhunt_main.cpp); the parser gets them as a CliProgram, so that cli.cpp links
// without any mode's code.
struct CliMode {
  const char* name;
  int (*run)(const CliOptions&);
};
struct CliProgram {
  const CliMode* modes;
  int mode_count;
  void (*menu)();                     // -h: prints the usage and exits
};

int run_address_mode(const CliOptions& o);

// keyhunt_amd's getopt_long loop (keyhunt.cpp:489-779): fills o and prints the [+] / [W] / [E] lines in option order.
// Exits on -h, an unknown option, an unknown -m and a bad --check.
void parse_keyhunt_args(int argc, char** argv, CliOptions& o, const CliProgram& prog);
// The options keyhunt_amd and bsgsd_amd share (-k -t -6 -g and the long options below): false if c is none of them.
enum : int { kOptCpuBuild = 1004, kOptCheck = 1005, kOptResident = 1007 };
bool parse_shared_option(int c, const char* arg, CliOptions& o);
// --resident with -S or --cpu-build: prints the [E] line and exits.
void check_resident_conflict(const CliOptions& o);
std::vector<int> parse_devices(const char* arg);     // -g: ids separated by commas (or " \t:"); none: device 0
int parse_check_mode(const char* s);                 // --check: "host", "gpu" or "auto" (kCheck*); -1 else

void trim(char* s);                                  // trim(aux," \t\n\r") (util.c)
std::vector<std::string> tokens(const char* s);      // stringtokenizer (util.c:67-84): trim "\t\n\r :", split on " \t:"
bool valid_hex(const char* s);                       // isValidHex (util.c:169-178)

// The -r rule (keyhunt.cpp:816-838): 0 becomes 1, start and end swapped when reversed; equal bounds or a bound past
// the group order give no range (the callers fall back to -b or their default).  Prints the [W] / [E] lines.
struct CliRange {
  bool have = false;
  U256 start, end;
};
CliRange resolve_range(const CliOptions& o);

// "[+] Total %s keys in %s seconds: ..." (keyhunt.cpp:2194-2238)
std::string speed_line(const U256& total, uint64_t seconds);

// The stats thread (keyhunt.cpp:2154-2252): wakes every 100 ms, acts once per whole second and every `every` seconds
// (0: never) prints line(seconds) under mu, as "\r...\r" or, with -M, as a line of its own.
class StatsTicker {
 public:
  StatsTicker(uint64_t every, bool matrix, std::mutex& mu, std::function<std::string(uint64_t seconds)> line);
  ~StatsTicker() { stop(); }
  void stop();   // joins the thread; nothing is printed after it returns

 private:
  std::atomic<bool> done_{false};
  std::thread th_;
};

// A found key: file_text appended to KEYFOUNDKEYFOUND.txt and stdout_text printed, under mu.
void append_found(std::mutex& mu, const std::string& file_text, const std::string& stdout_text);
// The three "[+] Bloom filter for ..." lines and "[+] Allocating ... bP Points" (keyhunt.cpp:1214-1303)
void print_table_sizes(const Geometry& geo);
// --resident: one "[+] GPU <d> resident: L1 ..., gate ..., build ..." line per device of an open session (nothing
// on other tables).
void print_resident_lines(const Session& s);

}  // namespace khb
