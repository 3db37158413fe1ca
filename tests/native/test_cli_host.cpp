// host/cli.cpp on the CPU: parse_keyhunt_args on argv vectors, resolve_range, parse_devices, tokens and valid_hex.
// Built from cli.cpp, u256.cpp and secp_host.cpp alone.  The expected values are those of keyhunt_amd's main() before
// the parser was split out of it (and keyhunt.cpp's, which that followed): they are written down here, not computed.
#include <stdio.h>
#include <stdlib.h>

#include <deque>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../keyhuntm1cpu_amd/csrc/host/cli.hpp"
#include "../../keyhuntm1cpu_amd/csrc/host/engine.hpp"   // kCheck*

using namespace khb;

static int failures = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      fprintf(stderr, "FAIL line %d: %s\n", __LINE__, #c);         \
      failures++;                                                  \
    }                                                              \
  } while (0)

static const char* kOrder = "fffffffffffffffffffffffffffffffebaaedce6af48a03bbfd25e8cd0364141";
static const CliMode kModes[] = {{"xpoint", nullptr}, {"address", nullptr}, {"bsgs", nullptr}, {"rmd160", nullptr},
                                 {"pub2rmd", nullptr}, {"minikeys", nullptr}, {"vanity", nullptr}};
static void no_menu() {}

static CliOptions parse(std::initializer_list<const char*> args) {
  static std::deque<std::vector<std::string>> kept;   // -f, -n and -I keep pointers into argv
  kept.emplace_back(1, "keyhunt_amd");
  std::vector<std::string>& keep = kept.back();
  for (const char* a : args) keep.push_back(a);
  std::vector<char*> argv;
  for (std::string& s : keep) argv.push_back(&s[0]);
  argv.push_back(nullptr);
  CliOptions o;
  parse_keyhunt_args((int)keep.size(), argv.data(), o, {kModes, 7, no_menu});
  return o;
}

static std::string hex_of(const U256& v) { return v.hex(); }
typedef std::vector<std::string> Strs;
typedef std::vector<int> Ints;

int main() {
  {   // defaults
    const CliOptions o = parse({});
    CHECK(o.mode == kModeBsgs && o.bsgs_mode == 0 && o.kfactor == 1 && o.threads >= 1 && o.threads <= 16);
    CHECK(!o.flag_range && !o.flag_bits && o.out_seconds == 30 && o.devices == Ints{0} && o.search == 2);
    CHECK(!o.eth && !o.crypto_set && o.check_mode == kCheckHost && o.use_gate && o.bloom_multiplier == 1);
    CHECK(!resolve_range(o).have);
  }
  // -b: [2^(b-1), 2^b], the upper bound capped at the group order; 0 and 300 are refused and leave no bit range
  {
    CliOptions o = parse({"-b", "0"});
    CHECK(!o.flag_bits && o.bitrange == 0 && o.bits_min.empty());
    o = parse({"-b", "1"});
    CHECK(o.flag_bits && o.bitrange == 1 && o.bits_min == "1" && o.bits_max == "2");
    o = parse({"-b", "66"});
    CHECK(o.flag_bits && o.bitrange == 66 && o.bits_min == "20000000000000000" && o.bits_max == "40000000000000000");
    o = parse({"-b", "256"});
    CHECK(o.flag_bits && o.bitrange == 256 && o.bits_max == kOrder);
    CHECK(o.bits_min == "8000000000000000000000000000000000000000000000000000000000000000");
    o = parse({"-b", "300"});
    CHECK(!o.flag_bits && o.bitrange == 300 && o.bits_min.empty() && o.bits_max.empty());
  }
  // -r
  {
    CliOptions o = parse({"-r", "10"});                        // one token: up to the order
    CHECK(o.flag_range && o.range_start == "10" && o.range_end == kOrder);
    CliRange r = resolve_range(o);
    CHECK(r.have && hex_of(r.start) == "10" && hex_of(r.end) == kOrder);
    o = parse({"-r", "10:20"});                                // two tokens
    r = resolve_range(o);
    CHECK(o.flag_range && o.range_start == "10" && o.range_end == "20" && r.have && hex_of(r.start) == "10" &&
          hex_of(r.end) == "20");
    CHECK(!parse({"-r", "1:2:3"}).flag_range);                 // three tokens
    CHECK(!parse({"-r", "zz:20"}).flag_range);                 // no hex, first and second position
    CHECK(!parse({"-r", "10:zz"}).flag_range);
    CHECK(!parse({"-r", "zz"}).flag_range);
    o = parse({"-r", "5:5"});                                  // start equal to end: parsed, then no range
    CHECK(o.flag_range && !resolve_range(o).have);
    o = parse({"-r", "20:10"});                                // start greater than end: swapped
    r = resolve_range(o);
    CHECK(r.have && hex_of(r.start) == "10" && hex_of(r.end) == "20" && o.range_start == "20" && o.range_end == "10");
    o = parse({"-r", "1:fffffffffffffffffffffffffffffffebaaedce6af48a03bbfd25e8cd0364142"});   // end above the order
    CHECK(o.flag_range && !resolve_range(o).have);
    o = parse({"-r", (std::string("1:") + kOrder).c_str()});  // end equal to the order is in
    CHECK(resolve_range(o).have);
    o = parse({"-r", "0:20"});                                 // start 0 becomes 1
    r = resolve_range(o);
    CHECK(r.have && hex_of(r.start) == "1" && hex_of(r.end) == "20" && o.range_start == "0");
    o = parse({"-r", "0:1"});                                  // ... and then equals the end
    CHECK(o.flag_range && !resolve_range(o).have);
  }
  // -g
  CHECK(parse({"-g", "0"}).devices == Ints{0});
  CHECK((parse({"-g", "0,1,2"}).devices == Ints{0, 1, 2}));
  CHECK(parse({"-g", ",,3,"}).devices == Ints{3});
  CHECK(parse({"-g", ""}).devices == Ints{0});
  CHECK((parse({"-g", "0:1"}).devices == Ints{0, 1}));
  CHECK((parse_devices("2, 5") == Ints{2, 5}));
  // -k, -t
  CHECK(parse({"-k", "0"}).kfactor == 1 && parse({"-k", "8"}).kfactor == 8);
  CHECK(parse({"-t", "0"}).threads == 1 && parse({"-t", "5"}).threads == 5);
  // -l
  CHECK(parse({"-l", "uncompress"}).search == 0 && parse({"-l", "compress"}).search == 1);
  CHECK(parse({"-l", "both"}).search == 2 && parse({"-l", "nothing"}).search == 2);
  CHECK(parse({"-l", "compress", "-l", "nothing"}).search == 1);
  // -c
  {
    CliOptions o = parse({"-c", "btc"});
    CHECK(o.crypto_set && !o.eth);
    o = parse({"-c", "eth"});
    CHECK(o.crypto_set && o.eth);
    o = parse({"-c", "doge"});
    CHECK(!o.crypto_set && !o.eth);
  }
  // -B, -R
  {
    const char* names[5] = {"sequential", "backward", "both", "random", "dance"};
    for (int i = 0; i < 5; ++i) CHECK(parse({"-B", names[i]}).bsgs_mode == i);
    CHECK(parse({"-B", "sideways"}).bsgs_mode == 0);
    CHECK(parse({"-B", "dance", "-B", "sideways"}).bsgs_mode == 4);
    CHECK(parse({"-R"}).bsgs_mode == 3 && kBsgsRandom == 3 && kBsgsBoth == 2);
  }
  // --check
  CHECK(parse({"--check", "host"}).check_mode == kCheckHost && kCheckHost == 0);
  CHECK(parse({"--check", "gpu"}).check_mode == kCheckDevice && kCheckDevice == 1);
  CHECK(parse({"--check", "auto"}).check_mode == kCheckAuto && kCheckAuto == 2);
  CHECK(parse_check_mode("cpu") == -1);
  // the rest of the flags, and -m by the table's rows
  {
    const CliOptions o = parse({"-m", "rmd160", "-f", "a.txt", "-n", "0x400", "-I", "7", "-s", "0", "-q", "-M", "-e", "-S",
                                "-6", "-z", "0", "--cpu-build", "--resident", "--no-gate", "--gpu-blocks", "3",
                                "--max-chunks", "9", "--gpu"});
    CHECK(o.mode == kModeRmd160 && std::string(o.file) == "a.txt" && std::string(o.str_n) == "0x400");
    CHECK(std::string(o.stride) == "7" && o.out_seconds == 0 && o.quiet && o.matrix && o.endomorphism);
    CHECK(o.save_read_file && o.skip_checksum && o.bloom_multiplier == 1 && o.cpu_build && o.resident && !o.use_gate);
    CHECK(o.gpu_blocks == 3 && o.max_chunks == 9);
    CHECK(parse({"-m", "xpoint"}).mode == kModeXpoint && parse({"-m", "address"}).mode == kModeAddress);
    CHECK(parse({"-m", "vanity"}).mode == 6);
  }
  // tokens: the reference's stringtokenizer
  CHECK((tokens(" a:b\t c \r\n") == Strs{"a", "b", "c"}));
  CHECK(tokens(":::").empty());
  CHECK(tokens("").empty());
  CHECK((tokens("02ab # puzzle 1") == Strs{"02ab", "#", "puzzle", "1"}));
  // valid_hex: isValidHex, whose loop accepts the empty string (no token is ever empty)
  CHECK(valid_hex(""));
  CHECK(valid_hex("0aF"));
  CHECK(!valid_hex("0x1"));
  if (failures) return 1;
  printf("ok\n");
  return 0;
}
