/*
 * khhost.h — C ABI of the host half of the engine, libkhhost.so: keyhunt's BSGS setup and
 * confirmation (keyhunt.cpp:962-1880, 4271-4368) plus the multi-GPU search driver that calls
 * libkhbsgs.so.  The keyhunt_amd CLI is built from the same sources; this ABI exists so tests and
 * bench.py can drive exactly the code the CLI runs.
 *
 * Points and 256-bit values cross as big-endian bytes (x||y for points), like include/khbsgs.h.
 * Functions return 0 on success or a negative KHB_E* code (include/khbsgs.h).
 */
#ifndef KHHOST_H
#define KHHOST_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version of this header; bumped whenever a signature, a struct or an output array changes.
 * A binding checks khh_abi_version() == the KHH_ABI_VERSION it was written for before any other call.
 * ABI 7 added resident tables (large -k): khh_tables_new_resident and the khh_session_resident_* calls.
 * ABI 8 added -m address -c eth: khh_addr_new_eth, khh_addr_skipped, khh_eth_address, search = KHB_SEARCH_ETH and
 * khh_addr_confirm's kind KHB_ADDR_KIND_ETH.
 * ABI 9 added -m xpoint: khh_addr_new_xpoint, khh_addr_counted, search = KHB_SEARCH_XPOINT (optionally with
 * KHB_SEARCH_ENDOMORPHISM) and khh_addr_confirm's kinds KHB_ADDR_KIND_X | e << 2.
 * ABI 10 added -m vanity: khh_addr_new_vanity, khh_addr_vanity_intervals, khh_addr_vanity_match and
 * khh_vanity_target_ok.
 * ABI 11 added -m minikeys: khh_mini_new / khh_mini_free, khh_mini_search, khh_mini_string, khh_mini_valid,
 * khh_mini_key, khh_mini_table and khh_mini_set_queue_capacity / khh_mini_set_hit_capacity.
 * ABI 12 added the kangaroo interval search: the khh_kang_* calls. */
#define KHH_ABI_VERSION 12
int khh_abi_version(void);

typedef struct khh_tables khh_tables;

/* Geometry + all tables.  n_str: -n value ("0x.." or decimal) or NULL (2^44); k: -k factor;
 * threads: builder threads; gpl: GPU groups per lane (lane-offset table).  NULL on error (err). */
khh_tables* khh_tables_new(const char* n_str, int k, int threads, uint32_t gpl, char* err, size_t errlen);
void khh_tables_free(khh_tables* t);
/* Like khh_tables_new, with -S semantics (keyhunt.cpp:1373-1613, 1881-2025): the reference's table
 * files keyhunt_bsgs_{4,6,2,7}_*.{blm,tbl} are read from dir when present (checksums verified
 * unless skip_checksum), only the missing tables are computed, and with save != 0 the missing ones
 * are written back.  *have receives the mask of files read (1 L1, 2 L2, 4 bPtable, 8 L3). */
khh_tables* khh_tables_new_files(const char* n_str, int k, int threads, uint32_t gpl, const char* dir,
                                 int skip_checksum, int save, uint32_t* have, char* err, size_t errlen);
/* Like khh_tables_new with the baby-step walk on GPU `device` (khb_build_baby); identical tables.
 * *kernel_ms (nullable) receives the build kernel's time. */
khh_tables* khh_tables_new_gpu(const char* n_str, int k, int threads, uint32_t gpl, int device, double* kernel_ms,
                               char* err, size_t errlen);
/* Resident tables for large -k: L2, L3, the bPtable, the giant tables and the lane offsets as khh_tables_new_gpu
 * builds them (the walk covers only the first m2 baby steps), the level-1 geometry, and the level-1 build's inputs
 * (64 B per 2^20 baby steps).  No level-1 bloom and no gate exist on the host: khh_session_open builds both on
 * every device (khb_build_l1_resident) and they stay there.  gate_log2: 0 = sized per device from its free memory
 * (64 bits per level-1 x, at most 2^38, halved until it fits; none below 4 bits per x), otherwise an explicit size
 * in [13, 38] for tests and measurements.  On such tables khh_bloom(level 1) and khh_gate return NULL and
 * khh_tables_save fails; everything else, khh_search included, works. */
khh_tables* khh_tables_new_resident(const char* n_str, int k, int threads, uint32_t gpl, int device,
                                    uint32_t gate_log2, double* kernel_ms, char* err, size_t errlen);
int khh_tables_is_resident(const khh_tables* t);
/* The gate stages later sessions build on resident tables (khb_set_gate_stage1 / khb_set_gate_stage0 values; the
 * defaults are KHB_GATE_STAGE1_AUTO and 0). */
int khh_tables_set_resident_stages(khh_tables* t, uint32_t stage1_log2, uint32_t stage0_log2);
/* The gate policy of resident builds: log2 bits for l1ext level-1 entries and budget_bytes of device memory. */
uint32_t khh_resident_gate_log2(uint64_t l1ext, uint64_t budget_bytes);
/* 1 when a resident build with the AUTO stage-1 setting keeps the fold in front of a gate of 2^gate_log2 bits for
 * l1ext level-1 entries (at most 32 entries per 64-bit fold block: beyond that the fold passes most x), else 0. */
int khh_resident_keeps_fold(uint64_t l1ext, uint32_t gate_log2);
/* Write all four table files into dir. */
int khh_tables_save(const khh_tables* t, const char* dir, char* err, size_t errlen);
/* out: [0]=m [1]=m2 [2]=m3 [3]=aux [4]=cycles [5]=N(low64) [6]=l1 extent [7..9]=bloom entries L1..L3 */
void khh_params(const khh_tables* t, uint64_t out[10]);
/* level 1..3, sub-bloom idx 0..255: pointer to the bit array; geometry through the out params */
const uint8_t* khh_bloom(const khh_tables* t, int level, int idx, uint64_t* bytes, uint64_t* bits, uint32_t* hashes);
void khh_giant_table(const khh_tables* t, uint8_t out[513 * 64]);
void khh_amp_table(const khh_tables* t, int level, uint8_t out[32 * 64]);
uint32_t khh_lane_offsets(const khh_tables* t, uint8_t* out /* n*64, may be NULL */, uint32_t* gpl);
/* Level-0 gate (khb_load_gate): pointer to 2^log2 / 8 bytes, or NULL with *log2 = 0 when none */
const uint8_t* khh_gate(const khh_tables* t, uint32_t* log2);
/* Gate probes (bits per x, khb_load_gate's probes); 0 when the tables have no gate */
uint32_t khh_gate_probes(const khh_tables* t);
/* bPtable (sorted): m3 records of {6-byte value, 2 pad, u64 index} */
const uint8_t* khh_bptable(const khh_tables* t, uint64_t* n);

/* startP of (chunk base, target): keyhunt.cpp:3861-3869 */
int khh_chunk_centre(const khh_tables* t, const uint8_t base_be[32], const uint8_t target_xy[64], uint8_t out_xy[64]);
/* The search engine's batched centres (engine.cpp job_centres) of n_chunks x n_targets jobs:
 * out[64 * (c * n_targets + j)] = centre of chunk bases[c] for target j (what khh_chunk_centre gives
 * one at a time); consecutive bases (2N apart) take the batched auxiliary walk. */
int khh_job_centres(const khh_tables* t, const uint8_t* bases_be, uint32_t n_chunks, const uint8_t* targets_xy,
                    uint32_t n_targets, uint8_t* out_xy, int threads);
/* bsgs_secondcheck: 1 found (key_be filled), 0 not found */
int khh_secondcheck(const khh_tables* t, const uint8_t base_be[32], uint32_t a, const uint8_t target_xy[64],
                    uint8_t key_be[32]);

/* Multi-GPU search over [start, end): found[k] (0/1) and keys[k] (32 B BE) per target.
 * devices: n_devices device ordinals.  stats_out (nullable): [0]=chunks [1]=giant steps
 * [2]=candidates [3]=degenerate groups [4]=kernel microseconds [5]=scan launches (stats_out holds 6). */
int khh_search(const khh_tables* t, const uint8_t* targets_xy, int n_targets, const uint8_t start_be[32],
               const uint8_t end_be[32], const int* devices, int n_devices, uint32_t lanes,
               uint32_t chunks_per_batch, uint64_t max_chunks, int* found, uint8_t* keys_be, uint64_t* stats_out,
               char* err, size_t errlen);

/* Persistent multi-GPU session: contexts opened and tables resident in HBM once, then any number
 * of searches.  khh_session_run writes the 6 stats entries of khh_search (stats_out holds 6).
 * khh_session_run_ex writes the first min(stats_len, KHH_SESSION_STATS) of: those 6, [6]=launches
 * rescanned in parts after a candidate-ring overflow, [7]=device-busy microseconds (union of each
 * device's launch intervals, summed over devices; two launches in flight overlap, so [7] <= [4]),
 * [8]=average shader clock of the launches in kHz, [9]=candidates confirmed on the GPU (khb_check),
 * [10]=microseconds spent in those khb_check calls, [11]=the launches' summed HIP-event microseconds
 * (khb_stats.event_ms: dispatch to end, what rocprofv3's kernel trace reports; [4] sums their execution
 * spans, khb_stats.kernel_ms). */
#define KHH_SESSION_STATS 12
typedef struct khh_session khh_session;
khh_session* khh_session_open(const khh_tables* t, const int* devices, int n_devices, uint32_t lanes,
                              uint32_t chunks_per_batch, int check_threads, char* err, size_t errlen);
int khh_session_run(khh_session* s, const uint8_t* targets_xy, int n_targets, const uint8_t start_be[32],
                    const uint8_t end_be[32], uint64_t max_chunks, int random_chunks, int* found, uint8_t* keys_be,
                    uint64_t* stats_out, char* err, size_t errlen);
int khh_session_run_ex(khh_session* s, const uint8_t* targets_xy, int n_targets, const uint8_t start_be[32],
                       const uint8_t end_be[32], uint64_t max_chunks, int random_chunks, int* found, uint8_t* keys_be,
                       uint64_t* stats_out, uint32_t stats_len, char* err, size_t errlen);
void khh_session_close(khh_session* s);
/* A session on resident tables: what each device built, KHH_RESIDENT_INFO values per device in device order:
 * [0]=L1 bytes [1]=gate log2 bits (0 = none) [2]=gate probes [3]=stage-1 fold log2 bytes (0 = none)
 * [4]=stage-0 filter log2 bytes (0 = none) [5]=build kernel microseconds [6]=free and [7]=total device memory
 * after the build.  Writes up to cap_devices entries; returns the device count (0 on other tables). */
#define KHH_RESIDENT_INFO 8
int khh_session_resident_info(const khh_session* s, uint64_t* out, uint32_t cap_devices);
/* Pass-throughs to the context of the session's device number `index` (any tables): khb_resident_bytes,
 * khb_resident_read, khb_resident_popcount and khb_gate_probe (include/khbsgs.h, KHB_TABLE_*). */
int khh_session_resident_bytes(khh_session* s, uint32_t index, int which, uint64_t* bytes);
int khh_session_resident_read(khh_session* s, uint32_t index, int which, uint64_t offset, uint64_t bytes,
                              uint8_t* out);
int khh_session_resident_popcount(khh_session* s, uint32_t index, int which, uint64_t* bits_set);
int khh_session_gate_probe(khh_session* s, uint32_t index, const uint8_t* xs, uint8_t* out, uint32_t n);
/* Test hooks: candidate ring capacity per launch (0 = default 2^20; small values drive the
 * split-and-rescan path), the level-0 gate on/off, recording of every level-1 candidate of the next
 * runs (khh_session_recorded), and optionally a replacement level-1 bloom of the tables' geometry
 * (256 sub-blooms concatenated; NULL keeps the tables'). */
int khh_session_set_test_hooks(khh_session* s, uint32_t cand_cap, int use_gate, int record, const uint8_t* l1_concat);
/* Where later runs confirm their level-1 candidates (bsgs_secondcheck/thirdcheck, keyhunt.cpp:4271-4368):
 * 0 = the host's CPU pool (default), 1 = the GPU that scanned them (khb_check; the check tables are
 * loaded into every context), 2 = the GPU for batches of more than 4096 candidates, else the host. */
#define KHH_CHECK_HOST 0
#define KHH_CHECK_DEVICE 1
#define KHH_CHECK_AUTO 2
int khh_session_set_check_mode(khh_session* s, int mode);
/* keyhunt's -B mode for later runs (keyhunt.cpp:227): 0 sequential, 1 backward, 2 both, 3 random, 4 dance
 * (the thread_process_bsgs* variants, 3778-5700; engine.hpp ChunkCursor).  A run's random_chunks != 0
 * still selects random. */
int khh_session_set_chunk_mode(khh_session* s, int mode);
/* The chunk bases a -B mode claims from [start, end) with chunks of two_n keys, in claim order, up to cap
 * (out: 32 B BE each); the seed drives both / dance.  Returns the count (the whole sequence unless cap is
 * reached or the mode is random).  Host only: the claim order the search uses. */
uint64_t khh_chunk_sequence(int mode, const uint8_t start_be[32], const uint8_t end_be[32], const uint8_t two_n_be[32],
                            uint64_t seed, uint8_t* out_be, uint64_t cap);
/* Secp256K1::Init's GTable (secp256k1/SECP256K1.cpp:43-54), 32*256 points x||y BE (khb_check_tables.gtable). */
void khh_gtable(uint8_t out[32 * 256 * 64]);
/* Candidates recorded in the last run: chunk base (32 B BE), target index, giant step a; returns the
 * count (may exceed cap). */
uint64_t khh_session_recorded(const khh_session* s, uint8_t* bases_be, uint32_t* targets, uint32_t* a, uint64_t cap);

/* helpers */
int khh_pubkey(const uint8_t key_be[32], uint8_t out_xy[64]);
int khh_parse_pubkey(const char* hex, uint8_t out_xy[64], int* compressed);

/* ---- -m address / -m rmd160 (BTC P2PKH, and ETH addresses with -c eth) and -m xpoint ----
 * Targets from a target file's text (base58 addresses or 40-hex rmd160 lines, keyhunt.cpp:6300-6358).
 * The generator (Gn table + lane offsets for chunks of n_seq keys) is built for stride and gpl. */
typedef struct khh_addr khh_addr;
khh_addr* khh_addr_new(const char* text, int bloom_multiplier, const uint8_t stride_be[32], uint64_t n_seq,
                       uint32_t gpl, int threads, char* err, size_t errlen);
/* -c eth: targets as forceReadFileAddressEth reads them (keyhunt.cpp:6374-6450).  Lines are trimmed of " \t\n\r";
 * lines of 40 or more characters size the bloom; a 40-character line must be hex, a 42-character line hex from
 * its third character (the two leading characters are not looked at), either letter case; every other counted
 * line is skipped.  Such a handle is searched with KHB_SEARCH_ETH only, and a khh_addr_new handle never with it:
 * the mismatch is an error return with a message, not an empty search. */
khh_addr* khh_addr_new_eth(const char* text, int bloom_multiplier, const uint8_t stride_be[32], uint64_t n_seq,
                           uint32_t gpl, int threads, char* err, size_t errlen);
/* -m xpoint: targets as forceReadFileXPoint reads them (keyhunt.cpp:6454-6552).  Lines are trimmed of " \t\n\r";
 * lines of 40 or more characters are counted, the count sizes the bloom (initBloomFilter and the multiplier) and is
 * also the number of lines read from the top of the text, as in the reference.  The first token of a line
 * (separators: space, tab, ':') decides: 64 hex characters are x; 66 are a compressed key whose two prefix
 * characters are dropped without being checked; 130 are an uncompressed key.  A token of any other length or with a
 * non-hex character is skipped (khh_addr_skipped) and not stored in the table.  The table holds the first 20 bytes
 * of x, sorted by memcmp, and the bloom the same 20 bytes.
 * One deliberate deviation: for a 130-character line the reference adds 04 || x[0..18] to the bloom and stores
 * x[1..20] in the table (keyhunt.cpp:6524-6528, offsets 0 and 2 where 1 was meant), so an uncompressed line can
 * never be found there; here both take x[0..19].
 * Such a handle is searched with KHB_SEARCH_XPOINT (16), alone or OR'ed with KHB_SEARCH_ENDOMORPHISM, only, and no
 * other handle ever with it: the mismatch is an error return with a message, as for -c eth. */
khh_addr* khh_addr_new_xpoint(const char* text, int bloom_multiplier, const uint8_t stride_be[32], uint64_t n_seq,
                              uint32_t gpl, int threads, char* err, size_t errlen);
/* -m vanity: text holds one address prefix per line (trimmed of " \t\n\r"; blank lines are passed over).  A target
 * is accepted iff it is valid Base58, 1 to 29 characters long, begins with '1' and yields at least one interval; every
 * other line is skipped (khh_addr_skipped).  A hash160 matches a target iff its P2PKH address begins with it.  Each
 * target becomes, per address length, the range from the target padded with '1' to the target padded with 'z', cut to
 * the 25-byte values with the target's number of leading zero bytes (a target of '1' characters alone: at least that
 * many) and shifted right by 32 bits to drop the checksum; the ranges of all targets are merged into sorted, disjoint
 * intervals (touching ones joined), the table khb_load_vanity takes.  The device reports every hash inside them and
 * khh_addr_confirm / the search keep a hit only if the recovered key's address begins with a target, so the found
 * set is exact.
 * Deliberate deviations from the reference: its addvanity (keyhunt.cpp:5837-5958) pairs the j-th '1'-padded bound
 * with the j-th 'z'-padded bound of two lists that can differ in length, which loses ranges (for "1Q" the 34-character
 * addresses are never matched); the intervals here are exact.  And it accepts targets that do not begin with '1'
 * ("3abc") and then matches P2PKH hashes whose printed address does not carry the prefix; they are rejected here.
 * Such a handle is searched with search = 0, 1 or 2 (-l), optionally OR'ed with KHB_SEARCH_ENDOMORPHISM; the search
 * adds KHB_SEARCH_VANITY itself.  A handle without an accepted target can be inspected; searching it is KHB_EINVAL
 * (the Python binding does not hand out such a handle: khhost.Addr raises ValueError when the library counted none).
 * It has no bloom and no 20-byte table (khh_addr_table gives n = 0). */
khh_addr* khh_addr_new_vanity(const char* text, const uint8_t stride_be[32], uint64_t n_seq, uint32_t gpl, int threads,
                              char* err, size_t errlen);
/* The merged intervals of a vanity handle: *n entries of lo || hi (20 bytes each, big-endian), ascending. */
const uint8_t* khh_addr_vanity_intervals(const khh_addr* a, uint64_t* n);
/* For n 20-byte hash160 values on a vanity handle: out[i] bit 0 = the value lies in a merged interval (what the device
 * reports), bit 1 = its address begins with an accepted target (what the confirmation keeps). */
int khh_addr_vanity_match(const khh_addr* a, const uint8_t* h20, uint8_t* out, uint64_t n);
/* 1 when s would be accepted as a vanity target, 0 when not ("was NOT Added"). */
int khh_vanity_target_ok(const char* s);
void khh_addr_free(khh_addr* a);
/* lines the loader omitted ("[I] Ommiting invalid line") */
uint64_t khh_addr_skipped(const khh_addr* a);
/* lines the loader counted (they size the bloom) */
uint64_t khh_addr_counted(const khh_addr* a);
/* sorted 20-byte table (n entries) and the target bloom */
const uint8_t* khh_addr_table(const khh_addr* a, uint64_t* n);
const uint8_t* khh_addr_bloom(const khh_addr* a, uint64_t* bytes, uint64_t* bits, uint32_t* hashes);
void khh_addr_giant_table(const khh_addr* a, uint8_t out[513 * 64]);
uint32_t khh_addr_lane_offsets(const khh_addr* a, uint8_t* out /* n*64, may be NULL */, uint32_t* gpl);
/* Sequential (random_chunks = 0) or -R search of [start, end) with search 0/1/2 (-l), OR'ed with
 * KHB_SEARCH_ENDOMORPHISM (4, include/khbsgs.h) for -e: the found keys are then lambda^e multiples too; or with
 * search = KHB_SEARCH_ETH (8) alone on a khh_addr_new_eth handle: found keys come back with compressed = 0 and the
 * 20 address bytes in rmd; or with search = KHB_SEARCH_XPOINT (16), alone or with KHB_SEARCH_ENDOMORPHISM, on a
 * khh_addr_new_xpoint handle: compressed = 0 and the matched first 20 bytes of x in rmd; or with search 0/1/2,
 * optionally with KHB_SEARCH_ENDOMORPHISM, on a khh_addr_new_vanity handle: every key in the range (with -e also its
 * lambda multiples, and n - key as the forms imply) whose address begins with a target; the search goes on after a
 * match, and a launch is sized from the targets' share of all hashes so that its expected hits stay at or below a
 * quarter of the hit ring.  Found keys
 * (32 B BE each) with compressed flags and rmd160s, in discovery order; *n_found may exceed cap.
 * Discovery order is batch order, and (chunk, key) order inside a batch, except after an overflow: a batch
 * whose bloom hits overflowed khb_addr_hit_capacity is rescanned in parts queued behind the batch already
 * submitted after it, so its keys are reported after that later batch's (the bsgs session reorders its
 * candidates the same way).  Callers that need range order sort the keys.
 * stats_out (nullable): [0]=chunks [1]=keys [2]=bloom hits [3]=degenerate groups [4]=kernel us
 * [5]=launches; khh_addr_search writes these 6.  khh_addr_search_ex writes the first
 * min(stats_len, KHH_ADDR_STATS) of them and [6]=average shader clock of the launches in kHz,
 * [7]=rescans (launches whose bloom hits overflowed khb_addr_hit_capacity and were rescanned in parts). */
#define KHH_ADDR_STATS 8
int khh_addr_search(const khh_addr* a, const uint8_t start_be[32], const uint8_t end_be[32], int search,
                    int random_chunks, const int* devices, int n_devices, uint32_t lanes, uint64_t max_chunks,
                    uint8_t* keys_be, uint8_t* compressed, uint8_t* rmd, uint32_t cap, uint32_t* n_found,
                    uint64_t* stats_out, char* err, size_t errlen);
int khh_addr_search_ex(const khh_addr* a, const uint8_t start_be[32], const uint8_t end_be[32], int search,
                       int random_chunks, const int* devices, int n_devices, uint32_t lanes, uint64_t max_chunks,
                       uint8_t* keys_be, uint8_t* compressed, uint8_t* rmd, uint32_t cap, uint32_t* n_found,
                       uint64_t* stats_out, uint32_t stats_len, char* err, size_t errlen);
/* Tests: bloom-hit ring capacity of the search's launches (0 = the library default, 2^18). */
int khh_addr_set_hit_capacity(khh_addr* a, uint32_t cap);
/* The host confirmation of one GPU bloom hit (khb_addr_hit.kind = form | e << 2) of the point with key key_be:
 * searchbinary of the hash the kind names, then the reference's key recovery (keyhunt.cpp:2789-2937; lambda^e * key,
 * negated for the other point of a compressed x or for form 3).  Returns 1 and the key / compressed flag when the
 * hash is a target, 0 when it is not.  kind KHB_ADDR_KIND_ETH (keyhunt.cpp:2989-3002): the ETH address of key*G
 * is looked up and the key returned unchanged.  kind KHB_ADDR_KIND_X | e << 2 (keyhunt.cpp:3005-3062): the first 20
 * bytes of beta^e * x(key*G) are looked up and lambda^e * key mod n returned (the key itself for e = 0), never
 * negated, compressed = 0.  On a vanity handle: the BTC kinds and recovery, and 1 only if the address of the
 * recovered key's hash160 begins with an accepted target. */
int khh_addr_confirm(const khh_addr* a, const uint8_t key_be[32], uint32_t kind, uint8_t out_key_be[32],
                     int* compressed);
/* hash160 of a public key (x||y BE) and its P2PKH address (out_addr >= 36 bytes) */
void khh_hash160(const uint8_t xy[64], int compressed, uint8_t out[20]);
void khh_rmd_to_address(const uint8_t rmd[20], char* out_addr);
/* ETH address of a public key (x||y BE; any 64 bytes): bytes 12..31 of Keccak-256(x||y), keyhunt.cpp:4783-4789 */
void khh_eth_address(const uint8_t xy[64], uint8_t out[20]);

/* ---- -m minikeys (thread_process_minikeys, keyhunt.cpp:2338-2505) ----
 * A minikey is 'S' and 21 characters of a 58-character alphabet; the 21 characters are the digits of a counter in
 * [0, 58^21), the first the most significant.  It is valid iff byte 0 of SHA-256(minikey || '?') is zero; its private
 * key is SHA-256(minikey) read big-endian; it is a find iff the hash160 of that key's uncompressed public key is a
 * target.  A search examines first, first + 1, ..., first + count - 1, each exactly once.  Two deliberate deviations
 * from the reference: its cycles step by 253 N candidates but run until N valid keys were seen, so they overlap or
 * leave gaps at random (keyhunt.cpp:897-917, 2430-2501), and it increments before its first test, so the base it
 * prints is never tested; here a span is exact and `first` is tested.
 *
 * text: the target file's contents, read as -m address reads it (BTC addresses or 40-hex hash160 lines; the same
 * bloom, sorted table and skipped / counted numbers as khh_addr_new).  alphabet: 58 distinct non-zero bytes, or NULL
 * for the reference's Ccoinbuffer_default.  window_bits: 4, 8 or 16, the width of the device's k*G table (0 = the
 * default, 16: DESIGN.md §2f), built here.  NULL with err on a bad argument. */
typedef struct khh_mini khh_mini;
khh_mini* khh_mini_new(const char* text, int bloom_multiplier, const uint8_t* alphabet, uint32_t window_bits,
                       int threads, char* err, size_t errlen);
void khh_mini_free(khh_mini* m);
/* The window table khb_load_mini_table takes (*n_points points of 64 bytes) and its width. */
const uint8_t* khh_mini_table(const khh_mini* m, uint64_t* n_points, uint32_t* window_bits);
/* out22 = the minikey `offset` candidates after first22 (22 characters, no terminator).  KHB_EINVAL for a first22
 * that is no minikey of the handle's alphabet or a sum of 58^21 or more. */
int khh_mini_string(const khh_mini* m, const char* first22, uint64_t offset, char* out22);
/* 1 when the 22 characters pass the typo check, 0 when not, KHB_EINVAL when they are no minikey of the alphabet. */
int khh_mini_valid(const khh_mini* m, const char* minikey22);
/* out32 = SHA-256 of the 22 characters: the private key, big-endian. */
void khh_mini_key(const char* minikey22, uint8_t out32[32]);
/* Tests: survivor-queue and bloom-hit ring capacities of the search's launches (0 = the library's defaults); an
 * overflowed launch is rescanned in halves. */
int khh_mini_set_queue_capacity(khh_mini* m, uint32_t cap);
int khh_mini_set_hit_capacity(khh_mini* m, uint32_t cap);
/* Examine `count` candidates from first22 (first_len must be 22) on the given devices, in launches of per_launch
 * candidates (0 = 2^30; at most 2^32).  Every device hit is confirmed by recomputing minikey -> key -> k*G -> hash160
 * and a lookup in the sorted table.  Finds: minikeys (22 bytes each), keys_be (32), rmd (20), up to cap; *n_found
 * counts them all.  stats_out[0 .. stats_len) of KHH_MINI_STATS values: candidates, valid, bad_keys, hits (device
 * bloom hits), launches, rescans, filter kernel us, key/point/match kernel us.  A bad first22 or
 * first + count > 58^21 is KHB_EINVAL with err, and nothing is launched. */
#define KHH_MINI_STATS 8
/* The CPU baseline of a measurement: the reference's loop (keyhunt.cpp:2430-2498: next candidate, SHA-256 of the 23
 * bytes, and for a valid one SHA-256 of the 22, k*G, hash160 of the uncompressed key, bloom, searchbinary) restated on
 * the host's own functions over the same exact span, `threads` threads each taking a contiguous part.  *valid and
 * *found count what it saw; returns the seconds it took, negative on a bad argument. */
double khh_mini_cpu_scan(const khh_mini* m, const char* first22, uint64_t count, int threads, uint64_t* valid,
                         uint64_t* found);
int khh_mini_search(const khh_mini* m, const char* first22, size_t first_len, uint64_t count, const int* devices,
                    int n_devices, uint32_t lanes, uint64_t per_launch, char* minikeys, uint8_t* keys_be, uint8_t* rmd,
                    uint32_t cap, uint32_t* n_found, uint64_t* stats_out, uint32_t stats_len, char* err,
                    size_t errlen);

/* ---- Pollard's kangaroo interval search for one public key (no reference counterpart) ----
 * The key of pub_xy is sought in [start, end), W = end - start with 2^16 <= W <= 2^200 (NULL with err otherwise, or
 * when end exceeds the group order).  Kangaroo i is tame for even i (its point is d*G) and wild for odd i (Q + d*G,
 * Q = P - start*G); all jump by the 32 jumps (s_j, s_j*G) of the handle, s_j drawn from the seeded generator in
 * [1, 2^(ceil(w/2) + 1)), w the bit length of W, redrawn until the 32 x differ.  The step rule and the distinguished
 * points are include/khbsgs.h's.  A tame and a wild kangaroo on one distinguished x give the key, which is verified
 * (key*G == P) before it is reported; two of one kind have merged, and the later one is replaced and counted.
 * dp_bits < 0 and herd == 0 ask for the defaults: the largest herd (kangaroos per device) and dp_bits with
 * herd * 2^dp_bits <= 2^(floor(w/2) - 2), the herd at most herd_cap (0 = one full residency of the walk kernel times
 * its slots per lane). */
typedef struct khh_kang khh_kang;
khh_kang* khh_kang_new(const uint8_t pub_xy[64], const uint8_t start_be[32], const uint8_t end_be[32], int dp_bits,
                       uint64_t herd, uint64_t seed, uint64_t herd_cap, char* err, size_t errlen);
void khh_kang_free(khh_kang* k);
int khh_kang_params(const khh_kang* k, uint32_t* dp_bits, uint64_t* herd, uint32_t* width_bits);
/* The jumps as khb_kang_load_jumps takes them: 32 distances (32 bytes BE) and 32 points (x||y BE). */
int khh_kang_jumps(const khh_kang* k, uint8_t* dist_be, uint8_t* xy);
/* The first n kangaroos a search gives its device number `stream` (0 for the first), by the host's own k*G. */
int khh_kang_make_herd(const khh_kang* k, uint32_t stream, uint64_t n, uint8_t* xy, uint8_t* dist_be);
/* The step rule on the portable field of device/fe.hpp, so the host logic is testable without a GPU: the n kangaroos
 * (x||y BE, distances 32 bytes BE, updated in place) make `steps` jumps each.  The distinguished points come step by
 * step, ascending kangaroo within a step: up to cap of them in dp_kangaroo / dp_x_be / dp_dist_be (any may be NULL),
 * *n_dp counts them all, *second_choice the times the x == J_j.x rule fired. */
int khh_kang_cpu_walk(const khh_kang* k, uint8_t* xy, uint8_t* dist_be, uint64_t n, uint32_t steps, uint32_t dp_bits,
                      uint32_t* dp_kangaroo, uint8_t* dp_x_be, uint8_t* dp_dist_be, uint64_t cap, uint64_t* n_dp,
                      uint64_t* second_choice);
/* Tests: ring entries per launch (0 = sized from the herd); the first n kangaroos of the first device's herd; keep
 * that device's herd as the search leaves it, for khh_kang_final_herd (*n = its size, up to cap copied). */
int khh_kang_set_ring_capacity(khh_kang* k, uint32_t cap);
int khh_kang_plant(khh_kang* k, const uint8_t* xy, const uint8_t* dist_be, uint64_t n);
int khh_kang_keep_herd(khh_kang* k, int keep);
int khh_kang_final_herd(const khh_kang* k, uint8_t* xy, uint8_t* dist_be, uint64_t cap, uint64_t* n);
/* One host thread and one herd per device, one shared table of distinguished points that grows and is never
 * truncated.  n_devices == 0: one herd walks on the CPU through khh_kang_cpu_walk's code.  max_steps: jumps in all
 * (0 = no limit); reaching it leaves *found = 0 and is no error.  After a launch whose ring overflowed the launches
 * are halved; the lost points cost time, not correctness, and are counted.  stats_out[0 .. stats_len) of
 * KHH_KANG_STATS values: steps, distinguished points digested, dead (merged kangaroos replaced), lost points,
 * launches, microseconds. */
#define KHH_KANG_STATS 6
int khh_kang_search(khh_kang* k, const int* devices, int n_devices, uint64_t max_steps, uint8_t key_be[32],
                    int* found, uint64_t* stats_out, uint32_t stats_len, char* err, size_t errlen);

#ifdef __cplusplus
}
#endif
#endif
