"""ctypes binding of libkhbsgs.so (include/khbsgs.h): the MI355X giant-step scan.

Replaces the CPU group loop of keyhunt.cpp:3867-4004 (thread_process_bsgs).  No fallback: if the
library or a gfx950 device is missing, KhbError is raised.
"""
from __future__ import annotations

import ctypes as C
import os

from . import LIB_DIR

LIB_PATH = os.path.join(LIB_DIR, "libkhbsgs.so")

KHB_GROUP = 1024


class KhbError(RuntimeError):
    code = 0                            # the KHB_E* value when a library call failed (_check)


class Cand(C.Structure):
    _fields_ = [("job", C.c_uint32), ("a", C.c_uint32)]


class Degenerate(C.Structure):
    _fields_ = [("job", C.c_uint32), ("group", C.c_uint32)]


class AddrHit(C.Structure):
    _fields_ = [("job", C.c_uint32), ("group", C.c_uint32), ("t", C.c_uint32), ("kind", C.c_uint32)]


class CheckTables(C.Structure):     # khb_check_tables
    _fields_ = [("gtable", C.c_char_p), ("amp2", C.c_char_p), ("amp3", C.c_char_p),
                ("l2", C.c_char_p), ("l2_bytes_per_sub", C.c_uint64), ("l2_bits_per_sub", C.c_uint64),
                ("l2_hashes", C.c_uint32),
                ("l3", C.c_char_p), ("l3_bytes_per_sub", C.c_uint64), ("l3_bits_per_sub", C.c_uint64),
                ("l3_hashes", C.c_uint32),
                ("bptable", C.c_char_p), ("m3", C.c_uint64),
                ("m_double_be", C.c_uint8 * 32), ("m2_double_be", C.c_uint8 * 32), ("m3_be", C.c_uint8 * 32),
                ("m3_double_be", C.c_uint8 * 32)]


class CheckIn(C.Structure):        # khb_check_in
    _fields_ = [("start_be", C.c_uint8 * 32), ("a", C.c_uint32), ("target", C.c_uint32)]


class CheckOut(C.Structure):       # khb_check_out
    _fields_ = [("key_be", C.c_uint8 * 32), ("found", C.c_uint32), ("l2_hits", C.c_uint32),
                ("l3_hits", C.c_uint32), ("bp_hits", C.c_uint32)]


class Stats(C.Structure):
    _fields_ = [("n_cand", C.c_uint32), ("n_degenerate", C.c_uint32), ("giant_steps", C.c_uint64),
                ("kernel_ms", C.c_float), ("launch_begin_ms", C.c_double), ("launch_end_ms", C.c_double),
                ("shader_mhz", C.c_float), ("event_ms", C.c_float)]


class MiniHit(C.Structure):        # khb_mini_hit
    _fields_ = [("offset", C.c_uint64), ("h160", C.c_uint8 * 20)]


class MiniStats(C.Structure):      # khb_mini_stats
    _fields_ = [("candidates", C.c_uint64), ("valid", C.c_uint64), ("bad_keys", C.c_uint64), ("hits", C.c_uint64),
                ("queue_overflow", C.c_uint32), ("hit_overflow", C.c_uint32), ("filter_ms", C.c_float),
                ("keys_ms", C.c_float)]


class KangDp(C.Structure):         # khb_kang_dp
    _fields_ = [("kangaroo", C.c_uint32), ("x_be", C.c_uint8 * 32), ("dist_be", C.c_uint8 * 32)]


class KangStats(C.Structure):      # khb_kang_stats
    _fields_ = [("steps_walked", C.c_uint64), ("n_dp", C.c_uint64), ("second_choice", C.c_uint64),
                ("dp_overflow", C.c_uint32), ("kernel_ms", C.c_float)]


MINI_ALPHABET = b"123456789ABCDEFGHJKLMNPQRSTUVWXYZabcdefghijkmnopqrstuvwxyz"   # the reference's Ccoinbuffer_default

_libs: dict[str, C.CDLL] = {}
KHB_ABI_VERSION = 7
TABLE_L1, TABLE_GATE, TABLE_FOLD, TABLE_STAGE0 = 0, 1, 2, 3      # include/khbsgs.h KHB_TABLE_*
FIELD_OP_RAW = 0x100                                             # include/khbsgs.h KHB_FIELD_OP_RAW
SEARCH_ENDOMORPHISM, SEARCH_ETH, ADDR_KIND_ETH = 4, 8, 16        # include/khbsgs.h KHB_SEARCH_*, KHB_ADDR_KIND_ETH
SEARCH_XPOINT, ADDR_KIND_X = 16, 32                              # KHB_SEARCH_XPOINT, KHB_ADDR_KIND_X (| e << 2)
SEARCH_VANITY = 32                                               # KHB_SEARCH_VANITY (| -l value, optionally | -e)


def lib(path: str | None = None) -> C.CDLL:
    """The bound library; `path` selects an alternative build (kernel variants in tools/)."""
    path = path or LIB_PATH
    if path not in _libs:
        if not os.path.exists(path):
            raise KhbError(f"{path} not built: run `make` (or __graft_entry__.build())")
        L = C.CDLL(path)
        P = C.POINTER
        # include/khbsgs.h KHB_ABI_VERSION: the structs and signatures below are written for it (older
        # timing-only variant builds without the symbol are accepted for tools/perf_variants.py)
        if hasattr(L, "khb_abi_version"):
            v = L.khb_abi_version()
            if v != KHB_ABI_VERSION:
                raise KhbError(f"{path}: ABI {v}, this binding is written for {KHB_ABI_VERSION}: rebuild (`make`)")
        elif path == LIB_PATH:
            raise KhbError(f"{path} predates khb_abi_version: rebuild (`make`)")
        L.khb_device_count.argtypes = [P(C.c_int)]
        L.khb_open.argtypes = [C.c_int, C.c_uint32, P(C.c_void_p)]
        L.khb_close.argtypes = [C.c_void_p]
        L.khb_strerror.restype = C.c_char_p
        L.khb_strerror.argtypes = [C.c_int]
        L.khb_last_hip_error.argtypes = [C.c_void_p]
        L.khb_stream.restype = C.c_void_p
        L.khb_stream.argtypes = [C.c_void_p]
        L.khb_lanes.restype = C.c_uint32
        L.khb_lanes.argtypes = [C.c_void_p]
        L.khb_default_lanes.restype = C.c_uint32
        L.khb_default_lanes.argtypes = [C.c_int]
        L.khb_groups_per_item.restype = C.c_uint32
        L.khb_groups_per_item.argtypes = []
        for name in ("khb_reserve_slots", "khb_set_candidate_capacity"):
            if hasattr(L, name):                 # absent only in older timing builds
                getattr(L, name).argtypes = [C.c_void_p, C.c_uint32 if "capacity" in name else C.c_int]
        if hasattr(L, "khb_candidate_capacity"):
            L.khb_candidate_capacity.restype = C.c_uint32
            L.khb_candidate_capacity.argtypes = [C.c_void_p]
            L.khb_reset_epoch.argtypes = [C.c_void_p]
        L.khb_load_bloom.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint32]
        L.khb_load_giant_table.argtypes = [C.c_void_p, C.c_char_p]
        L.khb_load_gate.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32, C.c_uint32]
        if hasattr(L, "khb_set_gate_stage1"):    # absent only in older timing builds (tools/perf_variants.py)
            L.khb_set_gate_stage1.argtypes = [C.c_void_p, C.c_uint32]
        if hasattr(L, "khb_build_info"):         # ABI 7
            L.khb_build_info.restype = C.c_char_p
            L.khb_build_info.argtypes = []
            L.khb_set_gate_stage0.argtypes = [C.c_void_p, C.c_uint32]
            L.khb_gate_stages.argtypes = [C.c_void_p]
            L.khb_last_handoff.argtypes = [C.c_void_p, P(C.c_uint32), P(C.c_uint32)]
        if hasattr(L, "khb_build_l1_resident"):  # the resident additions to ABI 7
            L.khb_build_l1_resident.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64,
                                                C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, P(C.c_float)]
            L.khb_mem_info.argtypes = [C.c_void_p, P(C.c_uint64), P(C.c_uint64), P(C.c_uint64)]
            L.khb_resident_bytes.argtypes = [C.c_void_p, C.c_int, P(C.c_uint64)]
            L.khb_resident_read.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_uint64, C.c_char_p]
            L.khb_resident_popcount.argtypes = [C.c_void_p, C.c_int, P(C.c_uint64)]
            L.khb_gate_probe.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_uint32]
        if hasattr(L, "khb_build_baby"):         # absent only in older timing builds
            L.khb_build_baby.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64,
                                         C.c_uint64, P(C.c_uint64), P(C.c_uint64), P(C.c_uint32), C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                         P(C.c_float)]
        L.khb_load_lane_offsets.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32, C.c_uint32]
        L.khb_submit.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32]
        L.khb_collect.argtypes = [C.c_void_p, P(Cand), C.c_uint32, P(Degenerate), C.c_uint32, P(Stats)]
        L.khb_scan.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, P(Cand), C.c_uint32,
                               P(Stats)]
        L.khb_dump_x.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32, C.c_uint32, C.c_char_p]
        L.khb_field_op.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32]
        L.khb_probe.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_uint32]
        L.khb_load_addr_bloom.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint32]
        L.khb_addr_submit.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int]
        L.khb_addr_collect.argtypes = [C.c_void_p, P(AddrHit), C.c_uint32, P(Stats)]
        L.khb_addr_scan.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int,
                                    P(AddrHit), C.c_uint32, P(Stats)]
        L.khb_addr_dump.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32, C.c_uint32, C.c_char_p]
        L.khb_hash160.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_char_p, C.c_uint32]
        if hasattr(L, "khb_load_vanity"):        # the -m vanity additions to ABI 7
            L.khb_load_vanity.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_uint32]
            L.khb_vanity_match.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_uint32]
        if hasattr(L, "khb_load_mini_table"):    # the -m minikeys additions to ABI 7
            L.khb_load_mini_table.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32]
            L.khb_addr_hit_capacity.restype = C.c_uint32
            L.khb_addr_hit_capacity.argtypes = [C.c_void_p]
            L.khb_mini_submit.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.c_char_p]
            L.khb_mini_collect.argtypes = [C.c_void_p, P(MiniHit), C.c_uint32, P(MiniStats)]
            L.khb_mini_scan.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.c_char_p, P(MiniHit), C.c_uint32,
                                        P(MiniStats)]
            L.khb_mini_set_queue_capacity.argtypes = [C.c_void_p, C.c_uint32]
            L.khb_mini_queue_capacity.restype = C.c_uint32
            L.khb_mini_queue_capacity.argtypes = [C.c_void_p, C.c_uint64]
            L.khb_mini_filter.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.c_char_p, P(C.c_uint64), C.c_uint32,
                                          P(C.c_uint64)]
            L.khb_mini_pubkey.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32]
        if hasattr(L, "khb_kang_submit"):        # the kangaroo additions to ABI 7
            L.khb_kang_per_lane.restype = C.c_uint32
            L.khb_kang_per_lane.argtypes = []
            L.khb_kang_full_herd.restype = C.c_uint32
            L.khb_kang_full_herd.argtypes = [C.c_int]
            L.khb_kang_load_jumps.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
            L.khb_kang_store.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_char_p, C.c_char_p]
            L.khb_kang_read.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_char_p, C.c_char_p]
            L.khb_kang_herd.restype = C.c_uint32
            L.khb_kang_herd.argtypes = [C.c_void_p]
            L.khb_kang_submit.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
            L.khb_kang_collect.argtypes = [C.c_void_p, P(KangDp), C.c_uint32, P(KangStats)]
            L.khb_kang_set_ring_capacity.argtypes = [C.c_void_p, C.c_uint32]
            L.khb_kang_ring_capacity.restype = C.c_uint32
            L.khb_kang_ring_capacity.argtypes = [C.c_void_p]
        if hasattr(L, "khb_check"):              # ABI 5
            L.khb_load_check_tables.argtypes = [C.c_void_p, P(CheckTables)]
            L.khb_check.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32, P(CheckIn), C.c_uint32, P(CheckOut)]
        _libs[path] = L
    return _libs[path]


KHB_EINVAL, KHB_ESTATE, KHB_EBUSY, KHB_EINCOMPLETE = -1, -5, -6, -7
KHB_EHANDOFF = -8


def _check(rc: int, ctx=None, L: C.CDLL | None = None) -> None:
    if rc != 0:
        L = L or lib()
        msg = L.khb_strerror(rc).decode()
        if ctx and rc == KHB_EHANDOFF and hasattr(L, "khb_last_handoff"):
            seen, total = C.c_uint32(0), C.c_uint32(0)
            L.khb_last_handoff(ctx, C.byref(seen), C.byref(total))
            msg += f" ({seen.value} of {total.value} waves)"
        elif ctx:
            msg += f" (hipError {L.khb_last_hip_error(ctx)})"
        err = KhbError(f"khbsgs: {msg} [{rc}]")
        err.code = rc
        raise err


def build_info(path: str | None = None) -> dict:
    """khb_build_info of the library at `path` (the in-tree build by default) as a dict, plus its path and the
    first 16 hex digits of its sha256: what a bench line records so that its number names the kernel."""
    import hashlib
    path = os.path.realpath(path or LIB_PATH)
    L = lib(path)
    info = {}
    if hasattr(L, "khb_build_info"):
        for w in L.khb_build_info().decode().split(" compiler=")[0].split():
            k, _, v = w.partition("=")
            info[k] = v
        info["compiler"] = L.khb_build_info().decode().split(" compiler=", 1)[-1]
    with open(path, "rb") as f:
        info["sha16"] = hashlib.sha256(f.read()).hexdigest()[:16]
    info["path"] = path
    return info


def kang_per_lane(path: str | None = None) -> int:
    """Kangaroo slots per lane of the walk kernel (khb_kang_per_lane), a build-time constant."""
    return int(lib(path).khb_kang_per_lane())


def groups_per_item() -> int:
    """Groups per work item of the -m bsgs scan kernel (khb_groups_per_item)."""
    return int(lib().khb_groups_per_item())


def default_lanes(device: int = 0) -> int:
    """Work lanes of one full residency on `device` (khb_default_lanes; 0 = unusable)."""
    return int(lib().khb_default_lanes(device))


def device_count() -> int:
    n = C.c_int(0)
    _check(lib().khb_device_count(C.byref(n)))
    return n.value


class Engine:
    """One libkhbsgs context (one device)."""

    def __init__(self, device: int = 0, lanes: int = 0, lib_path: str | None = None):
        self.L = lib(lib_path)
        self.h = C.c_void_p()
        _check(self.L.khb_open(device, lanes, C.byref(self.h)), None, self.L)
        self.gpl = 0
        self._kang_rings: list[int] = []                 # ring capacities of the kangaroo launches in flight

    def close(self) -> None:
        if self.h:
            self.L.khb_close(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def lanes(self) -> int:
        return int(self.L.khb_lanes(self.h))

    def stream(self) -> int:
        return int(self.L.khb_stream(self.h) or 0)

    def reserve_slots(self, depth: int) -> None:
        _check(self.L.khb_reserve_slots(self.h, depth), self.h, self.L)

    def set_candidate_capacity(self, cap: int) -> None:
        _check(self.L.khb_set_candidate_capacity(self.h, cap), self.h, self.L)

    def candidate_capacity(self) -> int:
        return int(self.L.khb_candidate_capacity(self.h))

    def reset_epoch(self) -> None:
        _check(self.L.khb_reset_epoch(self.h), self.h, self.L)

    def load_bloom(self, bf: bytes, bytes_per_sub: int, bits: int, hashes: int) -> None:
        assert len(bf) == 256 * bytes_per_sub
        _check(self.L.khb_load_bloom(self.h, bf, bytes_per_sub, bits, hashes), self.h, self.L)

    def load_gate(self, gate: bytes | None, log2_bits: int = 0, probes: int = 1) -> None:
        """Level-0 gate in front of the L1 probe (None removes it); probes = bits per x."""
        if gate is not None:
            assert len(gate) == (1 << log2_bits) // 8
        _check(self.L.khb_load_gate(self.h, gate, log2_bits if gate is not None else 0, probes), self.h, self.L)

    def set_gate_stage0(self, log2_bytes: int) -> None:
        """Stage-0 filter size for gates loaded later (0 none, 1 = KHB_GATE_STAGE0_AUTO, else log2 bytes)."""
        _check(self.L.khb_set_gate_stage0(self.h, log2_bytes), self.h, self.L)

    def gate_stages(self) -> int:
        """khb_gate_stages: bit 2 gate, bit 1 stage-1 fold, bit 0 stage-0 filter."""
        return int(self.L.khb_gate_stages(self.h))

    def set_gate_stage1(self, log2_bytes: int) -> None:
        """Stage-1 fold size (2^log2_bytes bytes) for gates loaded afterwards; 0 = none."""
        _check(self.L.khb_set_gate_stage1(self.h, log2_bytes), self.h, self.L)

    def load_giant_table(self, gsn: bytes) -> None:
        assert len(gsn) == 513 * 64
        _check(self.L.khb_load_giant_table(self.h, gsn), self.h, self.L)

    def load_lane_offsets(self, offs: bytes, gpl: int) -> None:
        assert len(offs) % 64 == 0
        _check(self.L.khb_load_lane_offsets(self.h, offs, len(offs) // 64, gpl), self.h, self.L)
        self.gpl = gpl

    def submit(self, centres: bytes, group_begin: int, group_count: int) -> None:
        _check(self.L.khb_submit(self.h, centres, len(centres) // 64, group_begin, group_count), self.h, self.L)

    def collect(self, cap: int = 1 << 20):
        cand = (Cand * cap)()
        deg = (Degenerate * 4096)()
        st = Stats()
        _check(self.L.khb_collect(self.h, cand, cap, deg, 4096, C.byref(st)), self.h, self.L)
        n = min(st.n_cand, cap)
        return ([(int(cand[i].job), int(cand[i].a)) for i in range(n)],
                [(int(deg[i].job), int(deg[i].group)) for i in range(min(st.n_degenerate, 4096))], st)

    def scan(self, centres: bytes, group_begin: int, group_count: int, cap: int = 1 << 20):
        self.submit(centres, group_begin, group_count)
        return self.collect(cap)

    def dump_x(self, centre: bytes, group_begin: int, group_count: int) -> bytes:
        out = C.create_string_buffer(group_count * KHB_GROUP * 32)
        _check(self.L.khb_dump_x(self.h, centre, group_begin, group_count, out), self.h, self.L)
        return out.raw

    def field_op(self, op: int, a: bytes, b: bytes | None) -> bytes:
        """khb_field_op; op | FIELD_OP_RAW (op 0, 1, 3, 5, 6) returns the lazy value, not canonicalised."""
        n = len(a) // 32
        out = C.create_string_buffer(n * 32)
        _check(self.L.khb_field_op(self.h, op, a, b, out, n), self.h, self.L)
        return out.raw

    def probe(self, xs: bytes) -> bytes:
        n = len(xs) // 32
        out = C.create_string_buffer(n)
        _check(self.L.khb_probe(self.h, xs, out, n), self.h, self.L)
        return out.raw

    # ---- baby-step tables on the GPU ----
    def build_baby(self, centres: bytes, groups_per_job: int, l1ext: int, m2: int, m3: int, geoms,
                   want=("l1", "l2", "l3", "bp", "gate"), gate_log2: int = 0, gate_probes: int = 3,
                   fill: int = 0) -> dict:
        """khb_build_baby over the loaded Gn table and build offsets.  geoms: (bytes_per_sub, bits, hashes) of levels
        1..3, None for a level that is not in `want`; want: which of "l1", "l2", "l3", "bp", "gate" to build (the
        others go in as null pointers).  Every host buffer is filled with the byte `fill` before the call, so what
        the call leaves untouched shows, and is followed by 64 guard bytes that must come back as they were.
        Returns {"l1", "l2", "l3", "bp", "gate"} (bytes, or None when not wanted), "kernel_ms" and "incomplete" (True
        when the library answered KHB_EINCOMPLETE: the buffers hold what a short walk wrote)."""
        want = set(want)
        if want - {"l1", "l2", "l3", "bp", "gate"}:
            raise ValueError(f"build_baby: unknown outputs {sorted(want)}")
        nb, bits, hashes = (C.c_uint64 * 3)(), (C.c_uint64 * 3)(), (C.c_uint32 * 3)()
        sizes = {"bp": 16 * m3, "gate": (1 << gate_log2) // 8}
        for l, g in enumerate(geoms):
            if g is not None:
                nb[l], bits[l], hashes[l] = g
                sizes[f"l{l + 1}"] = 256 * g[0]
            elif f"l{l + 1}" in want:
                raise ValueError(f"build_baby: level {l + 1} wanted without a geometry")
        guard = b"\x5a" * 64             # behind every buffer: the library must not write past what it was given
        bufs = {k: C.create_string_buffer(bytes([fill]) * sizes[k] + guard, sizes[k] + len(guard)) if k in want
                else None for k in ("l1", "l2", "l3", "bp", "gate")}
        ms = C.c_float(0)
        rc = self.L.khb_build_baby(self.h, centres, len(centres) // 64, groups_per_job, l1ext, m2, m3, nb, bits,
                                   hashes, bufs["l1"], bufs["l2"], bufs["l3"], bufs["bp"], bufs["gate"], gate_log2,
                                   gate_probes, C.byref(ms))
        if rc != KHB_EINCOMPLETE:
            _check(rc, self.h, self.L)
        for k, b in bufs.items():
            if b is not None and b.raw[sizes[k]:] != guard:
                raise KhbError(f"khbsgs: khb_build_baby wrote past the {sizes[k]} bytes of {k}")
        out = {k: b.raw[:sizes[k]] if b is not None else None for k, b in bufs.items()}
        out["kernel_ms"] = float(ms.value)
        out["incomplete"] = rc == KHB_EINCOMPLETE
        return out

    # ---- resident level-1 bloom and gate (additions to ABI 7) ----
    def build_l1_resident(self, centres: bytes, groups_per_job: int, l1ext: int, bytes_per_sub: int, bits: int,
                          hashes: int, gate_log2: int = 0, gate_probes: int = 3) -> float:
        """khb_build_l1_resident over the loaded Gn table and build offsets: the level-1 bloom and its gate are
        built on the device and installed there.  Returns the build kernel's ms."""
        ms = C.c_float(0)
        _check(self.L.khb_build_l1_resident(self.h, centres, len(centres) // 64, groups_per_job, l1ext, bytes_per_sub,
                                            bits, hashes, gate_log2, gate_probes, C.byref(ms)), self.h, self.L)
        return float(ms.value)

    def mem_info(self) -> tuple[int, int, int]:
        """(free, total, bytes of one submission slot's scratch) of the context's device."""
        f, t, s = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        _check(self.L.khb_mem_info(self.h, C.byref(f), C.byref(t), C.byref(s)), self.h, self.L)
        return int(f.value), int(t.value), int(s.value)

    def resident_bytes(self, which: int) -> int:
        n = C.c_uint64(0)
        _check(self.L.khb_resident_bytes(self.h, which, C.byref(n)), self.h, self.L)
        return int(n.value)

    def resident_read(self, which: int, offset: int = 0, nbytes: int | None = None) -> bytes:
        """A window of an installed table (TABLE_*); the whole table by default."""
        if nbytes is None:
            nbytes = self.resident_bytes(which) - offset
        out = C.create_string_buffer(max(1, nbytes))
        _check(self.L.khb_resident_read(self.h, which, offset, nbytes, out), self.h, self.L)
        return out.raw[:nbytes]

    def resident_popcount(self, which: int) -> int:
        n = C.c_uint64(0)
        _check(self.L.khb_resident_popcount(self.h, which, C.byref(n)), self.h, self.L)
        return int(n.value)

    def gate_probe(self, xs: bytes) -> bytes:
        """Per 32-byte BE x: bit 0 the full gate passes, bit 1 the stage-1 fold, bit 2 the stage-0 filter."""
        n = len(xs) // 32
        out = C.create_string_buffer(n)
        _check(self.L.khb_gate_probe(self.h, xs, out, n), self.h, self.L)
        return out.raw

    # ---- -m address ----
    def load_addr_bloom(self, bf: bytes, bits: int, hashes: int) -> None:
        _check(self.L.khb_load_addr_bloom(self.h, bf, len(bf), bits, hashes), self.h, self.L)

    def addr_scan(self, centres: bytes, group_begin: int, group_count: int, search: int = 2, cap: int = 1 << 18):
        """Bloom hits [(job, group, t, kind)] of -m address over group_count groups of each job (search: 0/1/2,
        | SEARCH_ENDOMORPHISM, SEARCH_ETH, or SEARCH_XPOINT optionally | SEARCH_ENDOMORPHISM; | SEARCH_VANITY on the
        -l values: every hash inside the table of load_vanity is a hit)."""
        hits = (AddrHit * cap)()
        st = Stats()
        _check(self.L.khb_addr_scan(self.h, centres, len(centres) // 64, group_begin, group_count, search, hits, cap,
                                    C.byref(st)), self.h, self.L)
        n = min(st.n_cand, cap)
        return [(int(hits[i].job), int(hits[i].group), int(hits[i].t), int(hits[i].kind)) for i in range(n)], st

    # ---- -m vanity ----
    def load_vanity(self, intervals) -> None:
        """The interval table of -m vanity: [(lo, hi)] of 20-byte big-endian bounds, sorted and disjoint."""
        lo = b"".join(bytes(a) for a, _ in intervals)
        hi = b"".join(bytes(b) for _, b in intervals)
        _check(self.L.khb_load_vanity(self.h, lo, hi, len(intervals)), self.h, self.L)

    def vanity_match(self, h20: bytes) -> bytes:
        """One byte per 20-byte value: 1 iff it lies in an interval of the loaded table (the kernels' own match)."""
        n = len(h20) // 20
        out = C.create_string_buffer(n)
        _check(self.L.khb_vanity_match(self.h, bytes(h20), out, n), self.h, self.L)
        return out.raw

    # ---- the kangaroo walk ----
    def kang_load_jumps(self, jumps) -> None:
        """The 32 jumps [(s_j, (x, y))], J_j = s_j * G (khhost.Kangaroo.jump_table)."""
        if len(jumps) != 32:
            raise ValueError("32 jumps")
        dist = b"".join(s.to_bytes(32, "big") for s, _ in jumps)
        xy = b"".join(x.to_bytes(32, "big") + y.to_bytes(32, "big") for _, (x, y) in jumps)
        _check(self.L.khb_kang_load_jumps(self.h, dist, xy), self.h, self.L)

    def kang_store(self, herd, first: int = 0) -> None:
        """Kangaroos first .. of the herd from [(x, y, d)]; an empty list with first = 0 forgets the herd."""
        xy = b"".join(x.to_bytes(32, "big") + y.to_bytes(32, "big") for x, y, _ in herd)
        d = b"".join(d.to_bytes(32, "big") for _, _, d in herd)
        _check(self.L.khb_kang_store(self.h, first, len(herd), xy or None, d or None), self.h, self.L)

    def kang_herd(self) -> int:
        return int(self.L.khb_kang_herd(self.h))

    def kang_read(self, first: int = 0, n: int | None = None):
        """[(x, y, d)] of kangaroos first .. first + n - 1 (to the herd's end by default)."""
        n = self.kang_herd() - first if n is None else n
        xy, d = C.create_string_buffer(64 * n), C.create_string_buffer(32 * n)
        _check(self.L.khb_kang_read(self.h, first, n, xy, d), self.h, self.L)
        f = int.from_bytes
        return [(f(xy.raw[64 * i:64 * i + 32], "big"), f(xy.raw[64 * i + 32:64 * i + 64], "big"),
                 f(d.raw[32 * i:32 * i + 32], "big")) for i in range(n)]

    def kang_set_ring_capacity(self, cap: int) -> None:
        _check(self.L.khb_kang_set_ring_capacity(self.h, cap), self.h, self.L)

    def kang_submit(self, steps: int, dp_bits: int) -> None:
        ring = int(self.L.khb_kang_ring_capacity(self.h))
        _check(self.L.khb_kang_submit(self.h, steps, dp_bits), self.h, self.L)
        self._kang_rings.append(ring)                    # the launch keeps the capacity it was submitted with

    def kang_collect(self, cap: int | None = None):
        """The oldest launch's distinguished points [(kangaroo, x, d)] (unordered, up to cap: the capacity of that
        launch's ring by default) and its KangStats."""
        ring = self._kang_rings[0] if self._kang_rings else int(self.L.khb_kang_ring_capacity(self.h))
        cap = ring if cap is None else cap
        out = (KangDp * max(cap, 1))()
        st = KangStats()
        rc = self.L.khb_kang_collect(self.h, out, cap, C.byref(st))
        if rc != KHB_ESTATE and self._kang_rings:        # the launch is retired whatever else the call answers
            self._kang_rings.pop(0)
        _check(rc, self.h, self.L)
        n = min(st.n_dp, cap, ring)                      # what the ring kept: the counter goes on past its capacity
        f = int.from_bytes
        return [(out[i].kangaroo, f(bytes(out[i].x_be), "big"), f(bytes(out[i].dist_be), "big")) for i in range(n)], st

    def kang_walk(self, steps: int, dp_bits: int, cap: int | None = None):
        """One launch: kang_submit and kang_collect."""
        self.kang_submit(steps, dp_bits)
        return self.kang_collect(cap)

    # ---- -m minikeys ----
    def load_mini_table(self, points: bytes, window_bits: int) -> None:
        """The window table of the device's k*G (khhost.Minikeys.table_points): d * 2^(w j) * G, 64 bytes each."""
        if window_bits in (4, 8, 16):
            assert len(points) == 64 * (256 // window_bits) * ((1 << window_bits) - 1)
        _check(self.L.khb_load_mini_table(self.h, points, window_bits), self.h, self.L)

    def set_mini_queue_capacity(self, cap: int) -> None:
        """Survivor-queue entries of later launches (0 = sized from the launch); for tests of the overflow path."""
        _check(self.L.khb_mini_set_queue_capacity(self.h, cap), self.h, self.L)

    def mini_scan(self, first_digits: bytes, count: int, alphabet: bytes = MINI_ALPHABET, cap: int = 1 << 18):
        """Bloom hits [(offset, hash160)] among the candidates first .. first + count - 1 (21 digit values), and the
        launch's MiniStats.  An overflow flag in the stats means the hits are incomplete."""
        hits = (MiniHit * cap)()
        st = MiniStats()
        _check(self.L.khb_mini_scan(self.h, bytes(first_digits), count, bytes(alphabet), hits, cap, C.byref(st)),
               self.h, self.L)
        n = min(st.hits, cap, self.L.khb_addr_hit_capacity(self.h))      # what the ring kept
        return [(int(hits[i].offset), bytes(hits[i].h160)) for i in range(n)], st

    def mini_filter(self, first_digits: bytes, count: int, alphabet: bytes = MINI_ALPHABET, cap: int = 1 << 20):
        """The filter kernel alone: (offsets of the valid candidates as the queue holds them, their number)."""
        out = (C.c_uint64 * max(1, cap))()
        n = C.c_uint64(0)
        _check(self.L.khb_mini_filter(self.h, bytes(first_digits), count, bytes(alphabet), out, cap, C.byref(n)),
               self.h, self.L)
        return [int(out[i]) for i in range(min(n.value, cap))], int(n.value)

    def mini_pubkey(self, scalars: list[int]) -> list[tuple[bytes, int]]:
        """[(x||y, bad-key flag)] of k*G over the loaded table for each scalar below 2^256."""
        n = len(scalars)
        xy = C.create_string_buffer(64 * n)
        fl = C.create_string_buffer(n)
        _check(self.L.khb_mini_pubkey(self.h, b"".join(k.to_bytes(32, "big") for k in scalars), xy, fl, n),
               self.h, self.L)
        r, f = xy.raw, fl.raw
        return [(r[64 * i:64 * i + 64], f[i]) for i in range(n)]

    def addr_dump(self, centre: bytes, group_begin: int, group_count: int) -> bytes:
        out = C.create_string_buffer(group_count * KHB_GROUP * 64)
        _check(self.L.khb_addr_dump(self.h, centre, group_begin, group_count, out), self.h, self.L)
        return out.raw

    def hash160(self, kind: int, xy: bytes) -> list[tuple[bytes, int]]:
        """[(hash160, bloom bit)] of each x||y point for kind 0/1 (compressed 02/03) or 2; kind 3: its ETH address;
        kind 4: the first 20 bytes of x (-m xpoint)."""
        n = len(xy) // 64
        out = C.create_string_buffer(21 * n)
        _check(self.L.khb_hash160(self.h, kind, xy, out, n), self.h, self.L)
        r = out.raw
        return [(r[21 * i:21 * i + 20], r[21 * i + 20]) for i in range(n)]

    # ---- second / third check (khb_load_check_tables, khb_check) ----
    def load_check_tables(self, gtable: bytes, amp2: bytes, amp3: bytes, l2: tuple, l3: tuple, bptable: bytes,
                          m3: int, m_double: int, m2_double: int, m3_value: int, m3_double: int) -> None:
        """l2 / l3: (256 sub-blooms concatenated, bytes per sub-bloom, bits, hashes) as bloom_concat gives them.
        The library copies every table to the device before it returns."""
        assert len(gtable) == 32 * 256 * 64 and len(amp2) == len(amp3) == 32 * 64 and len(bptable) == 16 * m3
        t = CheckTables()
        t.gtable, t.amp2, t.amp3 = gtable, amp2, amp3
        t.l2, t.l2_bytes_per_sub, t.l2_bits_per_sub, t.l2_hashes = l2
        t.l3, t.l3_bytes_per_sub, t.l3_bits_per_sub, t.l3_hashes = l3
        t.bptable, t.m3 = bptable, m3
        for name, v in (("m_double_be", m_double), ("m2_double_be", m2_double), ("m3_be", m3_value),
                        ("m3_double_be", m3_double)):
            getattr(t, name)[:] = list(v.to_bytes(32, "big"))
        _check(self.L.khb_load_check_tables(self.h, C.byref(t)), self.h, self.L)

    def check(self, targets_xy: list[bytes], cands: list[tuple[int, int, int]]) -> list[dict]:
        """bsgs_secondcheck on the device for [(chunk base, giant step a, target index)]: per candidate
        {"found", "key" (int or None), "l2_hits", "l3_hits", "bp_hits"}."""
        n = len(cands)
        ins = (CheckIn * max(1, n))()
        for i, (base, a, k) in enumerate(cands):
            ins[i].start_be[:] = list(base.to_bytes(32, "big"))
            ins[i].a = a
            ins[i].target = k
        outs = (CheckOut * max(1, n))()
        _check(self.L.khb_check(self.h, b"".join(targets_xy), len(targets_xy), ins, n, outs), self.h, self.L)
        return [{"found": int(o.found), "key": int.from_bytes(bytes(o.key_be), "big") if o.found else None,
                 "l2_hits": int(o.l2_hits), "l3_hits": int(o.l3_hits), "bp_hits": int(o.bp_hits)}
                for o in outs[:n]]
