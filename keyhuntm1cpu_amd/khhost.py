"""ctypes binding of libkhhost.so (include/khhost.h): the C++ host engine — BSGS geometry, tables,
chunk centres, second/third check and the multi-GPU search driver the keyhunt_amd CLI runs."""
from __future__ import annotations

import ctypes as C
import os

from . import LIB_DIR

LIB_PATH = os.path.join(LIB_DIR, "libkhhost.so")

_lib = None


KHH_ABI_VERSION = 12                # include/khhost.h
KHH_SESSION_STATS, KHH_ADDR_STATS = 12, 8
KHH_MINI_STATS = 8
KHH_KANG_STATS = 6
MINI_ALPHABET = "123456789ABCDEFGHJKLMNPQRSTUVWXYZabcdefghijkmnopqrstuvwxyz"   # Ccoinbuffer_default
KHH_RESIDENT_INFO = 8
TABLE_L1, TABLE_GATE, TABLE_FOLD, TABLE_STAGE0 = 0, 1, 2, 3      # include/khbsgs.h KHB_TABLE_*


class KhhError(RuntimeError):
    pass


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise KhhError(f"{LIB_PATH} not built: run `make`")
        L = C.CDLL(LIB_PATH)
        P = C.POINTER
        v = L.khh_abi_version() if hasattr(L, "khh_abi_version") else 0
        if v != KHH_ABI_VERSION:        # include/khhost.h KHH_ABI_VERSION
            raise KhhError(f"{LIB_PATH}: ABI {v}, this binding is written for {KHH_ABI_VERSION}: rebuild (`make`)")
        L.khh_tables_new.restype = C.c_void_p
        L.khh_tables_new.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_uint32, C.c_char_p, C.c_size_t]
        L.khh_tables_free.argtypes = [C.c_void_p]
        L.khh_tables_new_files.restype = C.c_void_p
        L.khh_tables_new_files.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_uint32, C.c_char_p, C.c_int, C.c_int,
                                           P(C.c_uint32), C.c_char_p, C.c_size_t]
        L.khh_tables_save.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_size_t]
        L.khh_tables_new_gpu.restype = C.c_void_p
        L.khh_tables_new_gpu.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_uint32, C.c_int, P(C.c_double), C.c_char_p,
                                         C.c_size_t]
        L.khh_tables_new_resident.restype = C.c_void_p
        L.khh_tables_new_resident.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_uint32,
                                              P(C.c_double), C.c_char_p, C.c_size_t]
        L.khh_tables_is_resident.argtypes = [C.c_void_p]
        L.khh_tables_set_resident_stages.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
        L.khh_resident_gate_log2.restype = C.c_uint32
        L.khh_resident_gate_log2.argtypes = [C.c_uint64, C.c_uint64]
        L.khh_resident_keeps_fold.argtypes = [C.c_uint64, C.c_uint32]
        L.khh_session_resident_info.argtypes = [C.c_void_p, P(C.c_uint64), C.c_uint32]
        L.khh_session_resident_bytes.argtypes = [C.c_void_p, C.c_uint32, C.c_int, P(C.c_uint64)]
        L.khh_session_resident_read.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_uint64, C.c_uint64, C.c_char_p]
        L.khh_session_resident_popcount.argtypes = [C.c_void_p, C.c_uint32, C.c_int, P(C.c_uint64)]
        L.khh_session_gate_probe.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p, C.c_char_p, C.c_uint32]
        L.khh_params.argtypes = [C.c_void_p, P(C.c_uint64)]
        L.khh_bloom.restype = P(C.c_uint8)
        L.khh_bloom.argtypes = [C.c_void_p, C.c_int, C.c_int, P(C.c_uint64), P(C.c_uint64), P(C.c_uint32)]
        L.khh_giant_table.argtypes = [C.c_void_p, C.c_char_p]
        L.khh_amp_table.argtypes = [C.c_void_p, C.c_int, C.c_char_p]
        L.khh_lane_offsets.restype = C.c_uint32
        L.khh_lane_offsets.argtypes = [C.c_void_p, C.c_char_p, P(C.c_uint32)]
        L.khh_bptable.restype = P(C.c_uint8)
        L.khh_bptable.argtypes = [C.c_void_p, P(C.c_uint64)]
        L.khh_gate.restype = C.c_void_p
        L.khh_gate.argtypes = [C.c_void_p, P(C.c_uint32)]
        L.khh_gate_probes.restype = C.c_uint32
        L.khh_gate_probes.argtypes = [C.c_void_p]
        L.khh_chunk_centre.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p]
        L.khh_job_centres.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, C.c_char_p, C.c_int]
        L.khh_secondcheck.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32, C.c_char_p, C.c_char_p]
        L.khh_search.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_char_p, C.c_char_p, P(C.c_int), C.c_int,
                                 C.c_uint32, C.c_uint32, C.c_uint64, P(C.c_int), C.c_char_p, P(C.c_uint64),
                                 C.c_char_p, C.c_size_t]
        L.khh_session_open.restype = C.c_void_p
        L.khh_session_open.argtypes = [C.c_void_p, P(C.c_int), C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_char_p,
                                       C.c_size_t]
        L.khh_session_run.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_char_p, C.c_char_p, C.c_uint64, C.c_int,
                                      P(C.c_int), C.c_char_p, P(C.c_uint64), C.c_char_p, C.c_size_t]
        L.khh_session_run_ex.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_char_p, C.c_char_p, C.c_uint64,
                                         C.c_int, P(C.c_int), C.c_char_p, P(C.c_uint64), C.c_uint32, C.c_char_p,
                                         C.c_size_t]
        L.khh_session_close.argtypes = [C.c_void_p]
        L.khh_session_set_test_hooks.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_char_p]
        L.khh_session_set_check_mode.argtypes = [C.c_void_p, C.c_int]
        L.khh_session_set_chunk_mode.argtypes = [C.c_void_p, C.c_int]
        L.khh_chunk_sequence.restype = C.c_uint64
        L.khh_chunk_sequence.argtypes = [C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint64, C.c_char_p,
                                         C.c_uint64]
        L.khh_gtable.argtypes = [C.c_char_p]
        L.khh_session_recorded.restype = C.c_uint64
        L.khh_session_recorded.argtypes = [C.c_void_p, C.c_char_p, P(C.c_uint32), P(C.c_uint32), C.c_uint64]
        L.khh_pubkey.argtypes = [C.c_char_p, C.c_char_p]
        L.khh_parse_pubkey.argtypes = [C.c_char_p, C.c_char_p, P(C.c_int)]
        L.khh_addr_new.restype = C.c_void_p
        L.khh_addr_new.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_uint64, C.c_uint32, C.c_int, C.c_char_p,
                                   C.c_size_t]
        L.khh_addr_new_eth.restype = C.c_void_p
        L.khh_addr_new_eth.argtypes = L.khh_addr_new.argtypes
        L.khh_addr_new_xpoint.restype = C.c_void_p
        L.khh_addr_new_xpoint.argtypes = L.khh_addr_new.argtypes
        L.khh_addr_new_vanity.restype = C.c_void_p
        L.khh_addr_new_vanity.argtypes = [C.c_char_p, C.c_char_p, C.c_uint64, C.c_uint32, C.c_int, C.c_char_p,
                                          C.c_size_t]
        L.khh_addr_vanity_intervals.restype = P(C.c_uint8)
        L.khh_addr_vanity_intervals.argtypes = [C.c_void_p, P(C.c_uint64)]
        L.khh_vanity_target_ok.argtypes = [C.c_char_p]
        L.khh_addr_vanity_match.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_uint64]
        L.khh_addr_counted.restype = C.c_uint64
        L.khh_addr_counted.argtypes = [C.c_void_p]
        L.khh_addr_free.argtypes = [C.c_void_p]
        L.khh_addr_skipped.restype = C.c_uint64
        L.khh_addr_skipped.argtypes = [C.c_void_p]
        L.khh_eth_address.argtypes = [C.c_char_p, C.c_char_p]
        L.khh_addr_table.restype = P(C.c_uint8)
        L.khh_addr_table.argtypes = [C.c_void_p, P(C.c_uint64)]
        L.khh_addr_bloom.restype = P(C.c_uint8)
        L.khh_addr_bloom.argtypes = [C.c_void_p, P(C.c_uint64), P(C.c_uint64), P(C.c_uint32)]
        L.khh_addr_giant_table.argtypes = [C.c_void_p, C.c_char_p]
        L.khh_addr_lane_offsets.restype = C.c_uint32
        L.khh_addr_lane_offsets.argtypes = [C.c_void_p, C.c_char_p, P(C.c_uint32)]
        L.khh_addr_search.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int, P(C.c_int), C.c_int,
                                      C.c_uint32, C.c_uint64, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32,
                                      P(C.c_uint32), P(C.c_uint64), C.c_char_p, C.c_size_t]
        L.khh_addr_search_ex.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int, P(C.c_int), C.c_int,
                                         C.c_uint32, C.c_uint64, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32,
                                         P(C.c_uint32), P(C.c_uint64), C.c_uint32, C.c_char_p, C.c_size_t]
        L.khh_addr_set_hit_capacity.argtypes = [C.c_void_p, C.c_uint32]
        L.khh_mini_new.restype = C.c_void_p
        L.khh_mini_new.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_uint32, C.c_int, C.c_char_p, C.c_size_t]
        L.khh_mini_free.argtypes = [C.c_void_p]
        L.khh_mini_table.restype = P(C.c_uint8)
        L.khh_mini_table.argtypes = [C.c_void_p, P(C.c_uint64), P(C.c_uint32)]
        L.khh_mini_string.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.c_char_p]
        L.khh_mini_valid.argtypes = [C.c_void_p, C.c_char_p]
        L.khh_mini_key.restype = None
        L.khh_mini_key.argtypes = [C.c_char_p, C.c_char_p]
        L.khh_mini_set_queue_capacity.argtypes = [C.c_void_p, C.c_uint32]
        L.khh_mini_set_hit_capacity.argtypes = [C.c_void_p, C.c_uint32]
        L.khh_mini_cpu_scan.restype = C.c_double
        L.khh_mini_cpu_scan.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.c_int, P(C.c_uint64), P(C.c_uint64)]
        L.khh_mini_search.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_uint64, P(C.c_int), C.c_int, C.c_uint32,
                                      C.c_uint64, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32, P(C.c_uint32),
                                      P(C.c_uint64), C.c_uint32, C.c_char_p, C.c_size_t]
        L.khh_kang_new.restype = C.c_void_p
        L.khh_kang_new.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64,
                                   C.c_char_p, C.c_size_t]
        L.khh_kang_free.argtypes = [C.c_void_p]
        L.khh_kang_params.argtypes = [C.c_void_p, P(C.c_uint32), P(C.c_uint64), P(C.c_uint32)]
        L.khh_kang_jumps.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
        L.khh_kang_make_herd.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_char_p, C.c_char_p]
        L.khh_kang_cpu_walk.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint32,
                                        P(C.c_uint32), C.c_char_p, C.c_char_p, C.c_uint64, P(C.c_uint64),
                                        P(C.c_uint64)]
        L.khh_kang_set_ring_capacity.argtypes = [C.c_void_p, C.c_uint32]
        L.khh_kang_plant.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_uint64]
        L.khh_kang_keep_herd.argtypes = [C.c_void_p, C.c_int]
        L.khh_kang_final_herd.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_uint64, P(C.c_uint64)]
        L.khh_kang_search.argtypes = [C.c_void_p, P(C.c_int), C.c_int, C.c_uint64, C.c_char_p, P(C.c_int),
                                      P(C.c_uint64), C.c_uint32, C.c_char_p, C.c_size_t]
        L.khh_addr_confirm.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32, C.c_char_p, C.POINTER(C.c_int)]
        L.khh_hash160.argtypes = [C.c_char_p, C.c_int, C.c_char_p]
        L.khh_rmd_to_address.argtypes = [C.c_char_p, C.c_char_p]
        _lib = L
    return _lib


def _b32(v: int) -> bytes:
    return int(v).to_bytes(32, "big")


def pubkey(k: int) -> bytes:
    out = C.create_string_buffer(64)
    if lib().khh_pubkey(_b32(k), out):
        raise KhhError("invalid private key")
    return out.raw


def parse_pubkey(s: str) -> tuple[bytes, bool] | None:
    out = C.create_string_buffer(64)
    comp = C.c_int(0)
    if lib().khh_parse_pubkey(s.encode(), out, C.byref(comp)):
        return None
    return out.raw, bool(comp.value)


class Tables:
    """keyhunt's BSGS tables built by the product host engine."""

    def __init__(self, n: str | None = None, k: int = 1, threads: int = 0, gpl: int = 4,
                 files_dir: str | None = None, save: bool = False, skip_checksum: bool = False,
                 gpu_device: int | None = None, resident: bool = False, gate_log2: int = 0,
                 stage1: int = 1, stage0: int = 0):
        """files_dir: -S semantics — read the reference's table files from that directory, compute
        only what is missing, and with save=True write the missing files back (self.have = mask).
        resident (with gpu_device): large -k tables, whose level-1 bloom and gate every Session builds on its
        devices and keeps there; gate_log2 0 = sized from the device's free memory, else an explicit size (log2
        bits, 13..38); stage1 / stage0 = the gate stages (khb_set_gate_stage1 / khb_set_gate_stage0 values)."""
        err = C.create_string_buffer(256)
        self.have = 0
        self.build_ms = 0.0
        self.resident = bool(resident)
        if resident:
            if gpu_device is None or files_dir is not None:
                raise KhhError("resident tables are built on a GPU (gpu_device=...), without table files")
            ms = C.c_double(0)
            self.h = lib().khh_tables_new_resident(n.encode() if n else None, k, threads, gpl, gpu_device, gate_log2,
                                                   C.byref(ms), err, 256)
            self.build_ms = ms.value
            if self.h and lib().khh_tables_set_resident_stages(self.h, stage1, stage0):
                lib().khh_tables_free(self.h)
                self.h = None
                raise KhhError("invalid gate stage sizes")
        elif gpu_device is not None:
            ms = C.c_double(0)
            self.h = lib().khh_tables_new_gpu(n.encode() if n else None, k, threads, gpl, gpu_device, C.byref(ms),
                                              err, 256)
            self.build_ms = ms.value
        elif files_dir is not None:
            have = C.c_uint32(0)
            self.h = lib().khh_tables_new_files(n.encode() if n else None, k, threads, gpl, files_dir.encode(),
                                                1 if skip_checksum else 0, 1 if save else 0, C.byref(have), err, 256)
            self.have = int(have.value)
        else:
            self.h = lib().khh_tables_new(n.encode() if n else None, k, threads, gpl, err, 256)
        if not self.h:
            raise KhhError(err.value.decode())
        p = (C.c_uint64 * 10)()
        lib().khh_params(self.h, p)
        (self.m, self.m2, self.m3, self.aux, self.cycles, self.n_low, self.l1ext, self.items1, self.items2,
         self.items3) = [int(v) for v in p]

    def close(self) -> None:
        if self.h:
            lib().khh_tables_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def save_files(self, directory: str) -> None:
        err = C.create_string_buffer(256)
        if lib().khh_tables_save(self.h, directory.encode(), err, 256):
            raise KhhError(err.value.decode())

    def bloom(self, level: int, idx: int) -> tuple[bytes, int, int]:
        nb, bits, h = C.c_uint64(), C.c_uint64(), C.c_uint32()
        p = lib().khh_bloom(self.h, level, idx, C.byref(nb), C.byref(bits), C.byref(h))
        if not p:
            raise KhhError("resident tables keep the level-1 bloom on the GPU (Session.resident_read)"
                           if level == 1 and self.resident else "no such bloom")
        return C.string_at(p, nb.value), int(bits.value), int(h.value)

    def l1_geometry(self) -> tuple[int, int, int]:
        """(bytes per sub-bloom, bits, hashes) of level 1; also on resident tables."""
        nb, bits, h = C.c_uint64(), C.c_uint64(), C.c_uint32()
        lib().khh_bloom(self.h, 1, 0, C.byref(nb), C.byref(bits), C.byref(h))
        return int(nb.value), int(bits.value), int(h.value)

    def bloom_concat(self, level: int = 1) -> tuple[bytes, int, int, int]:
        parts = [self.bloom(level, i)[0] for i in range(256)]
        _, bits, h = self.bloom(level, 0)
        return b"".join(parts), len(parts[0]), bits, h

    def giant_table(self) -> bytes:
        b = C.create_string_buffer(513 * 64)
        lib().khh_giant_table(self.h, b)
        return b.raw

    def amp_table(self, level: int) -> bytes:
        b = C.create_string_buffer(32 * 64)
        lib().khh_amp_table(self.h, level, b)
        return b.raw

    def lane_offsets(self) -> tuple[bytes, int]:
        g = C.c_uint32()
        n = lib().khh_lane_offsets(self.h, None, C.byref(g))
        b = C.create_string_buffer(64 * n)
        lib().khh_lane_offsets(self.h, b, C.byref(g))
        return b.raw, int(g.value)

    def gate_probes(self) -> int:
        """Bits per x of the level-0 gate (khb_load_gate's probes); 0 when there is no gate."""
        return int(lib().khh_gate_probes(self.h))

    def gate(self) -> tuple[bytes, int]:
        """The level-0 gate (khb_load_gate) and its log2 size; (b"", 0) when the tables have none."""
        if self.resident:
            raise KhhError("resident tables keep the gate on the GPU (Session.resident_read)")
        lg = C.c_uint32(0)
        p = lib().khh_gate(self.h, C.byref(lg))
        return (C.string_at(p, (1 << lg.value) // 8) if lg.value else b""), int(lg.value)

    def bptable(self) -> list[tuple[bytes, int]]:
        n = C.c_uint64()
        p = lib().khh_bptable(self.h, C.byref(n))
        raw = C.string_at(p, 16 * n.value)
        return [(raw[16 * i:16 * i + 6], int.from_bytes(raw[16 * i + 8:16 * i + 16], "little")) for i in range(n.value)]

    def bptable_raw(self) -> bytes:
        """bPtable as m3 x 16-byte struct bsgs_xvalue records (khb_check_tables.bptable)."""
        n = C.c_uint64()
        p = lib().khh_bptable(self.h, C.byref(n))
        return C.string_at(p, 16 * n.value)

    def check_tables(self) -> dict:
        """Everything khb_load_check_tables takes, from these tables (Engine.load_check_tables(**...))."""
        l2, nb2, bits2, h2 = self.bloom_concat(2)
        l3, nb3, bits3, h3 = self.bloom_concat(3)
        return {"gtable": gtable(), "amp2": self.amp_table(2), "amp3": self.amp_table(3),
                "l2": (l2, nb2, bits2, h2), "l3": (l3, nb3, bits3, h3), "bptable": self.bptable_raw(), "m3": self.m3,
                "m_double": 2 * self.m, "m2_double": 2 * self.m2, "m3_value": self.m3, "m3_double": 2 * self.m3}

    def chunk_centre(self, base: int, target_xy: bytes) -> bytes:
        out = C.create_string_buffer(64)
        lib().khh_chunk_centre(self.h, _b32(base), target_xy, out)
        return out.raw

    def job_centres(self, bases: list[int], targets_xy: list[bytes], threads: int = 8) -> bytes:
        """The engine's batched centres of every (chunk, target) job, chunk-major (khh_job_centres)."""
        out = C.create_string_buffer(64 * len(bases) * len(targets_xy))
        lib().khh_job_centres(self.h, b"".join(_b32(b) for b in bases), len(bases), b"".join(targets_xy),
                              len(targets_xy), out, threads)
        return out.raw

    def secondcheck(self, base: int, a: int, target_xy: bytes) -> int | None:
        key = C.create_string_buffer(32)
        if lib().khh_secondcheck(self.h, _b32(base), a, target_xy, key):
            return int.from_bytes(key.raw, "big")
        return None

    def search(self, targets_xy: list[bytes], start: int, end: int, devices=(0,), lanes: int = 0,
               chunks_per_batch: int = 0, max_chunks: int = 0):
        n = len(targets_xy)
        found = (C.c_int * n)()
        keys = C.create_string_buffer(32 * n)
        stats = (C.c_uint64 * 6)()
        devs = (C.c_int * len(devices))(*devices)
        err = C.create_string_buffer(256)
        rc = lib().khh_search(self.h, b"".join(targets_xy), n, _b32(start), _b32(end), devs, len(devices), lanes,
                              chunks_per_batch, max_chunks, found, keys, stats, err, 256)
        if rc:
            raise KhhError(f"search failed ({rc}): {err.value.decode()}")
        res = [int.from_bytes(keys.raw[32 * i:32 * i + 32], "big") if found[i] else None for i in range(n)]
        return res, {"chunks": stats[0], "giant_steps": stats[1], "candidates": stats[2], "degenerate": stats[3],
                     "kernel_s": stats[4] / 1e6, "launches": stats[5]}


_STAT_KEYS = ("chunks", "giant_steps", "candidates", "degenerate", "kernel_s", "launches", "rescans", "busy_s",
              "shader_mhz", "device_checked", "device_check_s", "event_s")
CHECK_HOST, CHECK_DEVICE, CHECK_AUTO = 0, 1, 2      # include/khhost.h KHH_CHECK_*
BSGS_MODES = ("sequential", "backward", "both", "random", "dance")     # keyhunt.cpp:227, -B


def chunk_sequence(mode: int, start: int, end: int, two_n: int, seed: int = 1, cap: int = 1 << 16) -> list[int]:
    """The chunk bases -B mode `mode` claims from [start, end) (khh_chunk_sequence; the engine's order)."""
    out = C.create_string_buffer(32 * cap)
    n = lib().khh_chunk_sequence(mode, _b32(start), _b32(end), _b32(two_n), seed, out, cap)
    return [int.from_bytes(out.raw[32 * i:32 * i + 32], "big") for i in range(n)]


def gtable() -> bytes:
    """Secp256K1::Init's GTable as 32*256 points x||y BE (khh_gtable; khb_check_tables.gtable)."""
    b = C.create_string_buffer(32 * 256 * 64)
    lib().khh_gtable(b)
    return b.raw


class Session:
    """Opened devices with the tables resident in HBM (khh_session_*)."""

    def __init__(self, tables: Tables, devices=(0,), lanes: int = 0, chunks_per_batch: int = 0,
                 check_threads: int = 0):
        self.tables = tables
        devs = (C.c_int * len(devices))(*devices)
        err = C.create_string_buffer(256)
        self.h = lib().khh_session_open(tables.h, devs, len(devices), lanes, chunks_per_batch, check_threads, err, 256)
        if not self.h:
            raise KhhError(err.value.decode())

    def close(self) -> None:
        if self.h:
            lib().khh_session_close(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def run(self, targets_xy: list[bytes], start: int, end: int, max_chunks: int = 0, random_chunks: bool = False):
        n = len(targets_xy)
        found = (C.c_int * n)()
        keys = C.create_string_buffer(32 * n)
        stats = (C.c_uint64 * KHH_SESSION_STATS)()
        err = C.create_string_buffer(256)
        rc = lib().khh_session_run_ex(self.h, b"".join(targets_xy), n, _b32(start), _b32(end), max_chunks,
                                      1 if random_chunks else 0, found, keys, stats, KHH_SESSION_STATS, err, 256)
        if rc:
            raise KhhError(f"search failed ({rc}): {err.value.decode()}")
        res = [int.from_bytes(keys.raw[32 * i:32 * i + 32], "big") if found[i] else None for i in range(n)]
        st = {k: int(stats[i]) for i, k in enumerate(_STAT_KEYS)}
        st["kernel_s"] = stats[4] / 1e6
        st["busy_s"] = stats[7] / 1e6
        st["shader_mhz"] = stats[8] / 1e3
        st["device_check_s"] = stats[10] / 1e6
        st["event_s"] = stats[11] / 1e6
        return res, st

    def set_chunk_mode(self, mode: int) -> None:
        """keyhunt's -B mode for later runs: BSGS_MODES.index(name) (0 sequential ... 4 dance)."""
        rc = lib().khh_session_set_chunk_mode(self.h, mode)
        if rc:
            raise KhhError(f"set_chunk_mode failed ({rc})")

    def set_check_mode(self, mode: int) -> None:
        """Where later runs confirm candidates: CHECK_HOST (CPU pool), CHECK_DEVICE (khb_check), CHECK_AUTO."""
        rc = lib().khh_session_set_check_mode(self.h, mode)
        if rc:
            raise KhhError(f"set_check_mode failed ({rc})")

    def set_test_hooks(self, cand_cap: int = 0, use_gate: bool = True, record: bool = False,
                       l1_concat: bytes | None = None) -> None:
        """Tests: candidate ring capacity (0 = default), gate on/off, candidate recording, replacement L1."""
        rc = lib().khh_session_set_test_hooks(self.h, cand_cap, 1 if use_gate else 0, 1 if record else 0, l1_concat)
        if rc:
            raise KhhError(f"set_test_hooks failed ({rc})")

    # ---- resident tables and the installed tables of any session (include/khbsgs.h KHB_TABLE_*) ----
    def resident_info(self) -> list[dict]:
        """Per device of a session on resident tables: what it built (khh_session_resident_info)."""
        n = lib().khh_session_resident_info(self.h, None, 0)
        out = (C.c_uint64 * (KHH_RESIDENT_INFO * max(1, n)))()
        lib().khh_session_resident_info(self.h, out, n)
        keys = ("l1_bytes", "gate_log2", "gate_probes", "fold_log2_bytes", "stage0_log2_bytes", "build_ms",
                "free_bytes", "total_bytes")
        res = []
        for i in range(n):
            d = {k: int(out[KHH_RESIDENT_INFO * i + j]) for j, k in enumerate(keys)}
            d["build_ms"] = d["build_ms"] / 1e3
            res.append(d)
        return res

    def _rc(self, rc: int, what: str) -> None:
        if rc:
            raise KhhError(f"{what} failed ({rc})")

    def resident_bytes(self, which: int, device_index: int = 0) -> int:
        n = C.c_uint64(0)
        self._rc(lib().khh_session_resident_bytes(self.h, device_index, which, C.byref(n)), "resident_bytes")
        return int(n.value)

    def resident_read(self, which: int, offset: int = 0, nbytes: int | None = None, device_index: int = 0) -> bytes:
        """A window of an installed table (TABLE_*) of one device; the whole table by default."""
        if nbytes is None:
            nbytes = self.resident_bytes(which, device_index) - offset
        out = C.create_string_buffer(max(1, nbytes))
        self._rc(lib().khh_session_resident_read(self.h, device_index, which, offset, nbytes, out), "resident_read")
        return out.raw[:nbytes]

    def resident_popcount(self, which: int, device_index: int = 0) -> int:
        n = C.c_uint64(0)
        self._rc(lib().khh_session_resident_popcount(self.h, device_index, which, C.byref(n)), "resident_popcount")
        return int(n.value)

    def gate_probe(self, xs: bytes, device_index: int = 0) -> bytes:
        """Per 32-byte BE x: bit 0 the full gate passes, bit 1 the stage-1 fold, bit 2 the stage-0 filter."""
        n = len(xs) // 32
        out = C.create_string_buffer(max(1, n))
        self._rc(lib().khh_session_gate_probe(self.h, device_index, xs, out, n), "gate_probe")
        return out.raw[:n]

    def recorded(self) -> list[tuple[int, int, int]]:
        """Level-1 candidates of the last run: (chunk base, target index, a)."""
        n = lib().khh_session_recorded(self.h, None, None, None, 0)
        bases = C.create_string_buffer(32 * max(1, n))
        tg = (C.c_uint32 * max(1, n))()
        a = (C.c_uint32 * max(1, n))()
        lib().khh_session_recorded(self.h, bases, tg, a, n)
        return [(int.from_bytes(bases.raw[32 * i:32 * i + 32], "big"), int(tg[i]), int(a[i])) for i in range(n)]


# ---- -m address / -m rmd160 ----
def hash160(xy: bytes, compressed: bool) -> bytes:
    out = C.create_string_buffer(20)
    lib().khh_hash160(xy, 1 if compressed else 0, out)
    return out.raw


def rmd_to_address(rmd: bytes) -> str:
    out = C.create_string_buffer(64)
    lib().khh_rmd_to_address(rmd, out)
    return out.value.decode()


def eth_address(xy: bytes) -> bytes:
    """ETH address of a public key x||y (64 bytes BE): bytes 12..31 of Keccak-256(x||y)."""
    if len(xy) != 64:
        raise ValueError("eth_address: 64 bytes x||y")
    out = C.create_string_buffer(20)
    lib().khh_eth_address(bytes(xy), out)
    return out.raw


def vanity_target_ok(s: str) -> bool:
    """Whether -m vanity accepts the target s: valid Base58, 1 to 29 characters, begins with '1', has an interval."""
    return bool(lib().khh_vanity_target_ok(s.encode()))


class Addr:
    """-m address targets (a target file's text) + generator for chunks of n_seq keys.  crypto="eth": the text is
    read as -c eth reads it (ETH addresses) and the handle is searched with KHB_SEARCH_ETH.  mode="xpoint": the text
    is read as -m xpoint reads it (x values and public keys) and the handle is searched with KHB_SEARCH_XPOINT.
    mode="vanity": the text holds one address prefix per line and the handle is searched with search 0, 1 or 2
    (optionally | 4) for every key whose address begins with one of them; a text without an accepted target is a
    ValueError."""

    def __init__(self, text: str, n_seq: int = 1 << 32, stride: int = 1, gpl: int = 16, bloom_multiplier: int = 1,
                 threads: int = 0, crypto: str = "btc", mode: str = "address"):
        if crypto not in ("btc", "eth"):
            raise ValueError("crypto: btc or eth")
        if mode not in ("address", "xpoint", "vanity"):
            raise ValueError("mode: address, xpoint or vanity")
        if mode != "address" and crypto == "eth":
            raise ValueError(f"mode {mode} has no crypto eth")
        err = C.create_string_buffer(256)
        if mode == "vanity":
            self.h = lib().khh_addr_new_vanity(text.encode(), _b32(stride), n_seq, gpl, threads, err, 256)
            # the binding's rule, by the library's own count: a vanity handle without an accepted target can only
            # be inspected in C, never searched, so the binding treats such a text as a bad argument
            if self.h and not lib().khh_addr_counted(self.h):
                lib().khh_addr_free(self.h)
                self.h = None
                raise ValueError("mode vanity: the text holds no target that is accepted (valid Base58, 1 to 29 "
                                 "characters, beginning with '1')")
        else:
            new = (lib().khh_addr_new_xpoint if mode == "xpoint"
                   else lib().khh_addr_new_eth if crypto == "eth" else lib().khh_addr_new)
            self.h = new(text.encode(), bloom_multiplier, _b32(stride), n_seq, gpl, threads, err, 256)
        if not self.h:
            raise KhhError(err.value.decode())
        self.n_seq, self.stride, self.crypto, self.mode = n_seq, stride, crypto, mode

    def skipped(self) -> int:
        """Lines the loader omitted as invalid."""
        return int(lib().khh_addr_skipped(self.h))

    def counted(self) -> int:
        """Lines the loader counted (they size the bloom)."""
        return int(lib().khh_addr_counted(self.h))

    def close(self) -> None:
        if self.h:
            lib().khh_addr_free(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def table(self) -> list[bytes]:
        n = C.c_uint64(0)
        p = lib().khh_addr_table(self.h, C.byref(n))
        raw = C.string_at(p, 20 * n.value) if n.value else b""
        return [raw[20 * i:20 * i + 20] for i in range(n.value)]

    def vanity_intervals(self) -> list[tuple[bytes, bytes]]:
        """mode="vanity": the merged table [(lo, hi)] of 20-byte big-endian bounds, ascending (khb_load_vanity's)."""
        n = C.c_uint64(0)
        p = lib().khh_addr_vanity_intervals(self.h, C.byref(n))
        raw = C.string_at(p, 40 * n.value) if n.value else b""
        return [(raw[40 * i:40 * i + 20], raw[40 * i + 20:40 * i + 40]) for i in range(n.value)]

    def vanity_match(self, h20: bytes) -> bytes:
        """mode="vanity": per 20-byte hash160, bit 0 = inside a merged interval (the device's report), bit 1 = its
        address begins with a target (the confirmation)."""
        n = len(h20) // 20
        out = C.create_string_buffer(n)
        if lib().khh_addr_vanity_match(self.h, bytes(h20), out, n):
            raise KhhError("khh_addr_vanity_match: not a vanity handle")
        return out.raw

    def bloom(self) -> tuple[bytes, int, int]:
        nb, bits, h = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
        p = lib().khh_addr_bloom(self.h, C.byref(nb), C.byref(bits), C.byref(h))
        return C.string_at(p, nb.value), int(bits.value), int(h.value)

    def giant_table(self) -> bytes:
        out = C.create_string_buffer(513 * 64)
        lib().khh_addr_giant_table(self.h, out)
        return out.raw

    def lane_offsets(self) -> tuple[bytes, int]:
        g = C.c_uint32(0)
        n = lib().khh_addr_lane_offsets(self.h, None, C.byref(g))
        out = C.create_string_buffer(64 * n)
        lib().khh_addr_lane_offsets(self.h, out, C.byref(g))
        return out.raw, int(g.value)

    def set_hit_capacity(self, cap: int) -> None:
        """Tests: the launches' bloom-hit ring capacity (0 = default 2^18); overflow -> rescan in parts."""
        if lib().khh_addr_set_hit_capacity(self.h, cap):
            raise KhhError("khh_addr_set_hit_capacity")

    def confirm(self, key: int, kind: int):
        """khh_addr_confirm: (key, compressed) recovered from a bloom hit of kind `kind` on the point of `key`, or
        None when its hash is not a target."""
        out = C.create_string_buffer(32)
        comp = C.c_int(0)
        r = lib().khh_addr_confirm(self.h, _b32(key), kind, out, C.byref(comp))
        if r < 0:
            raise KhhError(f"khh_addr_confirm [{r}]")
        return (int.from_bytes(out.raw, "big"), bool(comp.value)) if r == 1 else None

    def search(self, start: int, end: int, search: int = 2, devices=(0,), lanes: int = 0, max_chunks: int = 0,
               random_chunks: bool = False, cap: int = 4096):
        """Found [(key, compressed, rmd160)] in discovery order, plus stats.  search | 4 (KHB_SEARCH_ENDOMORPHISM)
        is -e; search = 8 (KHB_SEARCH_ETH) on a crypto="eth" handle gives (key, False, address); search = 16
        (KHB_SEARCH_XPOINT), alone or | 4, on a mode="xpoint" handle gives (key, False, first 20 bytes of x); search
        0/1/2, optionally | 4, on a mode="vanity" handle gives every key whose address begins with a target."""
        keys = C.create_string_buffer(32 * cap)
        comp = C.create_string_buffer(cap)
        rmd = C.create_string_buffer(20 * cap)
        nf = C.c_uint32(0)
        st = (C.c_uint64 * KHH_ADDR_STATS)()
        devs = (C.c_int * len(devices))(*devices)
        err = C.create_string_buffer(256)
        rc = lib().khh_addr_search_ex(self.h, _b32(start), _b32(end), search, 1 if random_chunks else 0, devs,
                                      len(devices), lanes, max_chunks, keys, comp, rmd, cap, C.byref(nf), st,
                                      KHH_ADDR_STATS, err, 256)
        if rc:
            raise KhhError(f"khh_addr_search: {err.value.decode()} [{rc}]")
        n = min(nf.value, cap)
        kb, cb, rb = keys.raw, comp.raw, rmd.raw     # one copy each: .raw copies the whole buffer
        found = [(int.from_bytes(kb[32 * i:32 * i + 32], "big"), bool(cb[i]), rb[20 * i:20 * i + 20]) for i in range(n)]
        return found, {"chunks": st[0], "keys": st[1], "hits": st[2], "degenerate": st[3], "kernel_s": st[4] / 1e6,
                       "launches": st[5], "shader_mhz": st[6] / 1e3, "rescans": st[7]}


class Minikeys:
    """-m minikeys: targets (a target file's text, read as -m address reads it) and the window table of the device's
    k*G.  A minikey is 'S' and 21 characters of `alphabet` (58 distinct characters; the reference's by default); a
    search examines `count` consecutive candidates from `first`, each exactly once, `first` included."""

    def __init__(self, text: str, alphabet: str | bytes | None = None, window_bits: int = 16,
                 bloom_multiplier: int = 1, threads: int = 0):
        if window_bits not in (4, 8, 16):
            raise ValueError("window_bits: 4, 8 or 16")
        a = alphabet.encode("latin-1") if isinstance(alphabet, str) else alphabet
        if a is not None and (len(a) != 58 or len(set(a)) != 58 or 0 in a):
            raise ValueError("alphabet: 58 distinct non-zero characters")
        self.alphabet = bytes(a) if a is not None else MINI_ALPHABET.encode()
        err = C.create_string_buffer(256)
        self.h = lib().khh_mini_new(text.encode(), bloom_multiplier, a, window_bits, threads, err, 256)
        if not self.h:
            raise KhhError(err.value.decode())
        self.window_bits = window_bits

    def close(self) -> None:
        if self.h:
            lib().khh_mini_free(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _mk(self, s: str | bytes) -> bytes:
        b = s.encode("latin-1") if isinstance(s, str) else bytes(s)
        if len(b) != 22 or b[:1] != b"S" or any(c not in self.alphabet for c in b[1:]):
            raise ValueError("a minikey is 'S' and 21 characters of the alphabet")
        return b

    def digits(self, s: str | bytes) -> bytes:
        """The 21 digit values of a minikey (what khbsgs.Engine.mini_scan takes)."""
        return bytes(self.alphabet.index(c) for c in self._mk(s)[1:])

    def table_points(self) -> bytes:
        """The window table khb_load_mini_table takes: d * 2^(w j) * G, 64 bytes x||y each."""
        n, w = C.c_uint64(0), C.c_uint32(0)
        p = lib().khh_mini_table(self.h, C.byref(n), C.byref(w))
        return C.string_at(p, 64 * n.value)

    def string(self, first: str | bytes, offset: int) -> str:
        """The minikey `offset` candidates after `first`; ValueError past 58^21 - 1."""
        out = C.create_string_buffer(22)
        if offset < 0 or offset >= 1 << 64 or lib().khh_mini_string(self.h, self._mk(first), offset, out):
            raise ValueError("offset out of range")
        return out.raw.decode("latin-1")

    def valid(self, minikey: str | bytes) -> bool:
        r = lib().khh_mini_valid(self.h, self._mk(minikey))
        if r < 0:
            raise ValueError("not a minikey of this alphabet")
        return bool(r)

    def key(self, minikey: str | bytes) -> int:
        out = C.create_string_buffer(32)
        lib().khh_mini_key(self._mk(minikey), out)
        return int.from_bytes(out.raw, "big")

    def set_queue_capacity(self, cap: int) -> None:
        """Tests: the launches' survivor-queue capacity (0 = sized from the launch); overflow -> rescan in halves."""
        if lib().khh_mini_set_queue_capacity(self.h, cap):
            raise KhhError("khh_mini_set_queue_capacity")

    def set_hit_capacity(self, cap: int) -> None:
        """Tests: the launches' bloom-hit ring capacity (0 = default 2^18); overflow -> rescan in halves."""
        if lib().khh_mini_set_hit_capacity(self.h, cap):
            raise KhhError("khh_mini_set_hit_capacity")

    def cpu_scan(self, first: str | bytes, count: int, threads: int = 16) -> tuple[float, int, int]:
        """The reference's loop on the CPU over the same span (a measurement's baseline): (seconds, valid, found)."""
        v, f = C.c_uint64(0), C.c_uint64(0)
        dt = lib().khh_mini_cpu_scan(self.h, self._mk(first), count, threads, C.byref(v), C.byref(f))
        if dt < 0:
            raise ValueError("cpu_scan: bad span")
        return float(dt), int(v.value), int(f.value)

    def search(self, first: str | bytes, count: int, devices=(0,), lanes: int = 0, per_launch: int = 0,
               cap: int = 4096):
        """Found [(minikey, key, rmd160)] in the order the launches report them (ascending within a launch) and
        stats.  A bad `first` or first + count > 58^21 is a ValueError."""
        fb = self._mk(first)
        if count < 1 or count >= 1 << 64:
            raise ValueError("count: 1 to 2^64 - 1")
        mk = C.create_string_buffer(22 * cap)
        keys = C.create_string_buffer(32 * cap)
        rmd = C.create_string_buffer(20 * cap)
        nf = C.c_uint32(0)
        st = (C.c_uint64 * KHH_MINI_STATS)()
        devs = (C.c_int * len(devices))(*devices)
        err = C.create_string_buffer(256)
        rc = lib().khh_mini_search(self.h, fb, len(fb), count, devs, len(devices), lanes, per_launch, mk, keys, rmd,
                                   cap, C.byref(nf), st, KHH_MINI_STATS, err, 256)
        if rc == -1:                    # KHB_EINVAL
            raise ValueError(f"khh_mini_search: {err.value.decode()}")
        if rc:
            raise KhhError(f"khh_mini_search: {err.value.decode()} [{rc}]")
        n = min(nf.value, cap)
        mb, kb, rb = mk.raw, keys.raw, rmd.raw
        found = [(mb[22 * i:22 * i + 22].decode("latin-1"), int.from_bytes(kb[32 * i:32 * i + 32], "big"),
                  rb[20 * i:20 * i + 20]) for i in range(n)]
        return found, {"candidates": st[0], "valid": st[1], "bad_keys": st[2], "hits": st[3], "launches": st[4],
                       "rescans": st[5], "filter_s": st[6] / 1e6, "keys_s": st[7] / 1e6}


def _herd_bytes(herd) -> tuple[bytes, bytes]:
    return (b"".join(_b32(x) + _b32(y) for x, y, _ in herd), b"".join(_b32(d) for _, _, d in herd))


def _herd_list(xy: bytes, d: bytes, n: int) -> list[tuple[int, int, int]]:
    f = int.from_bytes
    return [(f(xy[64 * i:64 * i + 32], "big"), f(xy[64 * i + 32:64 * i + 64], "big"), f(d[32 * i:32 * i + 32], "big"))
            for i in range(n)]


class Kangaroo:
    """Pollard's kangaroo interval search with distinguished points for one public key: the key of `pub` (x||y, 64
    bytes) is sought in [start, end), 2^16 <= end - start <= 2^200.  Kangaroo i is tame for even i (its point is d*G)
    and wild for odd i (Q + d*G, Q = P - start*G); a herd is a list of (x, y, d).  dp_bits and herd (kangaroos per
    device) default to the largest with herd * 2^dp_bits <= 2^(w // 2 - 2), w the bit length of the width."""

    def __init__(self, pub: bytes, start: int, end: int, dp_bits: int | None = None, herd: int | None = None,
                 seed: int = 0):
        err = C.create_string_buffer(256)
        if not (0 <= start < 1 << 256 and 0 <= end < 1 << 256):
            raise ValueError("the interval is start < end <= n")
        self.h = lib().khh_kang_new(bytes(pub), _b32(start), _b32(end), -1 if dp_bits is None else dp_bits,
                                    herd or 0, seed & ((1 << 64) - 1), 0, err, 256)
        if not self.h:
            raise ValueError(f"khh_kang_new: {err.value.decode()}")
        dp, hd, w = C.c_uint32(0), C.c_uint64(0), C.c_uint32(0)
        lib().khh_kang_params(self.h, C.byref(dp), C.byref(hd), C.byref(w))
        self.dp_bits, self.herd, self.width_bits = dp.value, hd.value, w.value
        self.start, self.end = start, end
        self._eng = None
        self._ring = 0

    def close(self) -> None:
        if getattr(self, "_eng", None) is not None:
            self._eng.close()
            self._eng = None
        if getattr(self, "h", None):
            lib().khh_kang_free(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def jump_table(self) -> list[tuple[int, tuple[int, int]]]:
        """The 32 jumps [(s_j, (x, y))] with (x, y) = s_j * G."""
        d, xy = C.create_string_buffer(32 * 32), C.create_string_buffer(64 * 32)
        lib().khh_kang_jumps(self.h, d, xy)
        return [(s, (x, y)) for x, y, s in _herd_list(xy.raw, d.raw, 32)]

    def make_herd(self, n: int | None = None, stream: int = 0) -> list[tuple[int, int, int]]:
        """The first n kangaroos a search gives its device number `stream` (the whole herd by default)."""
        n = self.herd if n is None else n
        xy, d = C.create_string_buffer(64 * n), C.create_string_buffer(32 * n)
        if lib().khh_kang_make_herd(self.h, stream, n, xy, d):
            raise KhhError("khh_kang_make_herd")
        return _herd_list(xy.raw, d.raw, n)

    def cpu_walk(self, herd, steps: int, dp_bits: int | None = None):
        """The step rule on the CPU (khh_kang_cpu_walk): (the herd after `steps` jumps each, the distinguished
        points [(kangaroo, x, d)] in the order they are met, the number of second choices)."""
        n = len(herd)
        dp = self.dp_bits if dp_bits is None else dp_bits
        xyb, db = _herd_bytes(herd)
        xy, d = C.create_string_buffer(xyb, 64 * n), C.create_string_buffer(db, 32 * n)
        cap = n * steps
        idx = (C.c_uint32 * cap)()
        px, pd = C.create_string_buffer(32 * cap), C.create_string_buffer(32 * cap)
        ndp, sec = C.c_uint64(0), C.c_uint64(0)
        if lib().khh_kang_cpu_walk(self.h, xy, d, n, steps, dp, idx, px, pd, cap, C.byref(ndp), C.byref(sec)):
            raise ValueError("khh_kang_cpu_walk: a herd, steps >= 1 and dp_bits <= 32")
        f = int.from_bytes
        dps = [(idx[i], f(px.raw[32 * i:32 * i + 32], "big"), f(pd.raw[32 * i:32 * i + 32], "big"))
               for i in range(ndp.value)]
        return _herd_list(xy.raw, d.raw, n), dps, sec.value

    # ---- the raw launch on one device (libkhbsgs through khbsgs.Engine) ----
    def engine(self, device: int = 0):
        """The device context of load_herd / read_herd / walk, opened on first use with the jump table loaded."""
        if self._eng is None:
            from .khbsgs import Engine
            self._eng = Engine(device)
            self._eng.kang_load_jumps(self.jump_table())
            if self._ring:
                self._eng.kang_set_ring_capacity(self._ring)
        return self._eng

    def load_herd(self, herd=None, device: int = 0) -> None:
        """Replace the device's herd by [(x, y, d)] (make_herd() by default)."""
        e = self.engine(device)
        e.kang_store([], 0)
        e.kang_store(self.make_herd() if herd is None else herd, 0)

    def read_herd(self) -> list[tuple[int, int, int]]:
        return self.engine().kang_read()

    def walk(self, steps: int, dp_bits: int | None = None):
        """One launch of `steps` jumps per kangaroo: ([(kangaroo, x, d)] unordered, stats dict)."""
        dps, st = self.engine().kang_walk(steps, self.dp_bits if dp_bits is None else dp_bits)
        return dps, {"steps_walked": st.steps_walked, "n_dp": st.n_dp, "second_choice": st.second_choice,
                     "dp_overflow": st.dp_overflow, "kernel_ms": st.kernel_ms}

    def set_ring_capacity(self, cap: int) -> None:
        """Ring entries per launch, of walk() and of search() (0 = the search's own sizing; walk keeps its last)."""
        lib().khh_kang_set_ring_capacity(self.h, cap)
        self._ring = cap
        if cap and self._eng is not None:
            self._eng.kang_set_ring_capacity(cap)

    # ---- test hooks of the search ----
    def plant(self, herd) -> None:
        """The first kangaroos of the first device's herd in the next searches."""
        xy, d = _herd_bytes(herd)
        if lib().khh_kang_plant(self.h, xy, d, len(herd)):
            raise ValueError("plant: more kangaroos than the herd")

    def keep_herd(self, keep: bool = True) -> None:
        lib().khh_kang_keep_herd(self.h, int(keep))

    def final_herd(self) -> list[tuple[int, int, int]]:
        n = C.c_uint64(0)
        lib().khh_kang_final_herd(self.h, None, None, 0, C.byref(n))
        xy, d = C.create_string_buffer(64 * n.value), C.create_string_buffer(32 * n.value)
        lib().khh_kang_final_herd(self.h, xy, d, n.value, C.byref(n))
        return _herd_list(xy.raw, d.raw, n.value)

    def search(self, devices=(0,), max_steps: int = 0) -> dict:
        """{key | None, steps, dps, dead, lost_dps, launches, seconds}.  One herd per entry of `devices`; an empty
        `devices` walks one herd on the CPU (cpu_walk's code).  max_steps: jumps in all, 0 = until found."""
        devs = (C.c_int * max(len(devices), 1))(*devices)
        key, found = C.create_string_buffer(32), C.c_int(0)
        st = (C.c_uint64 * KHH_KANG_STATS)()
        err = C.create_string_buffer(256)
        rc = lib().khh_kang_search(self.h, devs, len(devices), max_steps, key, C.byref(found), st, KHH_KANG_STATS,
                                   err, 256)
        if rc:
            raise KhhError(f"khh_kang_search: {err.value.decode()} [{rc}]")
        return {"key": int.from_bytes(key.raw, "big") if found.value else None, "steps": st[0], "dps": st[1],
                "dead": st[2], "lost_dps": st[3], "launches": st[4], "seconds": st[5] / 1e6}


def resident_gate_log2(l1ext: int, budget_bytes: int) -> int:
    """The gate policy of resident builds (Tables::resident_gate_log2): log2 bits, 0 = no gate."""
    return int(lib().khh_resident_gate_log2(l1ext, budget_bytes))


def resident_keeps_fold(l1ext: int, gate_log2: int) -> bool:
    """Whether a resident build's AUTO stage-1 setting keeps the fold (Tables::resident_keeps_fold)."""
    return bool(lib().khh_resident_keeps_fold(l1ext, gate_log2))
