"""GPU: the resident level-1 bloom and gate of large -k (khb_build_l1_resident; khhost.Tables(resident=True)).

The level-1 bloom and its gate are built on each device in the layout the probe reads and never exist on the
host, so everything here is checked through the inspection calls (resident_read, resident_popcount, gate_probe)
against the host build of the same geometry, against the gate's definition restated in Python (helpers.gate_bits)
and against the oracle's candidate stream.
"""
from __future__ import annotations

import os
import random
import socket
import subprocess
import time

import numpy as np
import pytest

from keyhuntm1cpu_amd import BIN_DIR, khhost
from keyhuntm1cpu_amd.khbsgs import Engine
from keyhuntm1cpu_amd.khhost import TABLE_FOLD, TABLE_GATE, TABLE_L1, TABLE_STAGE0
from tests.helpers import _fold, _popcount, _stage0, gate_bits

pytestmark = pytest.mark.gpu
LANES = 64 * 256
P63 = "0365ec2994b8cc0a20d40dd69edfe55ca32a54bcbbaa6b0ddcff36049301a54579"
P125 = "0233709eb11e0d4439a729f21c2c443dedb727528229713f0065721ba8fa46f00e"
GIB = 1 << 30


# ---------------------------------------------------------------------------------- 1. byte parity
@pytest.mark.parametrize("n,k,probes,stage0", [("0x40000000", 33, 3, 0), (None, 1, 3, 0), ("0x40000000", 33, 1, 0),
                                               ("0x40000000", 33, 3, 20), (None, 1, 3, 20)])
def test_packed_build_byte_parity(monkeypatch, n, k, probes, stage0):
    """The resident build writes the bytes the host build has: L1 in the probe's packed layout (sub-blooms of an odd
    byte count, so words straddle them; l1ext > m for k = 33, the quirk-vi overshoot), the gate, its stage-1 fold,
    the stage-0 filter, and with one probe the gate khb_load_gate keeps on the device (every hi word set)."""
    monkeypatch.setenv("KHB_GATE_PROBES", str(probes))
    host = khhost.Tables(n, k, threads=16, gpu_device=0)
    gate, lg = host.gate()
    assert lg and host.gate_probes() == probes
    res = khhost.Tables(n, k, threads=16, gpu_device=0, resident=True, gate_log2=lg, stage0=stage0)
    try:
        l1, nb, bits, hashes = host.bloom_concat(1)
        assert res.l1_geometry() == (nb, bits, hashes)
        if k == 33:
            assert host.l1ext == 2129920 > host.m and nb % 4 != 0
        if probes == 1:        # the device image of a one-probe gate (include/khbsgs.h KHB_TABLE_GATE)
            g = np.frombuffer(gate, dtype="<u4").copy()
            g[1::2] = 0xFFFFFFFF
            gate = g.tobytes()
        with khhost.Session(res, devices=[0], lanes=LANES) as s:
            info = s.resident_info()
            assert len(info) == 1 and info[0]["l1_bytes"] == len(l1) and info[0]["gate_log2"] == lg
            assert info[0]["gate_probes"] == probes and info[0]["build_ms"] > 0
            assert s.resident_read(TABLE_L1) == l1
            assert s.resident_read(TABLE_GATE) == gate
            f_log2 = info[0]["fold_log2_bytes"]
            assert f_log2 == 21                       # KHB_GATE_STAGE1_AUTO for a 32 MiB gate
            fold = _fold(gate, f_log2)
            assert s.resident_read(TABLE_FOLD) == fold
            assert s.resident_popcount(TABLE_L1) == _popcount(l1)
            assert s.resident_popcount(TABLE_GATE) == _popcount(gate)
            assert s.resident_popcount(TABLE_FOLD) == _popcount(fold)
            if stage0:
                assert info[0]["stage0_log2_bytes"] == stage0
                z = _stage0(gate, stage0)
                assert s.resident_read(TABLE_STAGE0) == z
                assert s.resident_popcount(TABLE_STAGE0) == _popcount(z)
            else:
                assert info[0]["stage0_log2_bytes"] == 0
            # a window that is neither word- nor sub-bloom-aligned
            assert s.resident_read(TABLE_L1, nb - 5, 4099) == l1[nb - 5:nb - 5 + 4099]
    finally:
        res.close()
        host.close()


# ---------------------------------------------------------------------------------- 2. wide gates
@pytest.fixture(scope="module")
def small_xs(ora):
    """x of every baby step of -n 0x40000000 -k 1 (m = l1ext = 32,768), from the oracle."""
    return [ora.pubkey(ic + 1).xy()[0] for ic in range(32768)]


def _window(bits: set[int], byte0: int, nbytes: int) -> bytes:
    out = bytearray(nbytes)
    for b in bits:
        if byte0 <= b >> 3 < byte0 + nbytes:
            out[(b >> 3) - byte0] |= 1 << (b & 7)
    return bytes(out)


@pytest.mark.parametrize("lg", [33, 36, 38])
def test_wide_gate(small_xs, lg):
    """Gates past 2^32 bits, each the first size past a limit: 33 (bit counts beyond 32 bits), 36 (byte offsets
    >= 2^32), 38 (word index 2 * blk >= 2^32 with a block mask of all ones).  The popcount equals the number of
    distinct expected bits, which an index that wraps cannot give."""
    if lg == 38:
        with Engine(0, lanes=LANES) as e:
            free = e.mem_info()[0]
        if free < 40 * GIB:
            pytest.skip(f"the 2^38-bit gate is 32 GiB and the device reports {free / GIB:.1f} GiB free (< 40 GiB)")
    probes = 3
    expected = set()
    for x in small_xs:
        expected.update(gate_bits(lg, probes, x))
    res = khhost.Tables("0x40000000", 1, threads=16, gpu_device=0, resident=True, gate_log2=lg)
    try:
        assert res.m == res.l1ext == 32768
        with khhost.Session(res, devices=[0], lanes=LANES) as s:
            info = s.resident_info()[0]
            assert info["gate_log2"] == lg and info["gate_probes"] == probes
            assert s.resident_bytes(TABLE_GATE) == 1 << (lg - 3)
            assert s.resident_popcount(TABLE_GATE) == len(expected)
            got = s.gate_probe(b"".join(x.to_bytes(32, "big") for x in small_xs))
            assert all(v & 1 for v in got) and all(v & 2 for v in got)      # members pass the gate and its fold
            rng = random.Random(lg)
            others = [rng.randrange(1, 1 << 256) for _ in range(4096)]
            got = s.gate_probe(b"".join(x.to_bytes(32, "big") for x in others))
            want = [all(b in expected for b in gate_bits(lg, probes, x)) for x in others]
            assert [bool(v & 1) for v in got] == want
            # the fold of the expected set: block j of the gate lands in block j mod 2^(fold - 3)
            nb1 = 1 << (info["fold_log2_bytes"] - 3)
            folded = {64 * ((b >> 6) % nb1) + (b & 63) for b in expected}
            f_lg = info["fold_log2_bytes"] + 3
            want1 = [all(b in folded for b in gate_bits(f_lg, probes, x)) for x in others]
            assert [bool(v & 2) for v in got] == want1
            assert s.resident_popcount(TABLE_FOLD) == len(folded)
            for b in (min(expected), max(expected)):
                byte0 = (b >> 3) & ~63
                assert s.resident_read(TABLE_GATE, byte0, 64) == _window(expected, byte0, 64)
            key = 0x2000000000000000 + 5 * 2 * res.n_low + 0x1234567
            found, st = s.run([khhost.pubkey(key)], 0x2000000000000000, 0x2000000000000000 + 16 * 2 * res.n_low)
            assert found == [key]
    finally:
        res.close()


# ---------------------------------------------------------------------------------- 3. scan parity at k > 4
K8 = ("0x1000000000", 8)      # m = 2^21, 32 groups per chunk
BASES = [0x7CCE5E0000000000, (1 << 62) + (5 << 45)]
KEY = BASES[0] + 0x12345678AB           # in the chunk at BASES[0] (2N = 2^37 keys)


@pytest.fixture(scope="module")
def ora_k8(ora):
    o = ora.Bsgs(K8[0], K8[1], 16)
    yield o
    o.close()


@pytest.fixture(scope="module")
def oracle_stream(ora, ora_k8):
    """The oracle's level-1 candidates of the two chunks, computed once: {(base, a)}."""
    tgt = ora.pubkey(KEY)
    out = set()
    for b in BASES:
        ref, _, _ = ora_k8.scan(ora_k8.chunk_start(b, tgt), 0, ora_k8.cycles)
        out.update((b, a) for a in ref)
    return out


def _chunk_xs(e: Engine, res: khhost.Tables, target_xy: bytes) -> dict[int, bytes]:
    """x of every giant step of the two chunks, from the GPU dump (one call per chunk: at k = 8 the level-1
    sub-blooms, sized for 1,000 entries, hold 8,192, so nearly every step is an oracle candidate)."""
    return {b: e.dump_x(res.chunk_centre(b, target_xy), 0, res.cycles) for b in BASES}


@pytest.mark.parametrize("gate_log2", [0, 33])
def test_scan_parity_k8(ora, ora_k8, oracle_stream, gate_log2):
    """k = 8 through a resident session, candidates recorded over two chunks (one holds the key): they are the
    oracle's level-1 candidates whose x passes gate_probe; with the gate dropped, the oracle's stream exactly.  The
    key comes back through the host check and through the device check."""
    tgt = khhost.pubkey(KEY)
    res = khhost.Tables(K8[0], K8[1], threads=16, gpu_device=0, resident=True, gate_log2=gate_log2)
    try:
        assert res.m == 1 << 21 and res.cycles == 32 == ora_k8.cycles
        two_n = 2 * res.n_low
        offs, gpl = res.lane_offsets()
        with khhost.Session(res, devices=[0], lanes=LANES) as s, Engine(0, lanes=LANES) as e:
            e.load_giant_table(res.giant_table())
            e.load_lane_offsets(offs, gpl)
            info = s.resident_info()[0]
            assert info["gate_log2"] == (gate_log2 or 27)      # the policy: 64 bits per x for l1ext = 2^21
            s.set_test_hooks(record=True)
            by_mode = {}
            for mode in (khhost.CHECK_HOST, khhost.CHECK_DEVICE):
                s.set_check_mode(mode)
                rec = set()
                for b in BASES:
                    found, st = s.run([tgt], b, b + two_n)
                    assert st["chunks"] == 1 and st["giant_steps"] == 32 * 1024
                    assert found == ([KEY] if b == BASES[0] else [None])
                    rec.update((base, a) for base, _, a in s.recorded())
                by_mode[mode] = rec
            assert by_mode[khhost.CHECK_HOST] == by_mode[khhost.CHECK_DEVICE]
            assert len(oracle_stream) > 50000          # the saturated level-1 bloom of k = 8 passes most steps
            xs = _chunk_xs(e, res, tgt)
            order = sorted(oracle_stream)
            passed = s.gate_probe(b"".join(xs[b][32 * a:32 * a + 32] for b, a in order))
            assert rec == {p for p, v in zip(order, passed) if v & 1}
            assert any(b == BASES[0] and res.secondcheck(b, a, tgt) == KEY for b, a in rec)
            # the gate off: the reference's exact stream; and it cannot come back (it exists on the device only)
            s.set_test_hooks(use_gate=False, record=True)
            rec = set()
            for b in BASES:
                found, _ = s.run([tgt], b, b + two_n)
                rec.update((base, a) for base, _, a in s.recorded())
            assert rec == oracle_stream
            with pytest.raises(khhost.KhhError):
                s.set_test_hooks(use_gate=True)
    finally:
        res.close()


# ---------------------------------------------------------------------------------- 4. two contexts
def test_two_contexts_build_their_own_tables():
    res = khhost.Tables(K8[0], K8[1], threads=16, gpu_device=0, resident=True)
    try:
        two_n = 2 * res.n_low
        lo = 1 << 56
        k1, k2 = lo + 3 * two_n + 0x1234567, lo + 41 * two_n + 0x89ABCDE
        with khhost.Session(res, devices=[0, 0], lanes=LANES, chunks_per_batch=4) as s:
            info = s.resident_info()
            assert len(info) == 2
            assert all(info[0][f] == info[1][f] for f in ("l1_bytes", "gate_log2", "gate_probes", "fold_log2_bytes"))
            assert s.resident_popcount(TABLE_L1, 0) == s.resident_popcount(TABLE_L1, 1) > 0
            assert s.resident_popcount(TABLE_GATE, 0) == s.resident_popcount(TABLE_GATE, 1) > 0
            found, st = s.run([khhost.pubkey(k1), khhost.pubkey(k2)], lo, lo + 64 * two_n)
        assert found == [k1, k2]
        assert st["launches"] >= 2
    finally:
        res.close()


# ---------------------------------------------------------------------------------- 5. refusals
def test_resident_tables_refuse_what_is_not_on_the_host(tmp_path):
    res = khhost.Tables("0x40000000", 1, threads=16, gpu_device=0, resident=True)
    try:
        with pytest.raises(khhost.KhhError):
            res.bloom(1, 0)
        with pytest.raises(khhost.KhhError):
            res.gate()
        with pytest.raises(khhost.KhhError):
            res.save_files(str(tmp_path))
        assert not list(tmp_path.iterdir())
        assert len(res.bloom(2, 0)[0]) > 0          # the host levels are there
    finally:
        res.close()


def _cli(args, cwd):
    exe = os.path.join(BIN_DIR, "keyhunt_amd")
    return subprocess.run([exe] + args, cwd=cwd, capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("other", ["-S", "--cpu-build"])
def test_cli_refuses_resident_with(tmp_path, other):
    (tmp_path / "63.pub").write_text(P63 + "\n")
    r = _cli(["-m", "bsgs", "-f", "63.pub", "-r", "7cce500000000000:7cce600000000000", "-n", "0x1000000000", "-k", "8",
              "--resident", other, "-q", "-s", "0"], tmp_path)
    assert r.returncode == 1
    assert "--resident" in r.stderr and other in r.stderr
    assert not [p for p in tmp_path.iterdir() if p.name != "63.pub"]


# ---------------------------------------------------------------------------------- 6. CLI
def test_cli_resident_puzzle63(tmp_path):
    (tmp_path / "63.pub").write_text(P63 + "\n")
    r = _cli(["-m", "bsgs", "-f", "63.pub", "-r", "7cce500000000000:7cce600000000000", "-n", "0x1000000000", "-k", "8",
              "--resident", "-q", "-s", "0"], tmp_path)
    assert r.returncode == 1, r.stdout + r.stderr          # keyhunt exits 1 after "All points were found"
    assert "[+] Thread Key found privkey 7cce5efdaccf6808" in r.stdout
    assert "[+] GPU 0 resident: L1 bloom " in r.stdout and "gate 2^27 bits" in r.stdout and ", build " in r.stdout
    assert (tmp_path / "KEYFOUNDKEYFOUND.txt").read_text() == f"Key found privkey 7cce5efdaccf6808\nPublickey {P63}\n"


def test_bsgsd_resident(tmp_path):
    """bsgsd_amd --resident answers the narrowed query of test_gpu_bsgsd.py and a negative one, and reads or writes
    no table file."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    log_path = tmp_path / "bsgsd.log"
    with open(log_path, "w") as log:
        p = subprocess.Popen([os.path.join(BIN_DIR, "bsgsd_amd"), "-k", "8", "-n", "0x1000000000", "-t", "8", "-p",
                              str(port), "--resident"], cwd=tmp_path, stdout=log, stderr=subprocess.STDOUT)
        try:
            t0 = time.time()
            while time.time() - t0 < 120 and p.poll() is None:
                if "[+] Listening in 127.0.0.1:%d" % port in log_path.read_text():
                    break
                time.sleep(0.1)
            assert p.poll() is None, log_path.read_text()

            def ask(line: bytes) -> str:
                with socket.create_connection(("127.0.0.1", port), timeout=120) as c:
                    c.sendall(line)
                    data = b""
                    while True:
                        chunk = c.recv(4096)
                        if not chunk:
                            return data.decode()
                        data += chunk

            assert ask(f"{P63} 7cce5e0000000000:7cce600000000000\n".encode()) == "7cce5efdaccf6808"
            assert ask(f"{P125} 4000000000000000:4000008000000000\n".encode()) == "404 Not Found"
        finally:
            p.terminate()
            try:
                p.wait(timeout=20)
            except subprocess.TimeoutExpired:
                p.kill()
                p.wait()
    assert "[+] GPU 0 resident: L1 bloom " in log_path.read_text()
    assert not [q for q in tmp_path.iterdir() if q.name.startswith("keyhunt_bsgs_")]
