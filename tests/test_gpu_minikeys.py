"""GPU parity for -m minikeys: the filter kernel (khb_mini_filter), the fixed-base k*G (khb_mini_pubkey), the whole
launch (khb_mini_scan) and the libkhhost search driver (khhost.Minikeys.search) against the tests' model
(tests/mini_ref.py: hashlib for the two SHA-256, the oracle for points and hash160s).  Every comparison is exact: each
survivor offset, each point, each hit, each find and the counts."""
from __future__ import annotations

import os

import pytest

from keyhuntm1cpu_amd import khbsgs, khhost
from tests import mini_ref as mr

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REV = mr.ALPHABET[::-1]


@pytest.fixture(scope="module")
def eng():
    e = khbsgs.Engine(0, lanes=16384)
    yield e
    e.close()


def _digits(s, alphabet=mr.ALPHABET):
    return bytes(mr.digits(s, alphabet))


@pytest.fixture(scope="module")
def targets():
    with open(os.path.join(HERE, "golden", "address", "1to32.rmd")) as f:
        return f.read()


def _planted(ora, first, offsets):
    """{offset: (minikey, key, rmd160)} of the model for valid candidates of a span."""
    out = {}
    for o in offsets:
        s = mr.step(first, o)
        assert mr.valid(s) and 0 < mr.key(s) < mr.N
        out[o] = (s, mr.key(s), mr.rmd160(ora, s))
    return out


def _text(targets, planted):
    """The golden targets and the planted hash160s.  The loader reads as many lines from the top as it counted lines
    of more than 20 characters (as the reference does), so the golden file's trailing blank line is dropped first."""
    return targets.rstrip("\n") + "\n" + "".join(r.hex() + "\n" for _, _, r in planted.values())


# ---------------------------------------------------------------------------------------------- 1: the filter
@pytest.mark.parametrize("first,count,want", mr.SPANS)
def test_filter_spans(eng, first, count, want):
    got, n = eng.mini_filter(_digits(first), count)
    ref = mr.valid_offsets(first, count)
    assert n == len(ref) == want == len(got)
    assert sorted(got) == ref


def test_filter_single_candidates(eng):
    first, count, _ = mr.SPANS[2]
    offs = mr.valid_offsets(first, count)
    assert eng.mini_filter(_digits(mr.step(first, offs[0])), 1) == ([0], 1)
    assert eng.mini_filter(_digits(mr.step(first, offs[0] + 1)), 1) == ([], 0)
    assert eng.mini_filter(_digits("S" + "z" * 21), 1)[1] == int(mr.valid("S" + "z" * 21))      # the last candidate


def test_filter_cut_in_two(eng):
    """One span cut at an offset that is no multiple of 64 (nor of the lanes' run): the halves are disjoint, their
    union is the whole, and nothing is dropped at the cut."""
    first, count, _ = mr.SPANS[3]
    ref = mr.valid_offsets(first, count)
    cut = ref[len(ref) // 2]                      # the second half begins exactly at a valid candidate
    assert cut % 64
    lo, nlo = eng.mini_filter(_digits(first), cut)
    hi, nhi = eng.mini_filter(_digits(mr.step(first, cut)), count - cut)
    hi = [o + cut for o in hi]
    assert nlo == len(lo) and nhi == len(hi)
    assert not set(lo) & set(hi) and cut in hi and cut not in lo
    assert sorted(lo + hi) == ref
    cap, n = eng.mini_filter(_digits(first), count, cap=5)         # a short output still reports the whole count
    assert n == len(ref) and len(cap) == 5 and set(cap) <= set(ref)


def test_filter_custom_alphabet(eng):
    first = mr.string(mr.value(mr.SPANS[0][0]), REV)              # the same counter value, other characters
    ref = mr.valid_offsets(first, 10109, REV)
    got, n = eng.mini_filter(_digits(first, REV), 10109, alphabet=REV.encode())
    assert n == len(ref) and sorted(got) == ref and ref != mr.valid_offsets(mr.SPANS[0][0], 10109)


# ---------------------------------------------------------------------------------------------- 2: k*G
@pytest.mark.parametrize("w", [4, 8, 16])
def test_pubkey(eng, ora, w):
    """The native test's directed scalars: w = 16's table builds in a fraction of a second, so it runs here too."""
    with khhost.Minikeys("", window_bits=w) as m:
        eng.load_mini_table(m.table_points(), w)
    good, bad = mr.directed_scalars(w)
    ks = good + bad
    got = eng.mini_pubkey(ks)
    for k, (xy, flag) in zip(ks, got):
        if k in bad:
            assert flag == 1 and xy == bytes(64), hex(k)
        else:
            assert flag == 0 and xy == ora.pubkey(k).be64(), hex(k)


# ---------------------------------------------------------------------------------------------- 3: the launch
def _load(eng, text, w=8, bloom_multiplier=1):
    with khhost.Minikeys(text, window_bits=w, bloom_multiplier=bloom_multiplier) as m:
        eng.load_mini_table(m.table_points(), w)
    with khhost.Addr(text, n_seq=1024, bloom_multiplier=bloom_multiplier) as a:     # the same loader: its bloom
        bf, bits, hashes = a.bloom()
    eng.load_addr_bloom(bf, bits, hashes)


def test_scan_planted(eng, ora, targets):
    first, count, nvalid = mr.SPANS[2]
    offs = mr.valid_offsets(first, count)
    pl = _planted(ora, first, [offs[0], offs[len(offs) // 2], offs[-1]])
    _load(eng, _text(targets, pl))
    hits, st = eng.mini_scan(_digits(first), count)
    assert (st.candidates, st.valid, st.bad_keys, st.queue_overflow, st.hit_overflow) == (count, nvalid, 0, 0, 0)
    assert st.hits == len(hits) and len({o for o, _ in hits}) == len(hits)
    got = dict(hits)
    assert set(pl) <= set(got) <= set(offs)                       # bloom false positives are valid candidates too
    for o, h in got.items():
        assert h == mr.rmd160(ora, mr.step(first, o))
    _load(eng, targets)                                           # the targets alone: no planted hit
    hits, st = eng.mini_scan(_digits(first), count)
    assert st.valid == nvalid and not set(pl) & {o for o, _ in hits}


def test_search_planted(ora, targets):
    first, count, nvalid = mr.SPANS[2]
    offs = mr.valid_offsets(first, count)
    pl = _planted(ora, first, [offs[0], offs[len(offs) // 2], offs[-1]])
    with khhost.Minikeys(_text(targets, pl)) as m:
        found, st = m.search(first, count, lanes=16384)
    assert found == [pl[o] for o in sorted(pl)]
    assert (st["candidates"], st["valid"], st["bad_keys"], st["rescans"]) == (count, nvalid, 0, 0)
    with khhost.Minikeys(targets) as m:
        found, st = m.search(first, count, lanes=16384)
    assert found == [] and (st["candidates"], st["valid"]) == (count, nvalid)


# ---------------------------------------------------------------------------------------------- 4: overflow
def test_queue_overflow_is_reported_and_rescanned(eng, ora, targets):
    first, count, nvalid = mr.SPANS[3]
    offs = mr.valid_offsets(first, count)
    pl = _planted(ora, first, [offs[0], offs[len(offs) // 2], offs[-1]])
    _load(eng, _text(targets, pl))
    eng.set_mini_queue_capacity(8)
    try:
        _, st = eng.mini_scan(_digits(first), count)
    finally:
        eng.set_mini_queue_capacity(0)
    assert st.queue_overflow == 1 and st.valid == nvalid          # counted past the capacity, and reported
    with khhost.Minikeys(_text(targets, pl)) as m:
        m.set_queue_capacity(8)
        found, st = m.search(first, count, lanes=16384)
    assert sorted(found) == sorted(pl.values())                   # rescan parts report in launch order
    assert (st["candidates"], st["valid"]) == (count, nvalid) and st["rescans"] >= 1
    # launches of a bounded size: the same span in pieces of 1,000 candidates
    with khhost.Minikeys(_text(targets, pl)) as m:
        found, st = m.search(first, count, lanes=16384, per_launch=1000)
    assert found == [pl[o] for o in sorted(pl)]
    assert (st["candidates"], st["valid"], st["launches"], st["rescans"]) == (count, nvalid, 66, 0)


def test_hit_ring_overflow_is_rescanned(eng, ora, targets):
    """All 38 valid candidates planted: every one is a bloom hit, a ring of 4 overflows and nothing is lost."""
    first, count, nvalid = mr.SPANS[2]
    pl = _planted(ora, first, mr.valid_offsets(first, count))
    text = _text(targets, pl)
    _load(eng, text)
    eng.set_candidate_capacity(4)
    try:
        hits, st = eng.mini_scan(_digits(first), count)
    finally:
        eng.set_candidate_capacity(1 << 20)
    assert st.hit_overflow == 1 and st.hits == nvalid and len(hits) == 4
    with khhost.Minikeys(text) as m:
        m.set_hit_capacity(4)
        found, st = m.search(first, count, lanes=16384)
    assert sorted(found) == sorted(pl.values()) and len(found) == nvalid      # in launch order, each once
    assert (st["candidates"], st["valid"]) == (count, nvalid) and st["rescans"] >= 1


# ---------------------------------------------------------------------------------------------- 5: long runs
# Every test above opens 16,384 lanes, where a filter lane's run is the minimum of 64 and the keys kernel never makes a
# second pass.  With 256 lanes the filter has 1,024 lanes and the keys kernel one block, so spans of a few million
# candidates reach the run lengths of a production launch (hundreds to 4,096, the clamp) against tests/mini_ref.py's
# block-wise enumerator.
FILTER_LANES = 4 * 256
RUN_SPANS = [(262_144, 256), (FILTER_LANES * 600 + 17, 601), (FILTER_LANES * 3400, 3400)]


@pytest.fixture(scope="module")
def small():
    e = khbsgs.Engine(0, lanes=256)
    assert e.lanes() == 256
    yield e
    e.close()


def _run(count):
    return min(4096, max(64, -(-count // FILTER_LANES)))


@pytest.mark.parametrize("count,run", RUN_SPANS, ids=["run-256", "run-601-ragged", "run-3400"])
def test_filter_run_lengths(small, count, run):
    """Runs of 256 (four d20 wraps each, most lanes starting mid-run), 601 with a ragged last lane, and 3,400: above
    58^2 = 3,364, so every lane repacks its head once and some twice."""
    assert _run(count) == run
    ref = [o for o in mr.valid_offsets_fast(mr.A, RUN_SPANS[-1][0]) if o < count]
    assert len(mr.valid_offsets_fast(mr.A, RUN_SPANS[-1][0])) == 13_332
    got, n = small.mini_filter(_digits(mr.A), count)
    assert n == len(ref) == len(got)
    assert sorted(got) == ref


def test_filter_run_clamp(small):
    """The run clamped at 4,096: more blocks than 4 * lanes / 256, a ragged tail, and the carry through 20 digits (six
    candidates in) inside the first lane's run."""
    count = FILTER_LANES * 4096 + 4096 * 3 + 5
    assert -(-count // FILTER_LANES) > 4096 == _run(count) and -(-count // 4096) == FILTER_LANES + 4
    ref = mr.valid_offsets_fast(mr.B, count)
    got, n = small.mini_filter(_digits(mr.B), count)
    assert n == len(ref) == len(got)
    assert sorted(got) == ref


def test_keys_kernel_second_pass(small, ora, targets):
    """275 survivors against the 256 lanes of the keys kernel's one block: 19 of them come from a second pass of its
    grid-stride loop.  Every survivor is planted, so each must come back once with the oracle's hash160."""
    first, count, nvalid = mr.SPANS[3]
    offs = mr.valid_offsets_fast(first, count)
    assert len(offs) == nvalid == 275 > small.lanes()
    pl = _planted(ora, first, offs)
    _load(small, _text(targets, pl), w=8)
    hits, st = small.mini_scan(_digits(first), count)
    assert (st.candidates, st.valid, st.hits, st.bad_keys) == (count, 275, 275, 0)
    assert (st.queue_overflow, st.hit_overflow) == (0, 0)
    assert len(hits) == 275 and sorted(o for o, _ in hits) == offs
    for o, h in hits:
        assert h == pl[o][2]


# ---------------------------------------------------------------------------------------------- 6: errors
def test_errors_launch_nothing(targets):
    last = "S" + "z" * 21
    with khbsgs.Engine(0, lanes=16384) as e:
        with pytest.raises(khbsgs.KhbError) as ei:                # before khb_load_mini_table
            e.mini_scan(_digits(mr.SPANS[0][0]), 10)
        assert ei.value.code == khbsgs.KHB_ESTATE
        with pytest.raises(khbsgs.KhbError) as ei:
            e.mini_pubkey([1])
        assert ei.value.code == khbsgs.KHB_ESTATE
        _load(e, targets, w=4)
        for first, count in ((last, 2), (mr.step(last, -9), 11), (mr.SPANS[0][0], 0), (mr.SPANS[0][0], (1 << 32) + 1)):
            with pytest.raises(khbsgs.KhbError) as ei:
                e.mini_scan(_digits(first), count)
            assert ei.value.code == khbsgs.KHB_EINVAL
            with pytest.raises(khbsgs.KhbError) as ei:
                e.mini_filter(_digits(first), count)
            assert ei.value.code == khbsgs.KHB_EINVAL
        with pytest.raises(khbsgs.KhbError) as ei:                # a digit of 58, a repeated alphabet byte
            e.mini_scan(bytes([58] * 21), 1)
        assert ei.value.code == khbsgs.KHB_EINVAL
        with pytest.raises(khbsgs.KhbError) as ei:
            e.mini_scan(_digits(last), 1, alphabet=b"1" + mr.ALPHABET[:57].encode())
        assert ei.value.code == khbsgs.KHB_EINVAL
        hits, st = e.mini_scan(_digits(mr.step(last, -9)), 10)    # the last ten candidates are a span
        assert st.candidates == 10
    with khhost.Minikeys(targets, window_bits=4) as m:
        with pytest.raises(ValueError):
            m.search(last, 2)
