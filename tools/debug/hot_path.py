"""VALU mix along the hot path of one loop of a gfx950 kernel (.s from `hipcc --cuda-device-only -S`).

The walk's rare branches (carry propagation, x >= p canonicalisation, queue flushes) are entered when
some lane needs them: `s_cbranch_vccz L` / `s_cbranch_execz L` skip them, so the hot path takes those
branches and falls through every other conditional branch.  The reduction's carry fix (fe_asm.hpp fm_fix_R)
is skipped by `s_cmp_eq_u64 <mask>, 0` ... `s_cbranch_scc1 L` (VALU in between leaves SCC alone) when no lane's
V mad carried out: that branch is taken too.  Starting at the loop header label, the path is followed until it branches back to a label at or
before the header (the loop's back edge).

Moves are split by what they copy: a VGPR that holds zero, an SGPR, a literal, or another VGPR.  The zero set is a
heuristic: a VGPR enters it when `v_mov_b32 vN, 0` (or a copy of a zero VGPR) writes it and leaves it when any
instruction names it as destination (VALU, or a scratch / global / LDS load), tracked from the kernel's entry in
layout order, not along control flow, and then along the path.  A register zeroed on a path the layout order skips is
missed, and one cleared only on such a path is dropped early.  Spill traffic (scratch_*) on the path is counted as well.
The scc1 rule takes every `s_cmp_eq_u64 sN, 0` ... `s_cbranch_scc1` pair, whatever it guards; check with -v that the
count of `s_cmp_eq_u64` on the path is the number of field products (13 in the pair loop) before relying on it.

Usage: python tools/debug/hot_path.py file.s <kernel-substring> <header-label> [-v]
Prints the instruction classes of tools/debug/bb_path.py (full-rate, half-rate, cndmask, nop), the carry adds,
the moves by source and the spill ops and, with -v, every opcode count and each cndmask with the instruction
before it.  With -w, every vector-memory, LDS and scratch instruction and every s_waitcnt on the path, in path order,
each with the number of VALU instructions and of v_mad_u64_u32 (64 per field product, 36 per squaring) issued on
the path before it: where the loads are issued and where the walk waits for them."""
import re
import sys
from collections import Counter

sys.path.insert(0, __import__("os").path.dirname(__file__))
from bb_path import klass  # noqa: E402


def main():
    src, name, header = sys.argv[1:4]
    lines = open(src).read().split("\n")
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\w*" + name + r"\w*:", l))
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith(".Lfunc_end"))
    body = [l.strip() for l in lines[start:end]]
    labels = {l.split(":")[0]: i for i, l in enumerate(body) if re.match(r"^\.LBB\d+_\d+:", l)}
    i = labels[header.rstrip(":")]
    h = i
    last = ""
    ops, cnd, seen = Counter(), [], 0
    prev = ""
    movs, zero, inner = Counter(), set(), set()
    mem, nvalu = [], 0

    def track(s):
        """Keep `zero` (VGPRs known to hold 0) current over instruction s; classify s if it is a move."""
        t = s.replace(",", " ").split()
        load = t[0].startswith(("scratch_load", "global_load", "flat_load", "buffer_load", "ds_read", "ds_load"))
        if not (t[0].startswith("v_") or load) or len(t) < 2:
            return None
        m = re.match(r"v\[(\d+):(\d+)\]$", t[1])
        dst = set(range(int(m.group(1)), int(m.group(2)) + 1)) if m else \
            ({int(t[1][1:])} if re.match(r"v\d+$", t[1]) else set())
        kind = None
        if t[0].startswith("v_mov_b32") and len(t) == 3:
            src = t[2]
            if re.match(r"v\d+$", src):
                kind = "zero" if int(src[1:]) in zero else "vgpr"
            else:
                kind = "sgpr" if re.match(r"s\d+$", src) else "literal"
            if src == "0" or kind == "zero":
                zero.update(dst)
                return kind
        zero.difference_update(dst)
        return kind

    for s in body[:h]:
        if s and not s.startswith((";", ".")):
            track(s)
    while True:
        i += 1
        seen += 1
        if seen > 200000:
            raise SystemExit("no back edge found")
        s = body[i]
        if not s or s.startswith((";", ".")):
            continue
        op = s.split()[0]
        skip_fix = op == "s_cbranch_scc1" and re.match(r"s_cmp_eq_u64 s\[\d+:\d+\], 0$", last)
        if op.startswith("s_") and not op.startswith(("s_nop", "s_waitcnt", "s_mov", "s_load", "s_cbranch", "s_branch")):
            last = s              # the latest instruction that may have written SCC
        if op.startswith("s_cbranch_vccz") or op.startswith("s_cbranch_execz") or op == "s_branch" or skip_fix:
            tgt = s.split()[1]
            if labels[tgt] <= h:
                break
            if labels[tgt] <= i:          # an inner loop's back edge (a queue drain): one pass, then fall through
                if tgt in inner:
                    continue
                inner.add(tgt)
            i = labels[tgt]
            continue
        if op.startswith("s_cbranch"):
            continue
        if op.startswith(("global_", "flat_", "buffer_", "scratch_", "ds_", "s_waitcnt")):
            mem.append((nvalu, ops["v_mad_u64_u32"], s))
        nvalu += op.startswith("v_")
        ops[op] += 1
        k = track(s)
        if k:
            movs[k] += 1
        if op.startswith("v_cndmask"):
            cnd.append((s, prev))
        if op.startswith("v_"):
            prev = s
    tot = Counter()
    for op, n in ops.items():
        tot[klass(op)] += n
    print("hot path", dict(tot), "valu", tot["full"] + tot["half"] + tot["cndmask"],
          "v_mad_u64_u32", ops["v_mad_u64_u32"], "cndmask_vcc", sum(1 for c, _ in cnd if c.endswith("vcc")))
    print("carry adds", sum(n for o, n in ops.items() if o.startswith(("v_addc_co_u32", "v_add_co_u32"))),
          "v_mov_b32", sum(movs.values()), dict(movs),
          "spill ops", sum(n for o, n in ops.items() if o.startswith("scratch_")))
    if "-w" in sys.argv:
        for v, m, t in mem:
            print(f"  valu {v:5d} mad {m:4d}  {t}")
    if "-v" in sys.argv:
        for k, v in ops.most_common(40):
            print(f"  {v:5d} {k}")
        for c, p in cnd:
            print(f"  {c}   <- {p}")


if __name__ == "__main__":
    main()
