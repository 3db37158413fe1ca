#!/usr/bin/env python3
"""Compare two device assembly files (hipcc --cuda-device-only -S) kernel by kernel.

Usage: tools/debug/isa_diff.py A.s B.s

Comment text, .file / .loc / .ident lines and the per-build __hip_cuid_* symbol are dropped; what is left is split
at the function labels (every symbol with a `.type sym,@function`), plus one section "<rest>" for everything outside
functions (kernel descriptors, metadata).  Prints "identical" or the first differing line per symbol; exit status 1
if anything differs.
"""
import re
import sys

DROP = re.compile(r"^\s*\.(file|loc|ident)\b")
FUNC = re.compile(r"^\s*\.type\s+([^,\s]+),@function")
END = re.compile(r"^\s*\.size\s+([^,\s]+),")
SET = re.compile(r"^\s*\.set\s+(\S+)\.\w+,")
NAME = re.compile(r"^    \.name:\s+(\S+)$")      # the kernel's own name (argument names sit deeper)


def strip(line):
    line = re.sub(r"\s*(;|//).*$", "", line.rstrip("\n")).rstrip()
    if not line.strip() or DROP.match(line) or "__hip_cuid_" in line:
        return None
    return line


def sections(path):
    out, cur = {"<rest>": []}, "<rest>"
    meta = None                      # lines of the metadata entry being read (one per kernel)

    def flush_meta():
        name = next((NAME.match(l).group(1) for l in meta if NAME.match(l)), "<rest>")
        out.setdefault(name, []).extend(meta)

    for raw in open(path, errors="replace"):
        line = strip(raw)
        if line is None:
            continue
        if meta is not None:         # inside .amdgpu_metadata: one "  - " entry per kernel, named by its .name
            if not line.startswith("    "):          # the next entry, or the keys after the kernel list
                flush_meta()
                meta = None if ".end_amdgpu_metadata" in line else []
            if meta is not None:
                meta.append(line)
                continue
        elif line.strip() == ".amdgpu_metadata":
            meta = []
        m = FUNC.match(line)
        if m:
            cur = m.group(1)
            out.setdefault(cur, [])
        m = SET.match(line)          # a function's resource counts follow its .size
        out[m.group(1) if m and m.group(1) in out else cur].append(line)
        m = END.match(line)
        if m and m.group(1) == cur:
            cur = "<rest>"
    return out


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    a, b = sections(sys.argv[1]), sections(sys.argv[2])
    differ = False
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            differ = True
            print(f"{name}: only in {sys.argv[2] if name in b else sys.argv[1]}")
            continue
        la, lb = a[name], b[name]
        if la == lb:
            print(f"{name}: identical ({len(la)} lines)")
            continue
        differ = True
        k = next((i for i, (x, y) in enumerate(zip(la, lb)) if x != y), min(len(la), len(lb)))
        print(f"{name}: DIFFERS at line {k} of {len(la)} / {len(lb)}")
        print(f"  A: {la[k].strip() if k < len(la) else '<end>'}")
        print(f"  B: {lb[k].strip() if k < len(lb) else '<end>'}")
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()
