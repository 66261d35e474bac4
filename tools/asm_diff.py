#!/usr/bin/env python3
"""Compare two device-assembly files kernel by kernel.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -I include \
        --cuda-device-only -S <pkg>/csrc/pcm_engine.hip -o new.s     (same for the parent: old.s)
    tools/asm_diff.py old.s new.s

The `__hip_cuid_` lines (a hash of the source) are dropped and local labels are
renumbered in order of appearance, so a kernel that only moved in the file
compares equal.  Prints every kernel whose code differs with both versions'
resource lines, then a one-line total; exit status 1 if any differs.
"""
import re
import sys

RES = ("TotalNumSgprs", "NumVgprs", "ScratchSize", "LDSByteSize", "Occupancy", "codeLenInByte")


def kernels(path):
    out, name, body = {}, None, []
    for line in open(path):
        if "__hip_cuid_" in line:
            continue
        m = re.match(r"^(_Z\w+):", line)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is not None:
            body.append(line.rstrip())
            if line.startswith(".Lfunc_end"):
                out[name] = body
                name = None
    # the resource comments follow .Lfunc_end: collect them per kernel
    res, cur = {}, None
    for line in open(path):
        m = re.match(r"^\s*\.size\s+(_Z\w+),", line)
        if m:
            cur = m.group(1)
            res[cur] = {}
        m = re.match(r"^; (\w+)(?::| =) (\d+)", line)
        if m and cur and m.group(1) in RES:
            res[cur].setdefault(m.group(1), m.group(2))
    return out, res


def normal(body):
    ids = {}
    def sub(m):
        return ids.setdefault(m.group(0), ".L%d" % len(ids))
    return [re.sub(r"\.L(?:BB|func_end|tmp)?[0-9_]+", sub, l) for l in body]


def main():
    a, ra = kernels(sys.argv[1])
    b, rb = kernels(sys.argv[2])
    bad = sorted(set(a) ^ set(b))
    for k in bad:
        print("only in one file:", k)
    ndiff = 0
    for k in sorted(set(a) & set(b)):
        if normal(a[k]) != normal(b[k]):
            ndiff += 1
            print("differs:", k)
            for r, tag in ((ra, "old"), (rb, "new")):
                print("   %s " % tag + " ".join("%s=%s" % (f, r.get(k, {}).get(f, "?")) for f in RES))
    print("%d kernels compared, %d differ, %d unmatched" % (len(set(a) & set(b)), ndiff, len(bad)))
    return 1 if (ndiff or bad) else 0


if __name__ == "__main__":
    sys.exit(main())
