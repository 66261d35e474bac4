#!/usr/bin/env python3
"""Compare device assembly kernel by kernel: one old file against one or more new ones.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -I include \
        --cuda-device-only -S <pkg>/csrc/<unit>.hip -o <unit>.s      (same for the parent: old.s)
    tools/asm_diff.py old.s new.s                  one unit against its parent
    tools/asm_diff.py old.s unit1.s unit2.s ...    a unit against the units it was split into

The `__hip_cuid_` lines (a hash of the source) are dropped and local labels are
renumbered in order of appearance, so a kernel that only moved in the file
compares equal.  Every kernel of the old file must appear in at least one new
file, every appearance must compare equal, and no new file may hold a kernel
the old one lacks.  Prints every kernel whose code differs with both versions'
resource lines, the kernels that appear in more than one new file (a split
should leave only non-template kernels of shared headers there), then a
one-line total; exit status 1 if any kernel differs or is unmatched.
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
    out = []
    for l in body:
        l = re.sub(r"\.L(?:BB|func_end|tmp)?[0-9_]+", sub, l)
        l = re.sub(r"\s+;", " ;", l)   # comments are padded to a column: a longer label number shifts them
        l = re.sub(r"\bBB\d+_(\d+)", r"BB_\1", l)   # loop comments name blocks by the function's index in its file
        # an `inline` kernel (one a header shared by several units defines) sits in COMDAT sections of its own
        l = re.sub(r'^\t\.section\t\.(text|rodata)\.\w+,"(\w+)G",@progbits,\w+,comdat$',
                   lambda m: "\t.text" if m.group(1) == "text" else '\t.section\t.rodata,"%s",@progbits' % m.group(2), l)
        out.append(l)
    return out


def main():
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    a, ra = kernels(sys.argv[1])
    news = [(p,) + kernels(p) for p in sys.argv[2:]]
    where = {}
    for p, b, _ in news:
        for k in b:
            where.setdefault(k, []).append(p)
    bad = sorted(set(a) ^ set(where))
    for k in bad:
        print("only in the old file:" if k in a else "only in %s:" % ", ".join(where[k]), k)
    ndiff = 0
    for p, b, rb in news:
        for k in sorted(set(a) & set(b)):
            if normal(a[k]) != normal(b[k]):
                ndiff += 1
                print("differs:", k, "(%s)" % p if len(news) > 1 else "")
                for r, tag in ((ra, "old"), (rb, "new")):
                    print("   %s " % tag + " ".join("%s=%s" % (f, r.get(k, {}).get(f, "?")) for f in RES))
    if len(news) > 1:
        for p, b, _ in news:
            print("%s: %d kernels" % (p, len(b)))
        for k in sorted(k for k, ps in where.items() if len(ps) > 1):
            print("in %d files: %s" % (len(where[k]), k))
    print("%d kernels compared, %d differ, %d unmatched" % (len(set(a) & set(where)), ndiff, len(bad)))
    return 1 if (ndiff or bad) else 0


if __name__ == "__main__":
    sys.exit(main())
