#!/usr/bin/env python3
"""asm_kernel_diff.py A.s B.s [NAME] -- per-kernel diff of two gfx950 assembly listings, up to label numbering.

The listings come from `hipcc $(FLAGS) --cuda-device-only -S -o X.s file.hip` (FLAGS of csrc/Makefile), once at the parent commit and once
at the branch.  Every function's instruction stream is compared with comments and directives dropped and the .LBB labels renumbered in
order of appearance; a kernel whose streams differ is listed with the number of differing lines, and with NAME (a substring of the
mangled name) its unified diff is printed.  Exit status 1 when any kernel differs.
"""
import difflib
import re
import sys


def kernels(path):
    out, name, body = {}, None, []
    for line in open(path):
        line = line.split(";")[0].rstrip()
        if not line.strip():
            continue
        m = re.match(r"^(\w+):\s*$", line)
        if m and name is None and not line.startswith(".L"):
            name, body = m.group(1), []
            continue
        if name is not None:
            if line.startswith(".Lfunc_end"):
                out[name] = body
                name = None
                continue
            s = line.strip()
            if s.startswith(".") and not s.startswith(".LBB"):
                continue                      # directives (.p2align, .loc, ...)
            body.append(s)
    return out


def renumbered(body):
    labels = {}
    return [re.sub(r"\.LBB\d+_\d+", lambda m: labels.setdefault(m.group(0), "L%d" % len(labels)), s) for s in body]


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    show = sys.argv[3] if len(sys.argv) > 3 else None
    bad = 0
    for k in sorted(set(a) | set(b)):
        if k not in a or k not in b:
            print("ONLY IN", sys.argv[1] if k in a else sys.argv[2], k)
            bad += 1
            continue
        na, nb = renumbered(a[k]), renumbered(b[k])
        if na != nb:
            d = [l for l in difflib.unified_diff(na, nb, lineterm="", n=0) if l[0] in "+-" and not l.startswith(("+++", "---"))]
            print("DIFF %5d lines (of %d / %d)  %s" % (len(d), len(na), len(nb), k))
            bad += 1
            if show and show in k:
                print("\n".join(difflib.unified_diff(na, nb, lineterm="", n=3)))
    print("%d kernels in %s, %d in %s, %d differ" % (len(a), sys.argv[1], len(b), sys.argv[2], bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
