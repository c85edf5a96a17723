#!/usr/bin/env python3
"""Compare two device-assembly files kernel by kernel (no GPU): python tools/isa_equal.py [--rename REGEX=REPL ...] old.s new.s

The files come from `hipcc <build.FLAGS> <build.EXTRA[source]> --cuda-device-only -S source.hip -o file.s` on the two trees; for kernels that
moved between translation units (the GEMM: build.GEMM), concatenate the units' files of a tree.  A kernel is
equal when its instruction text is equal (comments dropped, `.LBB<n>_` -> `.LBB_`: the function index in block labels shifts when kernels
move inside the file) and its `.amdhsa_kernel` block (VGPR / AGPR / SGPR counts, LDS, scratch) is equal.  --rename rewrites OLD kernel
names before they are matched, for kernels whose template parameter list changed.  Exit status 1 when any kernel differs or is unmatched."""
import re
import sys


def kernels(path):
    """name -> (instruction lines, descriptor lines) of every kernel of an assembly file"""
    descs, labelled = {}, {}
    name = desc = None
    for ln in open(path):
        m = re.match(r"\s+\.amdhsa_kernel (\S+)", ln)
        if m:
            desc = descs.setdefault(m.group(1), [])
        elif ".end_amdhsa_kernel" in ln:
            desc = None
        elif desc is not None:
            desc.append(ln.strip())
        elif re.match(r"\w+:", ln):   # a global symbol (labels inside a function start with .L)
            name = ln.split(":")[0]
            labelled[name] = []
        elif ln.startswith(".Lfunc_end"):
            name = None
        elif name is not None:
            text = re.sub(r"\.LBB\d+_", ".LBB_", ln.split(";")[0].rstrip())
            if text.strip():
                labelled[name].append(text)
    return {k: (labelled[k], descs[k]) for k in descs}   # (a function without a descriptor is not a kernel)


def main(argv):
    renames = []
    while argv and argv[0] == "--rename":
        pat, repl = argv[1].split("=", 1)
        renames.append((re.compile(pat), repl))
        argv = argv[2:]
    if len(argv) != 2:
        sys.exit(__doc__)
    old, new = kernels(argv[0]), kernels(argv[1])
    for pat, repl in renames:
        old = {pat.sub(repl, k): ([pat.sub(repl, t) for t in v[0]], v[1]) for k, v in old.items()}
    same = bad = 0
    for k in sorted(set(old) | set(new)):
        if k not in old or k not in new:
            print("only in %s: %s" % ("old" if k in old else "new", k))
        elif old[k][0] != new[k][0]:
            print("instructions differ (%d / %d lines): %s" % (len(old[k][0]), len(new[k][0]), k))
        elif old[k][1] != new[k][1]:
            print("kernel descriptor differs: %s" % k)
        else:
            same += 1
            continue
        bad += 1
    print("%d kernels in old, %d in new: %d identical, %d differing or unmatched" % (len(old), len(new), same, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
