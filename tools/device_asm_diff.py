#!/usr/bin/env python3
"""Compare the gfx950 device assembly of two source trees, file by file.

    tools/device_asm_diff.py OLD_TREE NEW_TREE [--trace] [--only OBJ] [--jobs N] [--keep DIR]

For a refactor that must not move a kernel: every compile command of csrc/Makefile (`make -n -B all`, or the -DORE_TRACE commands of
`make -n -B trace` with --trace) is re-run in each tree with `--cuda-device-only -S` in place of `-c`, and the two assembly files are
compared.  The `__hip_cuid_<hash>` lines (a hash of the translation unit) are ignored.  The flags come from each tree's own Makefile, so
a change of the flags of an object is reported too.  Prints one line per file -- "identical" or the diff -- and exits 1 on any
difference.  Cross-compiles; needs no GPU.

One known false alarm: hipcc does not always emit the two __device__ variables of the -DORE_TRACE build of ore_conv_kw.hip (g_zero_kw,
g_trace_kw) in the same order, even for two compilations of one tree.  A diff that only swaps those two data symbols is that; run again.  The swap has
also been seen to persist over repeated runs of one pair of trees (it appeared with a whitespace-only edit of a header): then compare the two
files with --keep -- the lines in front of the data symbols must be identical and the sorted files equal.
"""
import argparse
import difflib
import os
import shlex
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

CSRC = os.path.join("faster-orefsdet_amd", "csrc")


def compile_commands(tree, trace):
    """{object name: (argv without -c / -o, source)} from the tree's Makefile."""
    out = subprocess.run(["make", "-n", "-B", "-C", os.path.join(tree, CSRC), "trace" if trace else "all"],
                         check=True, capture_output=True, text=True).stdout
    cmds = {}
    for line in out.splitlines():
        argv = shlex.split(line)
        if "-c" not in argv or ("-DORE_TRACE" in argv) != trace:
            continue
        src = argv[argv.index("-c") + 1]
        obj = os.path.basename(argv[argv.index("-o") + 1])
        flags = [a for i, a in enumerate(argv) if a != "-c" and a != "-o" and argv[i - 1] not in ("-c", "-o")]
        cmds[obj] = (flags, src)
    return cmds


def assemble(tree, flags, src, dst):
    r = subprocess.run(flags + ["--cuda-device-only", "-S", src, "-o", dst], cwd=os.path.join(tree, CSRC), capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("%s: %s failed\n%s" % (tree, src, r.stderr))
    with open(dst) as f:
        return [l for l in f if "__hip_cuid_" not in l]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--trace", action="store_true", help="the -DORE_TRACE objects of `make trace`")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--only", action="append", help="compare only this object (e.g. ore_conv_kd.o); may be repeated")
    ap.add_argument("--keep", help="write the assembly files here (default: a temporary directory)")
    a = ap.parse_args()
    old, new = compile_commands(a.old, a.trace), compile_commands(a.new, a.trace)
    tmp = a.keep or tempfile.mkdtemp(prefix="ore_asm_")
    for side in ("old", "new"):
        os.makedirs(os.path.join(tmp, side), exist_ok=True)
    bad = 0
    for obj in sorted(set(old) ^ set(new)):
        print("%-28s only in %s" % (obj, "old" if obj in old else "new"))
        bad = 1
    objs = sorted(o for o in set(old) & set(new) if not a.only or o in a.only)
    with ThreadPoolExecutor(a.jobs) as ex:
        jobs = {}
        for obj in objs:
            s = os.path.join("%s", obj[:-2] + ".s")
            jobs[obj] = (ex.submit(assemble, a.old, *old[obj], os.path.abspath(s % os.path.join(tmp, "old"))),
                         ex.submit(assemble, a.new, *new[obj], os.path.abspath(s % os.path.join(tmp, "new"))))
        for obj in objs:
            if old[obj][0] != new[obj][0]:
                print("%-28s FLAGS DIFFER\n  old: %s\n  new: %s" % (obj, " ".join(old[obj][0]), " ".join(new[obj][0])))
                bad = 1
            x, y = jobs[obj][0].result(), jobs[obj][1].result()
            if x == y:
                print("%-28s identical (%d lines)" % (obj, len(x)))
            else:
                d = list(difflib.unified_diff(x, y, "old/" + old[obj][1], "new/" + new[obj][1], n=2))
                print("%-28s DIFFERS (%d diff lines)" % (obj, len(d)))
                sys.stdout.writelines(d[:200])
                bad = 1
    return bad


if __name__ == "__main__":
    sys.exit(main())
