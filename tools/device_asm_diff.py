#!/usr/bin/env python3
"""Compare the gfx950 device assembly of two source trees, file by file or kernel by kernel.

    tools/device_asm_diff.py OLD_TREE NEW_TREE [--kernels] [--trace] [--only OBJ] [--jobs N] [--keep DIR]

For a refactor that must not move a kernel: every compile command of csrc/Makefile (`make -n -B all`, or the -DORE_TRACE commands of
`make -n -B trace` with --trace) is re-run in each tree with `--cuda-device-only -S` in place of `-c`, and the two assembly files are
compared.  The `__hip_cuid_<hash>` lines (a hash of the translation unit) are ignored.  The flags come from each tree's own Makefile, so
a change of the flags of an object is reported too.  Prints one line per file -- "identical" or the diff -- and exits 1 on any
difference.  Cross-compiles; needs no GPU.

--kernels, for a refactor that moves code between translation units: the unit of comparison is the function symbol, wherever it lives.
The text of a symbol is its assembly from its label to its `.Lfunc_end`, plus its `.amdhsa_kernel` descriptor block (registers, LDS,
kernel-argument size) when it is a kernel.  The function-index part of local labels (`.LBB<n>_<m>`, `.Lfunc_end<n>`, and the `BB<n>_<m>`
of the loop comments), which counts the functions of the file in front of this one, is dropped, and so is the padding in front of a
comment.  Prints one line per symbol with the object(s) holding it on each side --
"identical", the diff, or "only in old / new" -- and exits 1 on any of the latter two.  (--only then limits the objects read, on both
sides.)

One known false alarm: hipcc does not always emit the two __device__ variables of the -DORE_TRACE build of ore_conv_kw.hip (g_zero_kw,
g_trace_kw) in the same order, even for two compilations of one tree.  A diff that only swaps those two data symbols is that; run again.  The swap has
also been seen to persist over repeated runs of one pair of trees (it appeared with a whitespace-only edit of a header): then compare the two
files with --keep -- the lines in front of the data symbols must be identical and the sorted files equal.
"""
import argparse
import difflib
import os
import re
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


FUNC_LABEL = re.compile(r"^([A-Za-z_$][\w$.]*):\s*; @\1\s*$")
FUNC_END = re.compile(r"^\.Lfunc_end\d+:")
KD_BEGIN = re.compile(r"^\s*\.amdhsa_kernel\s+(\S+)")
LOCAL_LABEL = re.compile(r"(\.L|\b)(BB|func_end)\d+")        # .LBB<n>_<m>, .Lfunc_end<n>, and the BB<n>_<m> of the loop comments
COMMENT_PAD = re.compile(r"[ \t]+;")                       # a comment's column depends on the length of the label in front of it


def symbols(lines):
    """{function symbol: its normalised lines} of one assembly file."""
    out, cur = {}, None
    for l in lines:
        m = FUNC_LABEL.match(l) or KD_BEGIN.match(l)
        if m:
            cur = out.setdefault(m.group(1), [])
        if cur is not None:
            cur.append(COMMENT_PAD.sub(" ;", LOCAL_LABEL.sub(r"\1\2", l)))
            if FUNC_END.match(l) or ".end_amdhsa_kernel" in l:
                cur = None
    return out


def diff_kernels(asm):
    """asm: {object: (old lines, new lines)}.  Compares every function symbol across all objects of a side."""
    sides = ({}, {})                                   # symbol -> [(object, lines)]
    for obj, pair in sorted(asm.items()):
        for side, lines in zip(sides, pair):
            for sym, text in symbols(lines or []).items():
                side.setdefault(sym, []).append((obj, text))
    bad = 0
    for sym in sorted(set(sides[0]) | set(sides[1])):
        o, n = sides[0].get(sym, []), sides[1].get(sym, [])
        where = "%s -> %s" % (",".join(x[0] for x in o) or "-", ",".join(x[0] for x in n) or "-")
        if not o or not n:
            print("%-72s only in %s (%s)" % (sym, "old" if o else "new", where))
            bad = 1
        elif sorted(x[1] for x in o) == sorted(x[1] for x in n):
            print("%-72s identical (%d lines; %s)" % (sym, sum(len(x[1]) for x in n), where))
        else:
            d = list(difflib.unified_diff(o[0][1], n[0][1], "old/" + o[0][0], "new/" + n[0][0], n=2))
            print("%-72s DIFFERS (%d diff lines; %s)" % (sym, len(d), where))
            sys.stdout.writelines(d[:200])
            bad = 1
    return bad


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--kernels", action="store_true", help="compare symbol by symbol across all objects instead of file by file")
    ap.add_argument("--trace", action="store_true", help="the -DORE_TRACE objects of `make trace`")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--only", action="append", help="compare only this object (e.g. ore_conv_kd.o); may be repeated")
    ap.add_argument("--keep", help="write the assembly files here (default: a temporary directory)")
    a = ap.parse_args()
    old, new = compile_commands(a.old, a.trace), compile_commands(a.new, a.trace)
    tmp = a.keep or tempfile.mkdtemp(prefix="ore_asm_")
    for side in ("old", "new"):
        os.makedirs(os.path.join(tmp, side), exist_ok=True)
    if a.kernels:
        with ThreadPoolExecutor(a.jobs) as ex:
            jobs = {}
            for obj in sorted(o for o in set(old) | set(new) if not a.only or o in a.only):
                s = os.path.join("%s", obj[:-2] + ".s")
                jobs[obj] = tuple(ex.submit(assemble, tree, *cmds[obj], os.path.abspath(s % os.path.join(tmp, side))) if obj in cmds else None
                                  for tree, cmds, side in ((a.old, old, "old"), (a.new, new, "new")))
            return diff_kernels({obj: tuple(j.result() if j else None for j in pair) for obj, pair in jobs.items()})
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
