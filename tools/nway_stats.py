#!/usr/bin/env python3
"""Kernel statistics of `rocprofv3 --kernel-trace --stats -- python3 tools/bench_nway.py --k K ...` from its rocpd database:
the whole run's per-kernel totals (what --stats tabulates), then ONE N-way pass (stem_1 .. k_roi_merge_classes) and ONE single-class pass
(stem_1 .. k_roi_tail), each averaged over the last `passes` passes of its kind.  usage: nway_stats.py <results.db> [passes]"""
import collections
import sqlite3
import sys


def short(n):
    n = n.replace("(anonymous namespace)::", "").replace("void ", "")
    return n.split("(")[0][:60]


def table(rows, npass, title):
    tot = collections.OrderedDict()
    for name, dur in rows:
        c = tot.setdefault(short(name), [0, 0])
        c[0] += 1
        c[1] += dur
    busy = sum(t for _, t in tot.values())
    print(f"# {title}: {busy / npass / 1e3:.1f} us of kernel time, {sum(c for c, _ in tot.values()) / npass:.1f} launches per pass")
    print("%-60s %7s %9s %9s %6s" % ("kernel", "calls", "us/pass", "avg_us", "%"))
    for n, (c, t) in sorted(tot.items(), key=lambda x: -x[1][1]):
        print("%-60s %7.1f %9.2f %9.2f %6.1f" % (n, c / npass, t / npass / 1e3, t / c / 1e3, 100.0 * t / busy))
    print()


def main():
    db = sqlite3.connect(sys.argv[1])
    P = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    ks = db.execute("select name, start, end, duration from kernels order by start").fetchall()
    allk = [(n, d) for n, _, _, d in ks]
    print("# rocprofv3 --kernel-trace of the whole run: %d dispatches" % len(allk))
    table(allk, 1, "whole run")
    stems = [i for i, k in enumerate(ks) if "k_stem1" in k[0]]
    ends = stems[1:] + [len(ks)]
    nway, single = [], []
    for a, e in zip(stems, ends):                        # a pass starts at its stem_1; the next stem_1 (or the end) bounds it
        names = [k[0] for k in ks[a:e]]
        if any("k_correlation_classes" in n for n in names):
            m = [j for j in range(a, e) if "k_roi_merge_classes" in ks[j][0]]
            if m:
                nway.append((a, m[0]))
        elif any("k_correlation<" in n for n in names):
            t = [j for j in range(a, e) if "k_roi_tail" in ks[j][0]]
            if t:
                single.append((a, t[0]))
    for passes, title in ((nway[-P:], "N-way pass: stem_1 .. k_roi_merge_classes"), (single[-P:], "single-class pass: stem_1 .. k_roi_tail")):
        if not passes:
            continue
        rows = [(ks[j][0], ks[j][3]) for a, b in passes for j in range(a, b + 1)]
        span = sum(ks[b][2] - ks[a][1] for a, b in passes) / len(passes)
        print("# %s, first launch to end of the last: %.1f us (average of the last %d passes)" % (title, span / 1e3, len(passes)))
        table(rows, len(passes), "ONE " + title.split(":")[0])


if __name__ == "__main__":
    main()
