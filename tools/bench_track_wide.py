"""Time the wide tracker (csrc/ore_track_wide.hip: k_track_wide_cand + k_track_wide_match, association contract "track v1").

  kernels   kernel time of the two launches of one update at (rows, tracks) = (320, 1024), (2000, 3000) and (8192, 16384), from
            rocprofv3 --kernel-trace in runs of their own (one child process per shape, this file with --child): per kernel the median
            over the timed launches.  At (320, 1024) the one-workgroup kernel k_track_update runs beside it in the same child, on the
            same rows.  Every row of the timed frame continues a track (boxes moved by a pixel, in another order); every call starts
            from the same state (a device copy restores it).  The ids are checked once per shape before anything is timed: against
            track_host(wide=True) at the first two shapes, against the construction (every row matched, no new id) at the limits,
            where the host twin's IoU matrix would be 512 MB.
  tiled     TiledPredictor frames/s on a 2160x3840 frame (tile 640, overlap 128, fold 8, max_detections 2000), tracking off and on,
            alternating round by round in one process, the profiler off.

The detector is the synthetic-weight model of the test suite.  Prints one JSON line.

    python tools/bench_track_wide.py [--launches 200] [--frames 20] [--rounds 5] [--out profiles/track_wide_bench.json] [--no-tiled]
"""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "faster-orefsdet_amd"), ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

SHAPES = [(320, 1024), (2000, 3000), (8192, 16384)]
KERNELS = ("k_track_wide_cand", "k_track_wide_match", "k_track_update")
FRAME_HW, TILE, OVERLAP, FOLD, MAX_DET = (2160, 3840), 640, 128, 8, 2000


def drifting(rows, tracks, seed):
    """`tracks` disjoint boxes (one per 100 x 100 cell), and `rows` of them moved by up to a pixel, in another order."""
    rng = np.random.default_rng(seed)
    cell = np.arange(tracks)
    x0, y0 = (cell % 128) * 100.0 + rng.uniform(0, 15, tracks), (cell // 128) * 100.0 + rng.uniform(0, 15, tracks)
    b = np.stack([x0, y0, x0 + rng.uniform(40, 80, tracks), y0 + rng.uniform(40, 80, tracks)], 1).astype(np.float32)
    pick = rng.permutation(tracks)[:rows]
    b1 = (b[pick] + rng.uniform(-1, 1, (rows, 4))).astype(np.float32)
    s = lambda k: rng.uniform(0.3, 1.0, k).astype(np.float32)
    return (b, s(tracks), np.zeros(tracks, np.int64)), (b1, s(rows), np.zeros(rows, np.int64))


def primed(tr, frame, chunk):
    """The tracker with every box of `frame` as a track: updates of at most `chunk` rows (the boxes are disjoint: nothing matches)."""
    tr.reset()
    b, s, c = frame
    for i in range(0, len(s), chunk):
        tr.update(torch.from_numpy(b[i:i + chunk]).cuda(), torch.from_numpy(s[i:i + chunk]).cuda(), torch.from_numpy(c[i:i + chunk]).cuda())
    return tr


def child(index, launches):
    """One shape under the profiler: `launches` timed updates per tracker, each behind a restore of the state."""
    import orehip
    rows, tracks = SHAPES[index]
    f0, f1 = drifting(rows, tracks, rows)
    trackers = [primed(orehip.WideBoxTracker("cuda", capacity=tracks, max_rows=rows), f0, rows)]
    if index == 0:
        trackers.append(primed(orehip.BoxTracker("cuda", capacity=tracks), f0, rows))
    b, s, c = (torch.from_numpy(a).cuda() for a in f1)
    ids = torch.empty(rows, dtype=torch.int64, device="cuda")
    for tr in trackers:
        before = tr.state_host()
        assert before["m"] == tracks, (before["m"], tracks)
        saved = tr._buf.clone()
        tr.update(b, s, c, out=ids)
        got = ids.cpu().numpy()
        if index < 2:
            want, _ = orehip.track_host(before, *f1, capacity=tracks, wide=True)
            assert np.array_equal(got, want), (rows, tracks)
        assert (got >= 0).all() and len(set(got.tolist())) == rows and got.max() < tracks and tr.stats()["started"] == tracks
        for _ in range(launches + 10):                       # the parent takes the last `launches` of each kernel
            tr._buf.copy_(saved)
            tr.update(b, s, c, out=ids)
        torch.cuda.synchronize()


def kernel_times(index, launches, limit):
    d = os.path.join(ROOT, "profiles", f"track_wide_trace_{index}")
    shutil.rmtree(d, ignore_errors=True)
    cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "track_wide", "--", sys.executable, os.path.abspath(__file__),
           "--child", str(index), "--launches", str(launches)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    if p.returncode != 0:
        raise SystemExit("rocprofv3 ended with %d: %s" % (p.returncode, (p.stdout + p.stderr)[-1500:]))
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit("no kernel trace under %s" % d)
    times = {k: [] for k in KERNELS}
    for f in files:
        with open(f) as fh:
            for r in sorted(csv.DictReader(fh), key=lambda r: int(r["Start_Timestamp"])):
                for k in KERNELS:
                    if k in r["Kernel_Name"]:
                        times[k].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    shutil.rmtree(d, ignore_errors=True)
    rows, tracks = SHAPES[index]
    rec = {"rows": rows, "tracks": tracks, "launches": launches}
    for k, v in times.items():
        if v:
            assert len(v) >= launches, (k, len(v))
            v = v[-launches:]
            rec[k + "_us"] = round(statistics.median(v), 2)
            rec[k + "_us_min_max"] = [round(min(v), 2), round(max(v), 2)]
    rec["wide_update_us"] = round(rec["k_track_wide_cand_us"] + rec["k_track_wide_match_us"], 2)
    print(json.dumps(rec), flush=True)
    return rec


def tiled_fps(args):
    from bench_overlay import demo_cfg, load_synthetic
    from predictor import TiledPredictor
    h, w = FRAME_HW
    rng = np.random.default_rng(h)
    raws = [torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).cuda() for _ in range(3)]
    preds = {}
    for key, track in (("untracked_fps", None), ("tracked_fps", True)):
        preds[key] = TiledPredictor(demo_cfg(), track=track, tile=TILE, overlap=OVERLAP, fold=FOLD, max_detections=MAX_DET)
        load_synthetic(preds[key].model)

    def fps(pred):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(args.frames):
            pred(raws[i % len(raws)])
        torch.cuda.synchronize()
        return args.frames / (time.perf_counter() - t0)

    for pred in preds.values():
        fps(pred)
    got = {k: [] for k in preds}
    for _ in range(args.rounds):
        for k, pred in preds.items():
            got[k].append(fps(pred))
    out = preds["tracked_fps"](raws[0])["instances"]
    rec = {"frame_hw": [h, w], "tile": TILE, "overlap": OVERLAP, "fold": FOLD, "max_detections": MAX_DET, "detections": len(out),
           "tracks_started": preds["tracked_fps"].track_stats()["started"], "frames_per_round": args.frames, "rounds": args.rounds}
    for k, v in got.items():
        rec[k] = round(float(np.median(v)), 2)
        rec[k + "_round_spread"] = [round(float(min(v)), 2), round(float(max(v)), 2)]
    rec["tracking_cost_us_per_frame"] = round(1e6 / rec["tracked_fps"] - 1e6 / rec["untracked_fps"], 1)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200, help="timed updates per shape and tracker")
    ap.add_argument("--frames", type=int, default=20, help="frames per round of the tiled predictor")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=int, default=300, help="seconds one profiled child may take")
    ap.add_argument("--out", default="", help="also write the record to this file")
    ap.add_argument("--no-tiled", action="store_true", help="only the kernel times")
    ap.add_argument("--child", type=int, default=-1, help=argparse.SUPPRESS)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_track_wide needs the GPU"
    import orehip
    orehip.lib()
    if args.child >= 0:
        child(args.child, args.launches)
        return
    out = {"workload": "wide_detection_tracking", "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"),
           "ore_version": int(orehip.lib().ore_version()),
           "command": "python tools/bench_track_wide.py --launches %d --frames %d --rounds %d" % (args.launches, args.frames, args.rounds),
           "kernel_protocol": "rocprofv3 --kernel-trace, one run per shape; per kernel the median over the last `launches` launches",
           "kernels": [kernel_times(i, args.launches, args.limit) for i in range(len(SHAPES))],
           "tiled_predictor": None if args.no_tiled else tiled_fps(args)}
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
