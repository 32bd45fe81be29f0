"""Time the belt's shift (csrc/ore_belt.hip, contract "belt shift v1") beside the tracker update it precedes.

  kernels   kernel time of one shift at (rows, tracks) = (320, 1024), (2000, 3000) and (8192, 16384), from rocprofv3 --kernel-trace in
            runs of their own (one child process per shape, this file with --child): per kernel the median over the timed launches.
            Form 1 (k_belt_one) at the first shape; form 2 (k_belt_vote<false>: per-block LDS histograms, one global add per non-zero
            bin and block; k_belt_finish) and form 3 (k_belt_vote<true>: every vote a global atomic) at all three.  The tracker's
            update (k_track_update at the first shape, k_track_wide_cand + k_track_wide_match beyond) runs behind every shift in the
            same child, so the shift is stated as a fraction of the update it precedes.  The scene: one box per 100 x 100 cell, every
            row a track moved by (36, 2) and a pixel of jitter, so every row is a true pair and the neighbours within the window of
            128 px are the false ones.  Every call starts from the same two states (device copies restore them).  Before anything is
            timed the forms are checked against each other byte for byte, and against belt_shift_host at the first two shapes.
  async     AsyncPredictor frames/s with put(track=BoxTracker) and put(track=BeltTracker), alternating round by round in one process,
            the profiler off.
  tiled     TiledPredictor frames/s on a 2160x3840 frame (tile 640, overlap 128, fold 8, max_detections 2000) with a WideBoxTracker and
            with a WideBeltTracker, alternating likewise.

The detector is the synthetic-weight model of the test suite.  Prints one JSON line.

    python tools/bench_belt.py [--launches 200] [--frames 20] [--rounds 5] [--out profiles/belt_bench.json] [--no-predictors]
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
# the name in the trace (demangled, or mangled) -> the record's key
KERNELS = {"k_belt_one": ("k_belt_one",), "k_belt_vote_lds": ("k_belt_vote<false>", "k_belt_voteILb0E"),
           "k_belt_vote_direct": ("k_belt_vote<true>", "k_belt_voteILb1E"), "k_belt_finish": ("k_belt_finish",),
           "k_track_update": ("k_track_update",), "k_track_wide_cand": ("k_track_wide_cand",), "k_track_wide_match": ("k_track_wide_match",)}
FRAME_HW, TILE, OVERLAP, FOLD, MAX_DET = (2160, 3840), 640, 128, 8, 2000
SHIFT = (36, 2)


def belt_scene(rows, tracks, seed):
    """`tracks` disjoint boxes (one per 100 x 100 cell), and `rows` of them moved by SHIFT and up to a pixel, in another order."""
    rng = np.random.default_rng(seed)
    cell = np.arange(tracks)
    x0, y0 = (cell % 128) * 100.0 + rng.uniform(0, 15, tracks), (cell // 128) * 100.0 + rng.uniform(0, 15, tracks)
    b = np.stack([x0, y0, x0 + rng.uniform(40, 80, tracks), y0 + rng.uniform(40, 80, tracks)], 1).astype(np.float32)
    pick = rng.permutation(tracks)[:rows]
    b1 = (b[pick] + np.array([SHIFT[0], SHIFT[1]] * 2) + rng.uniform(-1, 1, (rows, 4))).astype(np.float32)
    s = lambda k: rng.uniform(0.3, 1.0, k).astype(np.float32)
    return (b, s(tracks), np.zeros(tracks, np.int64)), (b1, s(rows), np.zeros(rows, np.int64))


def child(index, launches):
    """One shape under the profiler: per form `launches` timed (restore, shift, update) rounds."""
    import orehip
    from bench_track_wide import primed
    L = orehip.lib()
    rows, tracks = SHAPES[index]
    f0, f1 = belt_scene(rows, tracks, rows)
    kw = dict(capacity=tracks, bin=2, radius=128)
    tr = orehip.BeltTracker("cuda", **kw) if index == 0 else orehip.WideBeltTracker("cuda", max_rows=rows, **kw)
    tr._before_update = lambda *a, **k: None                   # here the shift is launched by hand, one form at a time
    primed(tr, f0, rows)
    before = tr.state_host()
    belt0 = before.pop("belt")
    assert before["m"] == tracks, (before["m"], tracks)
    saved, saved_belt = tr._buf.clone(), tr._belt.clone()
    ws = torch.empty(int(L.ore_belt_workspace_bytes(tracks, rows, 64)), dtype=torch.uint8, device="cuda")
    b, s, c = (torch.from_numpy(a).cuda() for a in f1)
    ids = torch.empty(rows, dtype=torch.int64, device="cuda")
    p, t = tr.belt_params, tr.params

    def shift(form):
        rc = L.ore_belt_shift_fwd(tr._belt.data_ptr(), tr._buf.data_ptr(), tracks, b.data_ptr(), s.data_ptr(), c.data_ptr(), None, rows, rows,
                                  float(t["score_thresh"]), 1, p["bin"], p["half_bins"], float(p["size_tol"]), p["min_votes"], 0, 0, form,
                                  ws.data_ptr(), ws.numel(), None)
        assert rc == 0, L.ore_last_error()

    forms = (1, 2, 3) if index == 0 else (2, 3)
    got = []
    for form in forms:
        tr._buf.copy_(saved)
        tr._belt.copy_(saved_belt)
        shift(form)
        torch.cuda.synchronize()
        got.append((tr._buf.cpu().numpy().copy(), tr._belt.cpu().numpy().copy()))
    assert all(np.array_equal(g[0], got[0][0]) and np.array_equal(g[1], got[0][1]) for g in got[1:]), "the forms disagree"
    votes = int(got[0][1][8:12].view(np.int32)[0])
    assert abs(int(got[0][1][:4].view(np.int32)[0]) - SHIFT[0]) <= 2 and votes > rows // 2, (got[0][1][:12].view(np.int32), rows)
    if index < 2:
        moved, belt = orehip.belt_shift_host(before, belt0, *f1, bin=2, half_bins=64)
        assert belt["votes"] == votes and np.array_equal(got[0][0][32:32 + 16 * tracks].view(np.float32).reshape(-1, 4), moved["boxes"])
    print(json.dumps({"rows": rows, "tracks": tracks, "votes_in_peak": votes}), flush=True)
    for form in forms:
        for _ in range(launches + 10):                          # the parent takes the last `launches` of each kernel
            tr._buf.copy_(saved)
            tr._belt.copy_(saved_belt)
            shift(form)
            tr.update(b, s, c, out=ids)
    torch.cuda.synchronize()


def kernel_times(index, launches, limit):
    d = os.path.join(ROOT, "profiles", f"belt_trace_{index}")
    shutil.rmtree(d, ignore_errors=True)
    cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "belt", "--", sys.executable, os.path.abspath(__file__),
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
                for k, names in KERNELS.items():
                    if any(nm in r["Kernel_Name"] for nm in names):
                        times[k].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    shutil.rmtree(d, ignore_errors=True)
    rows, tracks = SHAPES[index]
    rec = {"rows": rows, "tracks": tracks, "launches": launches}
    for line in p.stdout.splitlines():
        if line.startswith('{"rows"'):
            rec["votes_in_peak"] = json.loads(line)["votes_in_peak"]
    med = {}
    for k, v in times.items():
        if v:
            assert len(v) >= launches, (k, len(v))
            v = v[-launches:] if k != "k_belt_finish" else v    # the finish runs behind both vote kernels
            med[k] = statistics.median(v)
            rec[k + "_us"] = round(med[k], 2)
            rec[k + "_us_min_max"] = [round(min(v), 2), round(max(v), 2)]
    update = med["k_track_update"] if index == 0 else med["k_track_wide_cand"] + med["k_track_wide_match"]
    rec["update_us"] = round(update, 2)
    if "k_belt_one" in med:
        rec["form1_us"] = round(med["k_belt_one"], 2)
        rec["form1_fraction_of_update"] = round(med["k_belt_one"] / update, 3)
    rec["form2_us"] = round(med["k_belt_vote_lds"] + med["k_belt_finish"], 2)
    rec["form2_fraction_of_update"] = round(rec["form2_us"] / update, 3)
    rec["form3_direct_atomics_us"] = round(med["k_belt_vote_direct"] + med["k_belt_finish"], 2)
    print(json.dumps(rec), flush=True)
    return rec


def rounds_of(fps_fns, rounds):
    """Every function once to warm up, then `rounds` rounds of all of them in turn: {key: median, key_round_spread: [min, max]}."""
    for fn in fps_fns.values():
        fn()
    got = {k: [] for k in fps_fns}
    for _ in range(rounds):
        for k, fn in fps_fns.items():
            got[k].append(fn())
    rec = {}
    for k, v in got.items():
        rec[k] = round(float(np.median(v)), 2)
        rec[k + "_round_spread"] = [round(float(min(v)), 2), round(float(max(v)), 2)]
    return rec


def async_fps(args):
    import orehip
    from bench_overlay import demo_cfg, load_synthetic
    from predictor import AsyncPredictor
    h, w = 720, 1280
    rng = np.random.default_rng(w)
    raws = [torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).cuda() for _ in range(3)]
    ap = AsyncPredictor(demo_cfg())
    load_synthetic(ap.model)
    trackers = {"box_tracker_fps": orehip.BoxTracker(ap.model.device), "belt_tracker_fps": orehip.BeltTracker(ap.model.device, frame=(h, w))}
    frames = args.frames * 5

    def fps(tracker):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(frames):
            if len(ap) == ap.default_buffer_size:
                ap.get()
            ap.put(raws[i % len(raws)], track=tracker)
        while len(ap):
            ap.get()
        torch.cuda.synchronize()
        return frames / (time.perf_counter() - t0)

    try:
        rec = rounds_of({k: (lambda t=t: fps(t)) for k, t in trackers.items()}, args.rounds)
    finally:
        ap.shutdown()
    rec.update(frame_hw=[h, w], frames_per_round=frames, rounds=args.rounds, inflight=ap.default_buffer_size,
               shift_cost_us_per_frame=round(1e6 / rec["belt_tracker_fps"] - 1e6 / rec["box_tracker_fps"], 1))
    return rec


def tiled_fps(args):
    import orehip
    from bench_overlay import demo_cfg, load_synthetic
    from predictor import TiledPredictor
    h, w = FRAME_HW
    rng = np.random.default_rng(h)
    raws = [torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).cuda() for _ in range(3)]
    kw = dict(capacity=2 * MAX_DET, max_rows=MAX_DET)
    preds = {}
    for key, tracker in (("wide_box_tracker_fps", orehip.WideBoxTracker("cuda", **kw)), ("wide_belt_tracker_fps", orehip.WideBeltTracker("cuda", frame=(h, w), **kw))):
        preds[key] = TiledPredictor(demo_cfg(), track=tracker, tile=TILE, overlap=OVERLAP, fold=FOLD, max_detections=MAX_DET)
        load_synthetic(preds[key].model)

    def fps(pred):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(args.frames):
            pred(raws[i % len(raws)])
        torch.cuda.synchronize()
        return args.frames / (time.perf_counter() - t0)

    rec = rounds_of({k: (lambda p=p: fps(p)) for k, p in preds.items()}, args.rounds)
    out = preds["wide_belt_tracker_fps"](raws[0])["instances"]
    rec.update(frame_hw=[h, w], tile=TILE, overlap=OVERLAP, fold=FOLD, max_detections=MAX_DET, detections=len(out), frames_per_round=args.frames,
               rounds=args.rounds, shift_cost_us_per_frame=round(1e6 / rec["wide_belt_tracker_fps"] - 1e6 / rec["wide_box_tracker_fps"], 1))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200, help="timed shifts per shape and form")
    ap.add_argument("--frames", type=int, default=20, help="frames per round of the tiled predictor (the async predictor: five times as many)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=int, default=300, help="seconds one profiled child may take")
    ap.add_argument("--out", default="", help="also write the record to this file")
    ap.add_argument("--no-predictors", action="store_true", help="only the kernel times")
    ap.add_argument("--child", type=int, default=-1, help=argparse.SUPPRESS)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_belt needs the GPU"
    import orehip
    orehip.lib()
    if args.child >= 0:
        child(args.child, args.launches)
        return
    out = {"workload": "belt_shift", "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"),
           "ore_version": int(orehip.lib().ore_version()),
           "command": "python tools/bench_belt.py --launches %d --frames %d --rounds %d" % (args.launches, args.frames, args.rounds),
           "kernel_protocol": "rocprofv3 --kernel-trace, one run per shape; per kernel the median over the last `launches` launches",
           "kernels": [kernel_times(i, args.launches, args.limit) for i in range(len(SHAPES))],
           "async_predictor": None if args.no_predictors else async_fps(args),
           "tiled_predictor": None if args.no_predictors else tiled_fps(args)}
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
