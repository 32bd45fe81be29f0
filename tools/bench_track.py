"""Time the detection tracker (csrc/ore_track.hip, association contract "track v1") on the device.

  update       ore_track_update_fwd alone at three shapes -- 100 rows on 150 tracks (typical), 320 rows on 1024 tracks (full), and the
               chain of tests/track_ref.py scaled to 320 rows on 320 tracks (one pair per mutual-best round: the worst case) -- as the
               median over rounds of the mean of `launches` back-to-back calls between two device events, after a warm-up.  Every call
               of a shape starts from the same state (the state buffer is restored by a device copy inside the timed loop; the copy
               alone is timed the same way and subtracted) and its ids are checked against track_host once before anything is timed.
               track_host on the same rows, for scale.
  async        AsyncPredictor frames/s at 480x640 and 1080x1920, inflight 4: boxes only against boxes + tracking, alternating round by
               round in the same process (as tools/bench_overlay.py does for drawing)

The detector is the synthetic-weight model of the test suite.  Prints one JSON line.

    python tools/bench_track.py [--frames 64] [--rounds 5] [--launches 400] [--out profiles/track_bench.json] [--kernel-only]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "faster-orefsdet_amd"), ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

FRAME_SIZES = [(480, 640), (1080, 1920)]


def drifting(rows, tracks, seed):
    """Two frames: `tracks` boxes, then `rows` of them moved by a pixel or two, in another order -- every row continues a track."""
    rng = np.random.default_rng(seed)
    n = max(rows, tracks)
    cell = np.arange(n)                                      # one box per 100 x 100 cell of a 32-wide grid: no two tracks overlap
    x0, y0 = (cell % 32) * 100.0 + rng.uniform(0, 15, n), (cell // 32) * 100.0 + rng.uniform(0, 15, n)
    b = np.stack([x0, y0, x0 + rng.uniform(40, 80, n), y0 + rng.uniform(40, 80, n)], 1).astype(np.float32)
    pick = rng.permutation(n)[:rows]
    b1 = (b[pick] + rng.uniform(-1, 1, (rows, 4))).astype(np.float32)
    s = lambda k: rng.uniform(0.3, 1.0, k).astype(np.float32)
    return [(b[:tracks], s(tracks), np.zeros(tracks, np.int64)), (b1, s(rows), np.zeros(rows, np.int64))]


def shapes():
    import track_ref as TR
    chain = [(b, s, c) for b, s, c, _ in TR.chain_case(320)]
    return [("typical", 100, 150, 0.6, None), ("full", 320, 1024, 0.6, None), ("chain", 320, 320, TR.CHAIN_IOU_THRESH, chain)]


def event_us(fn, launches, rounds):
    for _ in range(max(launches // 4, 10)):
        fn()
    per = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        torch.cuda.synchronize()
        per.append(a.elapsed_time(b) * 1e3 / launches)
    return float(np.median(per)), [float(min(per)), float(max(per))]


def prime(orehip, tr, seed_frames):
    """The tracker brought to the state in front of the timed frame: frames of at most 320 rows each."""
    tr.reset()
    b, s, c = seed_frames
    for i in range(0, len(s), 320):
        tr.update(torch.from_numpy(b[i:i + 320]).cuda(), torch.from_numpy(s[i:i + 320]).cuda(), torch.from_numpy(c[i:i + 320]).cuda())


def update_cases(orehip, args):
    out = []
    for name, rows, tracks, thr, frames in shapes():
        frames = frames or drifting(rows, tracks, rows)
        tr = orehip.BoxTracker("cuda", iou_thresh=thr)
        prime(orehip, tr, frames[0])
        before = tr.state_host()
        assert before["m"] == tracks, (before["m"], tracks)
        saved = tr._buf.clone()
        b, s, c = (torch.from_numpy(a).cuda() for a in frames[1])
        ids = torch.empty(rows, dtype=torch.int64, device="cuda")
        t0 = time.perf_counter()
        want, _ = orehip.track_host(before, *frames[1], iou_thresh=thr)
        host_ms = (time.perf_counter() - t0) * 1e3
        tr.update(b, s, c, out=ids)
        assert np.array_equal(ids.cpu().numpy(), want), name

        def restore():
            tr._buf.copy_(saved)

        def both():
            tr._buf.copy_(saved)
            tr.update(b, s, c, out=ids)

        copy_us, _ = event_us(restore, args.launches, args.rounds)
        both_us, spread = event_us(both, args.launches, args.rounds)
        out.append({"shape": name, "rows": rows, "tracks": tracks, "iou_thresh": thr, "matched": int((want >= 0).sum()), "equals_track_host": True,
                    "restore_and_update_us": both_us, "restore_and_update_round_spread_us": spread, "restore_copy_us": copy_us,
                    "update_us": both_us - copy_us, "track_host_ms": host_ms})
    return out


def async_fps(ap, images, tracker):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pending = 0
    for img in images:
        if pending == ap.default_buffer_size:
            ap.get()
            pending -= 1
        ap.put(img, track=tracker)
        pending += 1
    while pending:
        ap.get()
        pending -= 1
    torch.cuda.synchronize()
    return len(images) / (time.perf_counter() - t0)


def predictor_cases(orehip, args):
    from bench_overlay import demo_cfg, load_synthetic
    from predictor import AsyncPredictor
    ap = AsyncPredictor(demo_cfg(), inflight=4)
    load_synthetic(ap.model)
    tracker = orehip.BoxTracker(ap.model.device)
    out = []
    for h, w in FRAME_SIZES:
        rng = np.random.default_rng(h + 1)
        raws = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(4)]
        images = [raws[i % len(raws)] for i in range(args.frames)]
        rates = {"boxes_fps": lambda: async_fps(ap, images, None), "boxes_tracked_fps": lambda: async_fps(ap, images, tracker)}
        for fn in rates.values():
            fn()
        fps = {k: [] for k in rates}
        for _ in range(args.rounds):
            for k, fn in rates.items():
                fps[k].append(fn())
        rec = {"frame_hw": [h, w], "inflight": 4, "detections": len(ap(raws[0])["instances"])}
        for k, v in fps.items():
            rec[k] = float(np.median(v))
            rec[k + "_round_spread"] = [float(np.min(v)), float(np.max(v))]
        rec["tracking_cost_us_per_frame"] = 1e6 / rec["boxes_tracked_fps"] - 1e6 / rec["boxes_fps"]
        out.append(rec)
    ap.shutdown()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64, help="frames per round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=400, help="update calls between the two events (>= 200)")
    ap.add_argument("--out", default="", help="also write the record to this file")
    ap.add_argument("--kernel-only", action="store_true", help="only the update calls (for a kernel-trace run of a profiler)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_track needs the GPU"
    assert args.launches >= 200
    import orehip
    orehip.lib()
    out = {"workload": "detection_tracking", "device": torch.cuda.get_device_name(0), "host_cpus_used": len(os.sched_getaffinity(0)),
           "date": time.strftime("%Y-%m-%d"), "frames_per_round": args.frames, "rounds": args.rounds, "launches": args.launches,
           "command": "python tools/bench_track.py" + "".join(f" --{k} {v}" for k, v in (("frames", args.frames), ("rounds", args.rounds),
                                                                                           ("launches", args.launches))),
           "update": update_cases(orehip, args), "predictors": [] if args.kernel_only else predictor_cases(orehip, args)}
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
