"""Time the rectification (csrc/ore_rectify.hip, contract "rectify v1") and what it costs a predictor per frame.

  kernel     kernel time of k_rectify_u8 at 1080x1920 -> 1080x1920 and 2160x3840 -> 2160x3840, from rocprofv3 --kernel-trace in a run
             of its own (one child process per size, this file with --child): the median over the last `launches` launches, warmed.
             The homography is that of the quad (560, 300) (1360, 300) (1900, 1000) (20, 1000) of a 1080x1920 frame, scaled to the
             frame.  Before anything is timed the output is checked against rectify_host byte for byte.  Beside it, in this process and
             with events: the same launch, and a device-to-device copy of the output's bytes.  The kernel is a gather: it writes
             every output byte once and reads the source bytes under the quad through L2 and the Infinity Cache; the rate is stated as
             (output bytes + source bytes under the quad) / kernel time.
  default    DefaultPredictor ms per frame from host memory with rectify= and without, alternating round by round in one process.
  async      AsyncPredictor frames/s (inflight 4) from host memory with put(rectify=) and without, alternating likewise.

The detector is the synthetic-weight model of the test suite.  Prints one JSON line.

    python tools/bench_rectify.py [--launches 200] [--frames 300] [--rounds 5] [--out profiles/rectify_bench.json] [--no-predictors]
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

SIZES = [(1080, 1920), (2160, 3840)]
QUAD_1080 = [(560, 300), (1360, 300), (1900, 1000), (20, 1000)]


def rectifier(orehip, hw):
    s = hw[0] / 1080.0
    return orehip.Rectifier(quad=[(x * s, y * s) for x, y in QUAD_1080], out_hw=hw)


def quad_area(hw):
    """Source pixels under the quad (shoelace)."""
    s = hw[0] / 1080.0
    q = [(x * s, y * s) for x, y in QUAD_1080]
    return abs(sum(q[k][0] * q[(k + 1) % 4][1] - q[(k + 1) % 4][0] * q[k][1] for k in range(4))) / 2.0


def frame_of(hw):
    return np.random.default_rng(hw[0]).integers(0, 256, (*hw, 3), dtype=np.uint8)


def child(index, launches):
    """One size under the profiler: the check, then launches + 50 launches into one output."""
    import orehip
    hw = SIZES[index]
    R = rectifier(orehip, hw)
    img = frame_of(hw)
    dev = torch.from_numpy(img).cuda()
    out = R(dev)
    torch.cuda.synchronize()
    equal = bool(np.array_equal(out.cpu().numpy(), R(img)))
    print(json.dumps({"frame_hw": list(hw), "equals_rectify_host": equal}), flush=True)
    if not equal:
        sys.exit("the device output differs from rectify_host")
    for _ in range(launches + 50):
        R(dev, out=out)
    torch.cuda.synchronize()


def kernel_time(index, launches, limit):
    d = os.path.join(ROOT, "profiles", f"rectify_trace_{index}")
    shutil.rmtree(d, ignore_errors=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "rectify", "--", sys.executable,
           os.path.abspath(__file__), "--child", str(index), "--launches", str(launches)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    if p.returncode != 0:
        raise SystemExit("rocprofv3 ended with %d: %s" % (p.returncode, (p.stdout + p.stderr)[-1500:]))
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit("no kernel trace under %s" % d)
    times = []
    for f in files:
        with open(f) as fh:
            for r in sorted(csv.DictReader(fh), key=lambda r: int(r["Start_Timestamp"])):
                if "k_rectify_u8" in r["Kernel_Name"]:
                    times.append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    shutil.rmtree(d, ignore_errors=True)
    assert len(times) >= launches, len(times)
    times = times[-launches:]
    hw = SIZES[index]
    med = statistics.median(times)
    out_bytes, src_bytes = hw[0] * hw[1] * 3, int(quad_area(hw) * 3)
    rec = {"frame_hw": list(hw), "out_hw": list(hw), "launches": launches, "equals_rectify_host": '"equals_rectify_host": true' in p.stdout,
           "k_rectify_u8_us": round(med, 2), "k_rectify_u8_us_min_max": [round(min(times), 2), round(max(times), 2)],
           "output_bytes": out_bytes, "source_bytes_under_quad": src_bytes,
           "bytes_per_s": round((out_bytes + src_bytes) / (med * 1e-6), -6)}
    return rec


def event_side(orehip, rec, launches, rounds):
    """In this process, with events: the launch itself and a device copy of the output's bytes."""
    from bench_overlay import event_us
    hw = tuple(rec["frame_hw"])
    R = rectifier(orehip, hw)
    dev = torch.from_numpy(frame_of(hw)).cuda()
    out = R(dev)
    other = torch.empty_like(out)
    rec["rectify_event_us"], rec["rectify_event_round_spread_us"] = event_us(lambda: R(dev, out=out), launches, rounds)
    rec["copy_of_output_event_us"], rec["copy_of_output_round_spread_us"] = event_us(lambda: other.copy_(out), launches, rounds)
    rec["copy_bytes_per_s"] = round(2 * out.numel() / (rec["copy_of_output_event_us"] * 1e-6), -6)
    rec["kernel_over_copy"] = round(rec["k_rectify_u8_us"] / rec["copy_of_output_event_us"], 2)
    for k in ("rectify_event_us", "copy_of_output_event_us"):
        rec[k] = round(rec[k], 2)
    for k in ("rectify_event_round_spread_us", "copy_of_output_round_spread_us"):
        rec[k] = [round(v, 2) for v in rec[k]]
    return rec


def rounds_of(fns, rounds):
    """Every function once to warm up, then `rounds` rounds of all of them in turn: {key: median, key_round_spread: [min, max]}."""
    for fn in fns.values():
        fn()
    got = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            got[k].append(fn())
    rec = {}
    for k, v in got.items():
        rec[k] = round(float(np.median(v)), 3)
        rec[k + "_round_spread"] = [round(float(min(v)), 3), round(float(max(v)), 3)]
    return rec


def predictor_cases(orehip, args):
    from bench_overlay import demo_cfg, load_synthetic, loop_ms
    from detectron2.engine.defaults import DefaultPredictor
    from predictor import AsyncPredictor
    pred = DefaultPredictor(demo_cfg())
    load_synthetic(pred.model)
    ap = AsyncPredictor(demo_cfg(), inflight=4)
    load_synthetic(ap.model)
    out = {"default_predictor": [], "async_predictor": []}

    def with_rectify(R, frames):
        pred.rectify = R
        try:
            return loop_ms(pred, frames)
        finally:
            pred.rectify = None

    def fps(R, frames):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for f in frames:
            if len(ap) == ap.default_buffer_size:
                ap.get()
            ap.put(f, rectify=R)
        while len(ap):
            ap.get()
        torch.cuda.synchronize()
        return len(frames) / (time.perf_counter() - t0)

    try:
        for hw in SIZES:
            R = rectifier(orehip, hw)
            rng = np.random.default_rng(hw[1])
            frames = [rng.integers(0, 256, (*hw, 3), dtype=np.uint8) for _ in range(3)] * (args.frames // 3 + 1)
            frames = frames[:args.frames]
            rec = rounds_of({"plain_ms": lambda: with_rectify(None, frames), "rectified_ms": lambda: with_rectify(R, frames)}, args.rounds)
            rec.update(frame_hw=list(hw), frames_per_round=args.frames, rounds=args.rounds,
                       rectify_cost_ms_per_frame=round(rec["rectified_ms"] - rec["plain_ms"], 3))
            out["default_predictor"].append(rec)
            many = frames * 3
            rec = rounds_of({"plain_fps": lambda: fps(None, many), "rectified_fps": lambda: fps(R, many)}, args.rounds)
            rec.update(frame_hw=list(hw), frames_per_round=len(many), rounds=args.rounds, inflight=ap.default_buffer_size,
                       rectify_cost_ms_per_frame=round(1e3 / rec["rectified_fps"] - 1e3 / rec["plain_fps"], 3))
            out["async_predictor"].append(rec)
    finally:
        ap.shutdown()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200, help="timed launches per size")
    ap.add_argument("--frames", type=int, default=300, help="frames per round of DefaultPredictor (AsyncPredictor: three times as many)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=int, default=300, help="seconds one profiled child may take")
    ap.add_argument("--out", default="", help="also write the record to this file")
    ap.add_argument("--no-predictors", action="store_true", help="only the kernel times")
    ap.add_argument("--child", type=int, default=-1, help=argparse.SUPPRESS)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_rectify needs the GPU"
    import orehip
    orehip.lib()
    if args.child >= 0:
        child(args.child, args.launches)
        return
    # the profiled children first: this process opens the GPU only after they have ended
    kernels = [kernel_time(i, args.launches, args.limit) for i in range(len(SIZES))]
    out = {"workload": "rectify", "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"),
           "ore_version": int(orehip.lib().ore_version()),
           "command": "python tools/bench_rectify.py --launches %d --frames %d --rounds %d" % (args.launches, args.frames, args.rounds),
           "kernel_protocol": "rocprofv3 --kernel-trace --stats, one run per size; the median over the last `launches` launches; the copy "
                              "and rectify_event_us are event-timed loops in the parent process",
           "kernels": [event_side(orehip, k, args.launches, args.rounds) for k in kernels]}
    out.update({"default_predictor": None, "async_predictor": None} if args.no_predictors else predictor_cases(orehip, args))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
