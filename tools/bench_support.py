"""Time the support crops (csrc/ore_support.hip, "support crop v1") and CenterNet2Detector.enrol on the device.

  crops        one ore_support_crop_u8_fwd call between device events -- the median over rounds of the mean of `launches`
               back-to-back calls between two events, after a warm-up, on a job buffer planned and uploaded once -- for (a) 25 small
               boxes of one 1080x1920 frame, every job of the LDS form (one launch), and (b) 4 boxes that cover most of that frame,
               every job of the workspace form (two launches).  This is the pace of back-to-back calls: it includes the launcher's
               host checks and the submission, so it bounds the kernel time from above; the kernel time itself comes from a
               profiler's kernel trace in a run of its own (below).  The crops are checked against tests/support_ref.py (Pillow)
               before anything is timed.  orehip.support_crops as a whole (plan, upload, launch; host clock around a synchronise).
  enrol        wall time of model.enrol(frame, 25 boxes) against the host composition run alternately in the same process: Pillow
               crops by tests/support_ref.py, then compute_support_dict on them.  Both end in a device synchronise.

The detector is the synthetic-weight model of the test suite.  Prints one JSON line.

    python tools/bench_support.py [--rounds 5] [--launches 2000] [--out profiles/support_bench.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_support.py --kernel-only      (kernel times, a run of its own)
    python tools/bench_support.py --summarise-trace DIR > profiles/support_kernel_stats.txt     (that run, per kernel and grid)
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

FRAME_HW = (1080, 1920)


def small_boxes(n, seed):
    """n boxes with sides of 40 .. 160 pixels anywhere in the frame (some overhang it)."""
    rng = np.random.default_rng(seed)
    h, w = FRAME_HW
    bw, bh = rng.uniform(40, 160, n), rng.uniform(40, 160, n)
    cx, cy = rng.uniform(20, w - 20, n), rng.uniform(20, h - 20, n)
    return np.stack([cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2], 1).astype(np.float32)


def large_boxes():
    h, w = FRAME_HW
    return np.array([[0, 0, w, h], [100, 40, w - 200, h - 30], [400, 0, w, h], [0, 100, 1500, 1000]], dtype=np.float32)


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


def wall_ms(fn, rounds):
    per = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        per.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(per)), [float(min(per)), float(max(per))]


def crop_cases(orehip, frame, args):
    import support_ref as SR
    L = orehip.lib()
    dev_frame = torch.from_numpy(frame).cuda()
    out = []
    for name, boxes, form in (("25_small_boxes", small_boxes(25, 1), orehip.RESIZE_FORM_LDS), ("4_large_boxes", large_boxes(), orehip.RESIZE_FORM_WORKSPACE)):
        forms = [orehip.support_crop_form(*FRAME_HW, b) for b in boxes]
        assert all(f == form for f in forms), (name, forms)
        K = len(boxes)
        crops, sboxes = orehip.support_crops(dev_frame, boxes)
        want, wboxes = SR.crops([frame], boxes)
        assert np.array_equal(crops.cpu().numpy(), want) and np.array_equal(sboxes.numpy(), wboxes), name
        st = orehip._SUPPORT_BUF[(str(dev_frame.device), orehip._stream())]               # the buffers that call planned and uploaded
        total = K * orehip.SUPPORT_JOB_INTS + sum(int(L.ore_support_crop_job_ints(*FRAME_HW, b.ctypes.data, 240, 16)) for b in boxes)
        ws_bytes = sum(int(L.ore_support_crop_workspace_bytes(*FRAME_HW, b.ctypes.data, 240, 16)) for b in boxes)
        fill = orehip.SUPPORT_FILL[0] | orehip.SUPPORT_FILL[1] << 8 | orehip.SUPPORT_FILL[2] << 16
        jobs_dev, jobs_host, ws, dst, stream = st["dev"].data_ptr(), st["last"]["host"].data_ptr(), st["ws"].data_ptr() if ws_bytes else None, crops.data_ptr(), orehip._stream()

        def launch():
            rc = L.ore_support_crop_u8_fwd(jobs_dev, jobs_host, total, K, 240, fill, dst, ws, ws_bytes, stream)
            assert rc == 0, rc

        us, spread = event_us(launch, args.launches, args.rounds)
        assert np.array_equal(crops.cpu().numpy(), want), name
        call_ms, call_spread = wall_ms(lambda: orehip.support_crops(dev_frame, boxes), max(args.rounds, 20))
        out.append({"case": name, "crops": K, "frame_hw": list(FRAME_HW), "form": "lds" if form == orehip.RESIZE_FORM_LDS else "workspace",
                    "launches_per_call": 1 if form == orehip.RESIZE_FORM_LDS else 2, "equals_pillow": True, "events_us_per_call": us,
                    "events_us_round_spread": spread, "support_crops_call_wall_ms": call_ms, "support_crops_call_wall_spread_ms": call_spread})
    return out


def enrol_case(orehip, frame, args):
    import support_ref as SR
    from bench_overlay import demo_cfg, load_synthetic
    from detectron2.modeling import build_model
    cfg = demo_cfg()
    cfg.freeze()
    model = load_synthetic(build_model(cfg))
    boxes = small_boxes(25, 2)

    def device():
        model.enrol(frame, boxes, cls_id=1)

    def host():
        crops, sboxes = SR.crops([frame], boxes)
        model.compute_support_dict(torch.from_numpy(crops), torch.from_numpy(sboxes), cls_id=1, merge=True)

    for fn in (device, host, device, host):
        fn()
    ms = {"enrol_ms": [], "host_composition_ms": []}
    for _ in range(args.rounds):
        ms["enrol_ms"].append(wall_ms(device, 1)[0])
        ms["host_composition_ms"].append(wall_ms(host, 1)[0])
    t0 = time.perf_counter()
    SR.crops([frame], boxes)
    pillow_ms = (time.perf_counter() - t0) * 1e3
    rec = {"shots": 25, "frame_hw": list(FRAME_HW), "frame": "host numpy array (uploaded by the call)", "pillow_crops_alone_ms": pillow_ms}
    for k, v in ms.items():
        rec[k] = float(np.median(v))
        rec[k + "_round_spread"] = [float(min(v)), float(max(v))]
    return rec


def summarise_trace(d):
    """Per kernel name and grid of a rocprofv3 --kernel-trace run of `--kernel-only`: launches and the median / min / max duration.
    The grid's z tells the cases apart: 25 jobs or 4."""
    import collections
    import csv
    import glob
    files = glob.glob(os.path.join(d, "**", "*_kernel_trace.csv"), recursive=True)
    assert files, f"no *_kernel_trace.csv under {d}"
    per = collections.defaultdict(list)
    for r in csv.DictReader(open(files[0])):
        name = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        if "k_support" in name:
            grid = tuple(int(r[f"Grid_Size_{a}"]) // int(r[f"Workgroup_Size_{a}"]) for a in "XYZ")
            per[(name, grid)].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    print(f"{'kernel':20s} {'grid (blocks)':>18s} {'launches':>9s} {'median us':>10s} {'min us':>8s} {'max us':>8s}")
    for (name, grid), v in sorted(per.items()):
        print(f"{name:20s} {str(grid):>18s} {len(v):9d} {float(np.median(v)):10.2f} {min(v):8.2f} {max(v):8.2f}")


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--summarise-trace":
        return summarise_trace(sys.argv[2])
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=2000, help="launch calls between the two events (>= 200)")
    ap.add_argument("--kernel-only", action="store_true", help="only the crop calls (for a kernel-trace run of a profiler)")
    ap.add_argument("--out", default="", help="also write the record to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_support needs the GPU"
    assert args.launches >= 200
    import orehip
    orehip.lib()
    frame = np.random.default_rng(7).integers(0, 256, (*FRAME_HW, 3), dtype=np.uint8)
    out = {"workload": "support_crops_and_enrolment", "device": torch.cuda.get_device_name(0), "host_cpus_used": len(os.sched_getaffinity(0)),
           "date": time.strftime("%Y-%m-%d"), "rounds": args.rounds, "launches": args.launches,
           "command": f"python tools/bench_support.py --rounds {args.rounds} --launches {args.launches}",
           "crops": crop_cases(orehip, frame, args), "enrol": None if args.kernel_only else enrol_case(orehip, frame, args)}
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
