#!/usr/bin/env python3
"""N-way inference (include/ore_hip.h, ore_engine_set_classes) against the workaround it replaces: at 640 x 640, fp32, synthetic seeded
weights and supports (as the tests make them), for K support classes

  nway      ONE engine with K class slots: Engine.detect_classes(img, 640, 640) + torch.cuda.synchronize() per call (the reference
            protocol's per-image pattern) -- backbone + FPN once, correlation .. second stage per class, merge;
  singles   K single-class engines in the same process: K back-to-back Engine.detect(img, 640, 640) calls + synchronize.

Prints and writes one JSON object: per K the median ms per call of both, their ratio, and the kernel launches of one eager N-way pass
(torch.profiler kernel events; --no-launch-count under an outside profiler).

    python3 tools/bench_nway.py [--k 1 2 4 8] [--iters 50] [--warmup 10] [--out profiles/nway_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "faster-orefsdet_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import orehip  # noqa: E402
from oracle import ref_model as R  # noqa: E402

H = W = 640
REG = (10.0, 10.0, 5.0, 5.0)


def supports(n):
    out = []
    for k in range(n):
        rc8 = torch.randn(6, 128, 8, 8, generator=torch.Generator().manual_seed(40 + k)) * 0.1
        out.append((R.synth_support(10 + k), rc8))
    return out


def single_engine(sd, roi_sd, sup):
    e = orehip.Engine(max_batch=1, max_h=H, max_w=W)
    e.load_state_dict(sd)
    e.set_support(sup[0])
    e.finalize()
    e.set_roi_head(roi_sd, sup[1], REG, 0.05, 0.9, 100)
    return e


def nway_engine(sd, roi_sd, sups):
    e = orehip.Engine(max_batch=len(sups), max_h=H, max_w=W)
    e.load_state_dict(sd)
    e.finalize()
    e.set_roi_head(roi_sd, sups[0][1], REG, 0.05, 0.9, 100)
    e.set_classes(list(range(len(sups))))
    for k, (p, rc8) in enumerate(sups):
        e.set_support(p, slot=k)
        e.set_roi_support(roi_sd, rc8, slot=k)
    return e


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
        torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts)


def launches(e, img):
    """Kernel launches of one EAGER N-way pass (the replayed graph holds the same kernels)."""
    from torch.profiler import ProfilerActivity, profile
    e.eval_classes_forward(img, use_graph=False)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        e.eval_classes_forward(img, use_graph=False)
        torch.cuda.synchronize()
    return sum(1 for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA and "emcpy" not in ev.name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-launch-count", action="store_true")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    sd = R.synth_state_dict(0)
    roi_sd = R.synth_roi_state(sd, 0)
    roi_sd["roi_heads.box_head.0.fc1.weight"] = roi_sd["roi_heads.box_head.0.fc1.weight"] * 0.01
    kmax = max(a.k)
    sups = supports(kmax)
    img = R.synth_image(3, H, W).cuda()
    singles = [single_engine(sd, roi_sd, s) for s in sups]
    rows = []
    for K in a.k:
        e = nway_engine(sd, roi_sd, sups[:K])
        nway_ms, nway_min = timed(lambda: e.detect_classes(img, H, W), a.iters, a.warmup)

        def run_singles():
            for s in singles[:K]:
                s.detect(img, H, W)
        single_ms, single_min = timed(run_singles, a.iters, a.warmup)
        n_det = int(e.detect_classes(img, H, W)[1].numel())
        row = {"K": K, "nway_ms": round(nway_ms, 4), "singles_ms": round(single_ms, 4), "ratio": round(nway_ms / single_ms, 4),
               "nway_min_ms": round(nway_min, 4), "singles_min_ms": round(single_min, 4), "detections": n_det}
        if not a.no_launch_count:
            try:
                row["launches_per_pass"] = launches(e, img)
            except Exception as ex:                       # the count is a side figure: a profiler that cannot attach does not end the run
                row["launches_per_pass"] = None
                row["launch_count_error"] = str(ex)[:200]
        rows.append(row)
        e.close()
        print(json.dumps(row), flush=True)
    for s in singles:
        s.close()
    res = {"bench": "nway", "image": [H, W], "precision": "fp32", "iters": a.iters, "warmup": a.warmup,
           "protocol": "one call + torch.cuda.synchronize() per timed step; singles = K back-to-back detect calls on K engines",
           "device": torch.cuda.get_device_name(0), "results": rows}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
