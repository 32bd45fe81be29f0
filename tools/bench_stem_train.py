#!/usr/bin/env python3
"""Training the stem (MODEL.BACKBONE.FREEZE_AT: 0) on one MI355X -> profiles/stem_train_bench.json.

    python tools/bench_stem_train.py                  # every leg, each in a process of its own under its own time limit
    python tools/bench_stem_train.py --leg events     # one leg in this process

Legs
  events  the three new launches (ore_conv2d_wgrad_s2_fwd, ore_conv2d_dgrad_s2_fwd, ore_stem1_wgrad_fwd) at the shapes of the 640x640 25-shot
          step's query batch (1 and 16 images), beside torch's own backward of the same layer (torch.autograd.grad of F.conv2d, stride 2,
          padding 1) in the same run, the forms alternating.  Device events around a batch of back-to-back launches divided by the batch
          (median over repeats): these hold the launch-to-launch gaps of a stream.
  trace   the same launches under rocprofv3 --kernel-trace in a run of its own: kernel times without the gaps (the reduce / pack launch
          of an entry point counted with it), and from them the fraction of the fp32 MFMA peak (wgrad_s2, dgrad_s2: algorithmic FLOPs of
          the shapes over kernel time over 157.3 TFLOP/s) or of the HBM bandwidth (stem1_wgrad: the bytes of dZ and of the image, each
          read once, over kernel time over 8.0 TB/s).
  train   tools/bench_train.py's step at --freeze-at 0 against --freeze-at 3, alternating in one run, at 1 and 16 images (ms/step).
The parent process never opens the GPU; a leg that ends in a fault or at its time limit ends the run (nothing is started behind it).
Every child -- a leg, rocprofv3 with the program it traces, a bench_train run -- is started as the leader of a process group of its own and
the whole group is killed at its limit, so nothing it started stays on the GPU; a leg's limit leaves a minute above the sum of the limits
of the children it starts, so those always end first."""
import argparse
import json
import os
import re
import signal
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "faster-orefsdet_amd"))
SIZE = 640
MFMA_FP32_PEAK = 157.3e12       # FLOP/s, fp32 matrix (spec)
HBM_PEAK = 8.0e12               # bytes/s (spec)
MEAN, STD = (103.53, 116.28, 123.675), (57.375, 57.12, 58.395)
BATCHES = (1, 16)
TRACE_N = 30


def _run_group(cmd, limit, capture=True):
    """Run cmd as the leader of a new process group under a time limit; at the limit the whole group is killed (a child of the child --
    the program under rocprofv3 -- must not outlive it on the GPU).  Returns (status, stdout, stderr); status 124 = limit."""
    pipe = subprocess.PIPE if capture else None
    p = subprocess.Popen(cmd, stdout=pipe, stderr=pipe, text=True, start_new_session=True)
    try:
        out, err = p.communicate(timeout=limit)
        return p.returncode, out or "", err or ""
    except subprocess.TimeoutExpired:
        try:
            os.killpg(p.pid, signal.SIGKILL)
        except ProcessLookupError:
            pass
        out, err = p.communicate()
        return 124, out or "", err or ""


def _shapes(B):
    """stem_3: X [B,320,320,64], dZ [B,160,160,128]; stem_1: image [B,3,640,640] uint8, dZ [B,320,320,64]."""
    return dict(B=B, H3=SIZE // 2, C2=64, C3=128, C1=64)


def _forms(torch, orehip, B):
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(B)
    s = _shapes(B)
    H3, C2, C3, C1 = s["H3"], s["C2"], s["C3"], s["C1"]
    x = torch.randn(B, H3, H3, C2, generator=g).cuda()
    dz3 = torch.randn(B, H3 // 2, H3 // 2, C3, generator=g).cuda()
    w3 = (torch.randn(C3, C2, 3, 3, generator=g) / (9 * C2) ** 0.5).cuda()
    img = torch.randint(0, 256, (B, 3, SIZE, SIZE), generator=g, dtype=torch.uint8).cuda()
    dz1 = torch.randn(B, H3, H3, C1, generator=g).cuda()
    dw3, dx, dw1 = torch.empty_like(w3), torch.empty_like(x), torch.empty(C1, 3, 3, 3, device="cuda")
    # torch's backward of the same layers (NCHW tensors in channels_last memory, as torch prefers them on this device)
    xt = x.permute(0, 3, 1, 2).requires_grad_(True)
    w3t = w3.clone().requires_grad_(True)
    gt3 = dz3.permute(0, 3, 1, 2)
    xn = ((img.float() - torch.tensor(MEAN).view(1, 3, 1, 1).cuda()) / torch.tensor(STD).view(1, 3, 1, 1).cuda())
    w1t = (torch.randn(C1, 3, 3, 3, generator=g) / 27 ** 0.5).cuda().requires_grad_(True)
    gt1 = dz1.permute(0, 3, 1, 2)
    M3, M1 = B * (H3 // 2) ** 2, B * H3 * H3
    forms = {
        "wgrad_s2": (lambda: orehip.conv2d_wgrad_s2(x, dz3, out=dw3), {"flops": 2.0 * M3 * C3 * C2 * 9}),
        "dgrad_s2": (lambda: orehip.conv2d_dgrad_s2(dz3, w3, H3, H3, out=dx), {"flops": 2.0 * M3 * C3 * C2 * 9}),
        "stem1_wgrad": (lambda: orehip.stem1_wgrad(img, SIZE, SIZE, MEAN, STD, dz1, out=dw1),
                        {"flops": 2.0 * M1 * C1 * 27, "bytes": 4.0 * M1 * C1 + img.numel()}),
        "torch_stem3_wgrad": (lambda: torch.autograd.grad(F.conv2d(xt, w3t, stride=2, padding=1), w3t, gt3), {}),
        "torch_stem3_dgrad": (lambda: torch.autograd.grad(F.conv2d(xt, w3t, stride=2, padding=1), xt, gt3), {}),
        "torch_stem3_fwd_only": (lambda: F.conv2d(xt, w3t, stride=2, padding=1), {}),
        "torch_stem1_wgrad": (lambda: torch.autograd.grad(F.conv2d(xn, w1t, stride=2, padding=1), w1t, gt1), {}),
        "torch_stem1_fwd_only": (lambda: F.conv2d(xn, w1t, stride=2, padding=1), {}),
    }
    return forms


def leg_events(a):
    import torch
    import orehip
    torch.cuda.set_device(0)
    out = []
    for B in BATCHES:
        forms = _forms(torch, orehip, B)
        samples = {k: [] for k in forms}
        for _ in range(a.repeats):                           # the forms alternate inside every repeat
            for k, (fn, _) in forms.items():
                for _ in range(a.warmup):
                    fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.batch):
                    fn()
                e1.record()
                e1.synchronize()
                samples[k].append(e0.elapsed_time(e1) * 1e3 / a.batch)
        row = {"images": B}
        for k, v in samples.items():
            row[k + "_us"] = round(statistics.median(v), 2)
            row[k + "_spread_us"] = [round(min(v), 2), round(max(v), 2)]
        # torch.autograd.grad of a fresh F.conv2d runs the forward too: its backward alone = the difference to the forward-only form
        row["torch_stem3_wgrad_minus_fwd_us"] = round(row["torch_stem3_wgrad_us"] - row["torch_stem3_fwd_only_us"], 2)
        row["torch_stem3_dgrad_minus_fwd_us"] = round(row["torch_stem3_dgrad_us"] - row["torch_stem3_fwd_only_us"], 2)
        row["torch_stem1_wgrad_minus_fwd_us"] = round(row["torch_stem1_wgrad_us"] - row["torch_stem1_fwd_only_us"], 2)
        out.append(row)
        print(json.dumps(row), flush=True)
    return {"protocol": "device events around %d back-to-back calls / %d, median of %d repeats, forms alternating; launch gaps included"
            % (a.batch, a.batch, a.repeats), "device": torch.cuda.get_device_name(0), "rows": out}


NEW = ("wgrad_s2", "dgrad_s2", "stem1_wgrad")


def leg_trace_child(a):
    import torch
    import orehip
    torch.cuda.set_device(0)
    for B in BATCHES:
        forms = _forms(torch, orehip, B)
        for k in NEW:
            for _ in range(TRACE_N):
                forms[k][0]()
            torch.cuda.synchronize()
    return {}


def leg_trace(a):
    import csv
    import glob
    import shutil
    d = os.path.abspath(a.out) + ".trace"
    shutil.rmtree(d, ignore_errors=True)
    cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "stem", "--", sys.executable, os.path.abspath(__file__),
           "--leg", "trace_child"]
    rc, so, se = _run_group(cmd, a.limit)
    if rc != 0:
        raise SystemExit("rocprofv3 ended with %d: %s" % (rc, (so + se)[-1500:]))
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            for r in csv.DictReader(fh):
                m = re.search(r"\bk_\w+", r["Kernel_Name"])
                if m:
                    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), m.group(0)))
    shutil.rmtree(d, ignore_errors=True)
    if not rows:
        raise SystemExit("no kernel of the library in the trace")
    rows.sort()
    # start order: per batch size, TRACE_N x wgrad_s2 (k_wgrad_s2 [+ k_wgrad_reduce]), TRACE_N x dgrad_s2 (k_pack_s2 + k_dgrad_s2), TRACE_N x
    # stem1_wgrad (k_stem1_wgrad [+ k_wgrad_reduce]); a helper kernel belongs to the entry point whose main kernel is nearest in the order
    main = {"k_wgrad_s2": "wgrad_s2", "k_dgrad_s2": "dgrad_s2", "k_stem1_wgrad": "stem1_wgrad"}
    groups, cur, pend, pend_names = [], None, 0.0, set()
    for t0, t1, name in rows:
        us = (t1 - t0) / 1e3
        if name in main:
            if cur is None or cur[0] != main[name] or len(cur[1]) == TRACE_N:
                cur = (main[name], [], set())
                groups.append(cur)
            cur[1].append(us + pend)
            cur[2].update(pend_names | {name})
            pend, pend_names = 0.0, set()
        elif name == "k_pack_s2":
            pend += us                                       # runs in front of its k_dgrad_s2
            pend_names.add(name)
        elif name.startswith("k_wgrad_reduce") and cur is not None:
            cur[1][-1] += us
            cur[2].add(name)
    assert [g[0] for g in groups] == list(NEW) * len(BATCHES), [g[0] for g in groups]
    out = []
    for gi, (form, times, names) in enumerate(groups):
        B = BATCHES[gi // len(NEW)]
        s = _shapes(B)
        M3, M1 = B * (s["H3"] // 2) ** 2, B * s["H3"] ** 2
        us = statistics.median(times)
        row = {"images": B, "launch": form, "kernels": sorted(names), "kernel_us": round(us, 2), "launches": len(times)}
        if form == "stem1_wgrad":
            nbytes = 4.0 * M1 * s["C1"] + B * 3 * SIZE * SIZE
            row["bytes"] = nbytes
            row["fraction_of_hbm_peak"] = round(nbytes / (us * 1e-6) / HBM_PEAK, 4)
        else:
            flops = 2.0 * M3 * s["C3"] * s["C2"] * 9            # both gradients of stem_3: as many multiply-adds as its forward
            row["flops"] = flops
            row["fraction_of_fp32_mfma_peak"] = round(flops / (us * 1e-6) / MFMA_FP32_PEAK, 4)
        out.append(row)
        print(json.dumps(row), flush=True)
    return {"protocol": "rocprofv3 --kernel-trace in a run of its own; per entry point the median over %d calls of one call's summed kernel time; "
            "peaks: %.1f TFLOP/s fp32 MFMA, %.1f TB/s HBM (spec)" % (TRACE_N, MFMA_FP32_PEAK / 1e12, HBM_PEAK / 1e12), "rows": out}


def leg_train(a):
    out = {}
    for batch in BATCHES:
        for rep in range(a.train_repeats):
            for fa in (0, 3):                                # alternating: both see the same machine
                cmd = [sys.executable, os.path.join(ROOT, "tools", "bench_train.py"), "--freeze-at", str(fa), "--batch", str(batch), "--steps",
                       str(a.train_steps), "--warmup", "3"]
                rc, so, se = _run_group(cmd, a.limit)
                if rc != 0:
                    raise SystemExit("bench_train --freeze-at %d --batch %d ended with %d: %s" % (fa, batch, rc, se[-800:]))
                r = json.loads(so.strip().splitlines()[-1])
                out.setdefault("freeze_at_%d/batch%d" % (fa, batch), []).append(r["ms_per_step"])
                print(fa, batch, r["ms_per_step"], flush=True)
    return {"protocol": "tools/bench_train.py --freeze-at <n> --batch <n> --warmup 3 --steps %d, eager fp32 step, %d alternating runs each"
            % (a.train_steps, a.train_repeats), "ms_per_step": out, "ms_per_step_median": {k: statistics.median(v) for k, v in out.items()}}


LEGS = {"events": leg_events, "trace": leg_trace, "trace_child": leg_trace_child, "train": leg_train}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=sorted(LEGS), default=None)
    ap.add_argument("--legs", nargs="+", default=["trace", "train", "events"])
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=50, help="calls per event pair (events)")
    ap.add_argument("--train-steps", type=int, default=10)
    ap.add_argument("--train-repeats", type=int, default=2)
    ap.add_argument("--limit", type=int, default=240, help="seconds a leg (a bench_train run inside train) may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stem_train_bench.json"))
    ap.add_argument("--leg-out", default=None)
    a = ap.parse_args()
    if a.leg:
        res = LEGS[a.leg](a)
        if a.leg_out:
            with open(a.leg_out, "w") as f:
                json.dump(res, f)
        return
    res = {"bench": "stem_train", "date": time.strftime("%Y-%m-%d"), "image": [SIZE, SIZE], "precision": "fp32"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for leg in a.legs:
        tmp = a.out + "." + leg + ".tmp"
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--leg-out", tmp, "--out", a.out]
        cmd += [x for k in ("warmup", "repeats", "batch", "limit", "train_steps", "train_repeats") for x in ("--" + k.replace("_", "-"), str(getattr(a, k)))]
        limit = a.limit * (2 * len(BATCHES) * a.train_repeats if leg == "train" else 1) + 60     # above the sum of the leg's children's limits
        rc = _run_group(cmd, limit, capture=False)[0]
        if rc != 0:
            res[leg] = {"error": "leg ended with status %d" % rc}
            print("leg %s ended with status %d: nothing more is started" % (leg, rc), flush=True)
            break
        with open(tmp) as f:
            res[leg] = json.load(f)
        os.remove(tmp)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: ("ok" if "error" not in v else v["error"]) for k, v in res.items() if isinstance(v, dict)}))


if __name__ == "__main__":
    main()
