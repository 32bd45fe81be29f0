#!/usr/bin/env python3
"""The depthwise body (V-19-slim-dw-eSE) beside the dense one (V-19-slim-eSE) on one MI355X -> profiles/dw_bench.json.

    python tools/bench_dw.py                      # every leg, each in a process of its own under its own time limit
    python tools/bench_dw.py --leg units          # one leg in this process

Legs
  engine  bench.py's sequential protocol (one 640x640 image per call through the captured engine pass, 25-shot cached support, bs 1)
          for both bodies in ONE process, alternating: images/s, kernel launches per image, the library's FLOP count of the pass.
  units   every distinct depthwise unit shape of the slim body at 640x640 (stem_2, stem_3, the stage 2-5 layers): the fused launch
          (k_dwpw, forced), the unfused composition (k_dw3x3 + the 1x1 conv launch), what the library's planner runs there
          (orehip.dwpw as the model calls it: library_form / library_us) and the dense 3x3 conv + FrozenBN + ReLU launch of the
          same (M, C) -- the layer the dense body runs there, from this library: this change leaves the conv kernels as they were.
          Times are device events around a batch of back-to-back launches divided by the batch (median over repeats), so they hold
          the launch-to-launch gap of a stream, not a trace's kernel time.
  trace   the same three forms per shape under rocprofv3 --kernel-trace, in a run of its own: kernel times without the gaps.
  train   tools/bench_train.py's step for both bodies at 1 and 16 images (ms/step).
The parent process never opens the GPU; a leg that ends in a fault or at its time limit ends the run (nothing is started behind it)."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "faster-orefsdet_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
SIZE = 640
DENSE = dict(stem=(64, 64, 128), conv=(64, 80, 96, 112), out=(112, 256, 384, 512))
DW = dict(stem=(64, 64, 64), conv=(64, 80, 96, 112), out=(112, 256, 384, 512))
# (name, rows = H x W of the unit's INPUT at 640x640, C, stride)
UNITS = [("stem_2", 320, 64, 1), ("stem_3", 320, 64, 2), ("stage2", 160, 64, 1), ("stage3", 80, 80, 1), ("stage4", 40, 96, 1),
         ("stage5", 20, 112, 1)]
# the other shapes the planner's rule (stride 1, rows x C >= 2^22) sends to the unfused form: frozen units of a 16-image training step
# (name, images, H = W, C, stride)
UNITS_BATCHED = [("stem_2 x16 images", 16, 320, 64, 1), ("stage2 x16 images", 16, 160, 64, 1)]
ALL_UNITS = [(n, 1, hw, C, st) for n, hw, C, st in UNITS] + UNITS_BATCHED


def leg_engine(a):
    import torch
    import orehip
    from oracle import ref_model as R
    import vovnet_dw_ref as D
    torch.cuda.set_device(0)
    img = R.synth_image(0, SIZE, SIZE).cuda()
    engines = {}
    for name, spec, sd, dw in (("V-19-slim-dw-eSE", DW, D.synth_state_dict_dw(1), True), ("V-19-slim-eSE", DENSE, R.synth_state_dict(0), False)):
        e = orehip.Engine(stem=spec["stem"], conv=spec["conv"], out=spec["out"], max_batch=1, max_h=SIZE, max_w=SIZE, depthwise=dw)
        e.load_state_dict(sd)
        e.set_support(R.synth_support(0))
        e.finalize()
        engines[name] = e
    from torch.profiler import ProfilerActivity, profile
    out = {}
    for name, e in engines.items():
        e.eval_forward(img, use_graph=False)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            e.eval_forward(img, use_graph=False)
            torch.cuda.synchronize()
        n = sum(1 for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA and "emcpy" not in ev.name)
        out[name] = {"launches_per_image": n, "flops_per_image": e.last_flops(), "images_per_s": []}
    for _ in range(a.warmup):
        for e in engines.values():
            e.eval_forward(img, use_graph=True)
    torch.cuda.synchronize()
    for _ in range(a.repeats):                               # alternate the bodies: both see the same machine
        for name, e in engines.items():
            t0 = time.perf_counter()
            for _ in range(a.steps):
                e.eval_forward(img, use_graph=True)
                torch.cuda.synchronize()
            out[name]["images_per_s"].append(a.steps / (time.perf_counter() - t0))
    for v in out.values():
        v["images_per_s_median"] = statistics.median(v["images_per_s"])
    for e in engines.values():
        e.close()
    return {"protocol": "eval_forward(use_graph=True) + synchronize per image, %d images x %d repeats per body, alternating" % (a.steps, a.repeats),
            "device": torch.cuda.get_device_name(0), "bodies": out}


def leg_units(a):
    import torch
    import orehip
    torch.cuda.set_device(0)
    g = torch.Generator().manual_seed(0)
    rows = []
    for name, nb, hw, C, stride in ALL_UNITS:
        x = torch.randn(nb, hw, hw, C, generator=g).cuda()
        w_dw = (torch.randn(C, 1, 3, 3, generator=g) / 3).cuda()
        w_pw = torch.randn(C, C, 1, 1, generator=g) / C ** 0.5
        w_33 = torch.randn(C, C, 3, 3, generator=g) / (9 * C) ** 0.5
        sc, sh = (torch.rand(C, generator=g) + 0.5).cuda(), torch.randn(C, generator=g).cuda()
        pw, p33 = orehip.pack_conv_weight(w_pw.cuda()), orehip.pack_conv_weight(w_33.cuda())
        wino = orehip.winograd_weight(p33, C, C) if stride == 1 and orehip.winograd_covers(C, C) else None
        ho = (hw - 1) // stride + 1
        out = torch.empty(nb, ho, ho, C, device="cuda")
        t = torch.empty(nb, ho, ho, C, device="cuda")
        M = nb * ho * ho
        forms = {
            "dwpw_us": lambda: orehip.dwpw(x, w_dw, pw, C, stride, sc, sh, out=out, fused=True),
            "library_us": lambda: orehip.dwpw(x, w_dw, pw, C, stride, sc, sh, out=out),
            "dw3x3_plus_1x1_us": lambda: (orehip.dw3x3(x, w_dw, C, stride, out=t),
                                          orehip.conv2d(t, pw, C, 1, 1, 0, scale=sc, shift=sh, relu_cout=C, out=out)),
            "dw3x3_us": lambda: orehip.dw3x3(x, w_dw, C, stride, out=t),
            "dense3x3_us": lambda: orehip.conv2d(x, p33, C, 3, stride, 1, scale=sc, shift=sh, relu_cout=C, out=out, w_wino=wino),
        }
        row = {"unit": name, "M": M, "C": C, "stride": stride,
               "library_form": "k_dw3x3 + 1x1" if orehip.dwpw_prefers_composition(M, C, stride) else "k_dwpw", "dwpw_flops": 2.0 * M * C * (9 + C),
               "dense3x3_flops": 2.0 * M * C * C * 9}
        samples = {k: [] for k in forms}
        for _ in range(a.repeats):                           # the forms alternate inside every repeat
            for k, fn in forms.items():
                for _ in range(a.warmup):
                    fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.batch):
                    fn()
                e1.record()
                e1.synchronize()
                samples[k].append(e0.elapsed_time(e1) * 1e3 / a.batch)
        for k, v in samples.items():
            row[k] = round(statistics.median(v), 3)
            row[k.replace("_us", "_spread_us")] = [round(min(v), 3), round(max(v), 3)]
        row["fused_vs_unfused"] = round(row["dwpw_us"] / row["dw3x3_plus_1x1_us"], 3)
        row["fused_vs_dense3x3"] = round(row["dwpw_us"] / row["dense3x3_us"], 3)
        rows.append(row)
        print(json.dumps(row), flush=True)
    return {"protocol": "device events around %d back-to-back launches / %d, median of %d repeats, forms alternating" % (a.batch, a.batch, a.repeats),
            "device": torch.cuda.get_device_name(0), "units": rows}


TRACE_N = 60          # launches per form and shape in the traced run


def _unit_forms(orehip, torch, g, nb, hw, C, stride):
    x = torch.randn(nb, hw, hw, C, generator=g).cuda()
    w_dw = (torch.randn(C, 1, 3, 3, generator=g) / 3).cuda()
    pw = orehip.pack_conv_weight((torch.randn(C, C, 1, 1, generator=g) / C ** 0.5).cuda())
    p33 = orehip.pack_conv_weight((torch.randn(C, C, 3, 3, generator=g) / (9 * C) ** 0.5).cuda())
    sc, sh = (torch.rand(C, generator=g) + 0.5).cuda(), torch.randn(C, generator=g).cuda()
    wino = orehip.winograd_weight(p33, C, C) if stride == 1 and orehip.winograd_covers(C, C) else None
    ho = (hw - 1) // stride + 1
    out, t = torch.empty(nb, ho, ho, C, device="cuda"), torch.empty(nb, ho, ho, C, device="cuda")
    return [lambda: orehip.dwpw(x, w_dw, pw, C, stride, sc, sh, out=out, fused=True),
            lambda: orehip.conv2d(x, p33, C, 3, stride, 1, scale=sc, shift=sh, relu_cout=C, out=out, w_wino=wino),
            lambda: (orehip.dw3x3(x, w_dw, C, stride, out=t), orehip.conv2d(t, pw, C, 1, 1, 0, scale=sc, shift=sh, relu_cout=C, out=out))]


def leg_trace_child(a):
    """What the traced run executes: per unit shape TRACE_N x [k_dwpw], TRACE_N x [dense 3x3], TRACE_N x [k_dw3x3, 1x1 conv], in that
    order (leg_trace tells the forms apart by it), a synchronise behind every form."""
    import torch
    import orehip
    torch.cuda.set_device(0)
    g = torch.Generator().manual_seed(0)
    for name, nb, hw, C, stride in ALL_UNITS:
        for fn in _unit_forms(orehip, torch, g, nb, hw, C, stride):
            for _ in range(TRACE_N):
                fn()
            torch.cuda.synchronize()
    return {}


def leg_trace(a):
    """Kernel times without launch gaps: rocprofv3 --kernel-trace around leg_trace_child in a run of its own, the library's kernels
    (k_*) taken in start order and attributed by the child's order of forms.  Per form: the median over its launches of the summed
    kernel time of one launch."""
    import csv
    import glob
    import shutil
    d = os.path.abspath(a.out) + ".trace"
    shutil.rmtree(d, ignore_errors=True)
    cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "dw", "--", sys.executable, os.path.abspath(__file__),
           "--leg", "trace_child"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
    if p.returncode != 0:
        raise SystemExit("rocprofv3 ended with %d: %s" % (p.returncode, (p.stdout + p.stderr)[-1500:]))
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit("no kernel trace under %s: %s" % (d, os.listdir(d)))
    rows = []
    for f in files:
        with open(f) as fh:
            for r in csv.DictReader(fh):
                m = re.search(r"\bk_\w+", r["Kernel_Name"])          # the library's kernels; torch's own are not named k_*
                if m:
                    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), m.group(0)))
    rows.sort()
    shutil.rmtree(d, ignore_errors=True)
    # start order -> (shape, form): a k_dwpw after anything else opens the next shape; a conv kernel behind k_dwpw is the dense
    # layer's until the first k_dw3x3, behind which everything is the composition's
    per = []
    state = None
    for t0, t1, name in rows:
        if name.startswith("k_dwpw"):
            if state != "fused":
                per.append({"fused": [], "dense": [], "comp": []})
            state = "fused"
        elif name.startswith("k_dw3x3"):
            state = "comp"
        elif state == "fused":
            state = "dense"
        if state is None or name.startswith("k_pack") or name.startswith("k_wino_weight"):
            continue
        per[-1][state].append((t0, t1, name))
    assert len(per) == len(ALL_UNITS), (len(per), [len(v["fused"]) for v in per])
    out = []
    for (uname, nb, hw, C, stride), forms in zip(ALL_UNITS, per):
        row = {"unit": uname, "C": C, "stride": stride}
        for key, label in (("fused", "k_dwpw"), ("dense", "dense3x3"), ("comp", "dw3x3_plus_1x1")):
            ks = forms[key]
            assert len(ks) % TRACE_N == 0 and ks, (uname, key, len(ks))
            per_launch = len(ks) // TRACE_N
            sums = [sum(t1 - t0 for t0, t1, _ in ks[i * per_launch:(i + 1) * per_launch]) / 1e3 for i in range(TRACE_N)]
            row[label + "_kernel_us"] = round(statistics.median(sums), 3)
            row[label + "_kernels"] = sorted({n for _, _, n in ks})
        out.append(row)
        print(json.dumps(row), flush=True)
    return {"protocol": "rocprofv3 --kernel-trace in a run of its own; per form the median over %d launches of one launch's summed kernel time" % TRACE_N,
            "units": out}


def leg_train(a):
    """tools/bench_train.py for both bodies, alternating, each run a process of its own under its own time limit."""
    out = {}
    for batch in (1, 16):
        for cfg in ("finetune_vovnet_dw.yaml", "finetune_vovnet.yaml"):
            cmd = [sys.executable, os.path.join(ROOT, "tools", "bench_train.py"), "--config", cfg, "--batch", str(batch), "--steps", str(a.train_steps),
                   "--warmup", "3"]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
            if p.returncode != 0:
                raise SystemExit("bench_train %s batch %d ended with %d: %s" % (cfg, batch, p.returncode, p.stderr[-800:]))
            r = json.loads(p.stdout.strip().splitlines()[-1])
            out["%s/batch%d" % (cfg, batch)] = {"ms_per_step": r["ms_per_step"], "images_per_s": r["value"], "steps": r["steps"]}
            print(cfg, batch, out["%s/batch%d" % (cfg, batch)], flush=True)
    return {"protocol": "tools/bench_train.py --config <file> --batch <n> --warmup 3, eager fp32 step", "runs": out}


LEGS = {"engine": leg_engine, "units": leg_units, "train": leg_train, "trace": leg_trace, "trace_child": leg_trace_child}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=sorted(LEGS), default=None)
    ap.add_argument("--legs", nargs="+", default=["engine", "units", "trace", "train"])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=200, help="launches per event pair (units)")
    ap.add_argument("--train-steps", type=int, default=10)
    ap.add_argument("--limit", type=int, default=240, help="seconds a leg (a bench_train run inside train) may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dw_bench.json"))
    ap.add_argument("--leg-out", default=None)
    a = ap.parse_args()
    if a.leg:
        res = LEGS[a.leg](a)
        if a.leg_out:
            with open(a.leg_out, "w") as f:
                json.dump(res, f)
        return
    res = {"bench": "dw", "date": time.strftime("%Y-%m-%d"), "image": [SIZE, SIZE], "precision": "fp32"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for leg in a.legs:
        tmp = a.out + "." + leg + ".tmp"
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--leg-out", tmp] + [x for k in ("steps", "warmup", "repeats", "batch", "limit")
                                                                                             for x in ("--" + k, str(getattr(a, k)))]
        cmd += ["--train-steps", str(a.train_steps)]
        limit = a.limit * (5 if leg == "train" else 1)
        try:
            rc = subprocess.run(cmd, timeout=limit).returncode
        except subprocess.TimeoutExpired:
            rc = 124
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
