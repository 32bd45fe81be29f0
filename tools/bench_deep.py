#!/usr/bin/env python3
"""The deep bodies (V-39-eSE, V-57-eSE) beside V-19-eSE on one MI355X -> profiles/deep_bench.json.

    python tools/bench_deep.py                      # every leg, each in a process of its own under its own time limit
    python tools/bench_deep.py --leg tail           # one leg in this process

Legs
  engine  bench.py's sequential protocol (one 640x640 image per call through the captured engine pass, cached support, bs 1) for the
          three bodies in ONE process, alternating: images/s, kernel launches per image, the library's FLOP count of the pass.
  tail    the tail of an identity block at the stage-4 and stage-5 shapes of a 640x640 image (40 x 40 x 768, 20 x 20 x 1024), two forms:
          ore_ese_gate_residual_fwd (gate, product, identity add and the copy into the next concat buffer in ONE launch), and what
          the module path runs there: the gate launch (ese_gate_from_colsum), scale_channels, `+ ident`, and the slice copy into a
          fresh concat buffer.  Device events around a batch of back-to-back launches divided by the batch (median over repeats, the
          forms alternating), so the times hold the launch-to-launch gap of a stream.  Beside them: a device-to-device copy of the
          same bytes (two maps read, one written = a copy of 1.5 maps), the measure of tools/stream_bw.py, in the same process.
  trace   the same two forms per shape under rocprofv3 --kernel-trace, in a run of its own: kernel times without the gaps.
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
SIZE = 640
BODIES = ("V-19-eSE", "V-39-eSE", "V-57-eSE")
# (name, H = W of the stage at 640x640, C = stage_out_ch, concat width of an identity block = C + 5 * stage_conv_ch)
SHAPES = [("stage4", 40, 768, 768 + 5 * 192), ("stage5", 20, 1024, 1024 + 5 * 224)]
TRACE_N = 60          # launches per form and shape in the traced run


def leg_engine(a):
    import torch
    import orehip
    from oracle import ref_model as R
    torch.cuda.set_device(0)
    img = R.synth_image(0, SIZE, SIZE).cuda()
    engines = {}
    for body in BODIES:
        spec = R.VOVNET_SPECS[body]
        e = orehip.Engine(stem=spec["stem"], conv=spec["conv"], out=spec["out"], layers=spec["layers"], blocks=spec["blocks"], max_batch=1,
                          max_h=SIZE, max_w=SIZE)
        e.load_state_dict(R.synth_state_dict(0, body))
        e.set_support(R.synth_support(0))
        e.finalize()
        engines[body] = e
    from torch.profiler import ProfilerActivity, profile
    out = {}
    for name, e in engines.items():
        e.eval_forward(img, use_graph=False)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            e.eval_forward(img, use_graph=False)
            torch.cuda.synchronize()
        names = [ev.name for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA and "emcpy" not in ev.name]
        out[name] = {"launches_per_image": len(names), "identity_tail_launches": sum("k_ese_gate_residual" in n for n in names),
                     "identity_blocks": sum(b - 1 for b in R.VOVNET_SPECS[name]["blocks"]), "flops_per_image": e.last_flops(), "images_per_s": []}
    for _ in range(a.warmup):
        for e in engines.values():
            e.eval_forward(img, use_graph=True)
    torch.cuda.synchronize()
    for _ in range(a.repeats):                               # alternate the bodies: all see the same machine
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


def _tail_forms(orehip, torch, g, hw, C, cat_w):
    """The operands of one identity block's tail and its two forms: ([fused], [gate, scale_channels, + ident, slice copy])."""
    HW = hw * hw
    y = torch.relu(torch.randn(1, hw, hw, C, generator=g)).cuda()
    cat = torch.relu(torch.randn(1, hw, hw, cat_w, generator=g)).cuda()         # the block's own concat buffer: identity = first C channels
    nxt = torch.empty(1, hw, hw, cat_w, device="cuda")                          # the next block's
    P = (HW + 127) // 128
    part = torch.stack([c.sum(0) for c in y.view(HW, C).chunk(P)]).contiguous()
    fw, fb = (torch.randn(C, C, generator=g) / C ** 0.5).cuda(), (torch.randn(C, generator=g) * 0.5).cuda()

    def fused():
        orehip.ese_gate_residual(part, fw, fb, y, cat, nxt)

    def composed():
        gate = orehip.ese_gate_from_colsum(part, HW, fw, fb)
        out = orehip.scale_channels(y, gate) + cat[..., :C]
        fresh = torch.empty(1, hw, hw, cat_w, device="cuda")
        fresh[..., :C] = out
        return fresh

    def composed_tail_only(gate=orehip.ese_gate_from_colsum(part, HW, fw, fb)):
        out = orehip.scale_channels(y, gate) + cat[..., :C]
        fresh = torch.empty(1, hw, hw, cat_w, device="cuda")
        fresh[..., :C] = out
        return fresh

    return {"ese_gate_residual": fused, "module_path_4_launches": composed, "module_path_3_launches_gate_given": composed_tail_only}


def leg_tail(a):
    import torch
    import orehip
    torch.cuda.set_device(0)
    g = torch.Generator().manual_seed(0)
    rows = []
    for name, hw, C, cat_w in SHAPES:
        forms = _tail_forms(orehip, torch, g, hw, C, cat_w)
        nbytes = 3 * hw * hw * C * 4                         # two maps read, one written
        src = torch.empty(nbytes // 8, device="cuda").normal_()
        dst = torch.empty_like(src)
        forms["d2d_copy_same_bytes"] = lambda: dst.copy_(src)
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
        row = {"shape": name, "HW": hw * hw, "C": C, "bytes": nbytes}
        for k, v in samples.items():
            row[k + "_us"] = round(statistics.median(v), 3)
            row[k + "_spread_us"] = [round(min(v), 3), round(max(v), 3)]
        row["fused_vs_module_path"] = round(row["ese_gate_residual_us"] / row["module_path_4_launches_us"], 3)
        row["ese_gate_residual_GBps"] = round(nbytes / row["ese_gate_residual_us"] / 1e3, 1)
        row["d2d_copy_GBps"] = round(nbytes / row["d2d_copy_same_bytes_us"] / 1e3, 1)
        rows.append(row)
        print(json.dumps(row), flush=True)
    return {"protocol": "device events around %d back-to-back launches / %d, median of %d repeats, forms alternating" % (a.batch, a.batch, a.repeats),
            "device": torch.cuda.get_device_name(0), "shapes": rows}


def leg_trace_child(a):
    """What the traced run executes: per shape TRACE_N x [fused], then TRACE_N x [gate, scale_channels, add, copy], a synchronise
    behind every form (leg_trace tells the forms apart by the kernel names)."""
    import torch
    import orehip
    torch.cuda.set_device(0)
    g = torch.Generator().manual_seed(0)
    for name, hw, C, cat_w in SHAPES:
        forms = _tail_forms(orehip, torch, g, hw, C, cat_w)
        torch.cuda.synchronize()
        for k in ("ese_gate_residual", "module_path_4_launches"):
            for _ in range(TRACE_N):
                forms[k]()
            torch.cuda.synchronize()
    return {}


def _short(kernel_name):
    """k_name of a library kernel, the function name of anyone else's"""
    m = re.search(r"\bk_\w+", kernel_name) or re.search(r"[\w:]+", re.sub(r"^void\s+", "", kernel_name))
    return m.group(0)[:60] if m else kernel_name[:60]


def leg_trace(a):
    """Kernel times without launch gaps: rocprofv3 --kernel-trace around leg_trace_child in a run of its own.  The fused form is the
    launches of k_ese_gate_residual; the module path's form is every kernel between one k_ese_gate_fused and the next (the gate, the
    product, the add, the slice copy).  Per form and shape: the median over its TRACE_N launches of one launch's summed kernel time."""
    import csv
    import glob
    import shutil
    d = os.path.abspath(a.out) + ".trace"
    shutil.rmtree(d, ignore_errors=True)
    cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "deep", "--", sys.executable, os.path.abspath(__file__),
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
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    shutil.rmtree(d, ignore_errors=True)
    first = next(i for i, r in enumerate(rows) if "k_ese_gate_residual" in r[2])
    rows = rows[first:]                                       # everything before is the set-up of the first shape
    out, i = [], 0
    for name, hw, C, cat_w in SHAPES:
        while "k_ese_gate_residual" not in rows[i][2]:        # the set-up of this shape (its one k_ese_gate_fused included)
            i += 1
        fused = [(t1 - t0) / 1e3 for t0, t1, n in rows[i:i + TRACE_N]]
        assert all("k_ese_gate_residual" in n for _, _, n in rows[i:i + TRACE_N]), name
        i += TRACE_N
        groups = []
        while i < len(rows) and "k_ese_gate_residual" not in rows[i][2] and len(groups) <= TRACE_N:
            if "k_ese_gate_fused" in rows[i][2]:
                groups.append([])
            if groups:
                groups[-1].append(rows[i])
            i += 1
            if len(groups) == TRACE_N and len(groups[-1]) == len(groups[0]):
                break
        assert len(groups) == TRACE_N and len({len(gp) for gp in groups}) == 1, (name, len(groups), sorted({len(gp) for gp in groups}))
        comp = [sum(t1 - t0 for t0, t1, _ in gp) / 1e3 for gp in groups]
        row = {"shape": name, "HW": hw * hw, "C": C, "ese_gate_residual_kernel_us": round(statistics.median(fused), 3),
               "module_path_kernel_us": round(statistics.median(comp), 3), "module_path_kernels": [_short(n) for _, _, n in groups[0]]}
        out.append(row)
        print(json.dumps(row), flush=True)
    return {"protocol": "rocprofv3 --kernel-trace in a run of its own; per form the median over %d launches of one launch's summed kernel time" % TRACE_N,
            "shapes": out}


LEGS = {"engine": leg_engine, "tail": leg_tail, "trace": leg_trace, "trace_child": leg_trace_child}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=sorted(LEGS), default=None)
    ap.add_argument("--legs", nargs="+", default=["engine", "tail", "trace"])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=200, help="launches per event pair (tail)")
    ap.add_argument("--limit", type=int, default=240, help="seconds a leg may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deep_bench.json"))
    ap.add_argument("--leg-out", default=None)
    a = ap.parse_args()
    if a.leg:
        res = LEGS[a.leg](a)
        if a.leg_out:
            with open(a.leg_out, "w") as f:
                json.dump(res, f)
        return
    res = {"bench": "deep", "date": time.strftime("%Y-%m-%d"), "image": [SIZE, SIZE], "precision": "fp32"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for leg in a.legs:
        tmp = a.out + "." + leg + ".tmp"
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--leg-out", tmp, "--out", a.out]
        cmd += [x for k in ("steps", "warmup", "repeats", "batch", "limit") for x in ("--" + k, str(getattr(a, k)))]
        try:
            rc = subprocess.run(cmd, timeout=a.limit + 30).returncode
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
