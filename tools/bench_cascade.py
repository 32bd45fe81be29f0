#!/usr/bin/env python3
"""What the cascade of CustomCascadeROIHeads costs: K = 1 against K = 3 stages (IOUS [0.6, 0.7, 0.8]), fp32, synthetic seeded weights and
supports as the tests make them.  Three modes, each a run of its own (merged into one JSON file by --out):

  eval      at 640 x 640: Engine.detect(img, 640, 640) + torch.cuda.synchronize() per call (the reference's FPS protocol: one image per
            forward), K = 1 and K = 3 in the same run: median ms, images/s, kernel launches of one eager pass;
  kernels   kernel time of ore_roi_cascade_refine_fwd and ore_roi_predict_cascade_fwd at cap 320, fc width 128, K-split 32 (the engine's
            form) and finished rows, from torch.profiler's kernel events; ore_roi_predict_parts_fwd next to them;
  train     one training step (forward, backward, optimizer) at 1 and 16 images of 320 x 320, eager and replayed by
            GraphedTrainStep, K = 1 and K = 3.

    python3 tools/bench_cascade.py --mode eval|kernels|train [--iters 50] [--warmup 10] [--out profiles/cascade_bench.json]
"""
import argparse
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "faster-orefsdet_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import orehip  # noqa: E402
import cascade_ref as CR  # noqa: E402
from oracle import ref_model as R  # noqa: E402

H = W = 640


def state(scale):
    sd = CR.synth_cascade_state(R.synth_roi_state(R.synth_state_dict(0), 0), 0, 3)
    for k in range(3):
        sd[f"roi_heads.box_head.{k}.fc1.weight"] = sd[f"roi_heads.box_head.{k}.fc1.weight"] * scale
    return sd


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


def kernel_events(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [(ev.name, ev.device_time if hasattr(ev, "device_time") else ev.cuda_time) for ev in prof.events()
            if ev.device_type == torch.autograd.DeviceType.CUDA and "emcpy" not in ev.name and "emset" not in ev.name]


def mode_eval(a):
    sd = state(0.01)
    sup = (R.synth_support(10), torch.randn(6, 128, 8, 8, generator=torch.Generator().manual_seed(40)) * 0.1)
    img = R.synth_image(3, H, W).cuda()
    rows = []
    for K in (1, 3):
        e = orehip.Engine(max_batch=1, max_h=H, max_w=W)
        e.load_state_dict(sd)
        e.set_support(sup[0])
        e.finalize()
        e.set_roi_cascade(sd, sup[1], CR.REG_W[:K], 0.05, 0.9, 100)
        ms, mn = timed(lambda: e.detect(img, H, W), a.iters, a.warmup)
        row = {"stages": K, "detect_ms": round(ms, 4), "detect_min_ms": round(mn, 4), "images_per_s": round(1e3 / ms, 2),
               "detections": int(e.detect(img, H, W)[1].numel())}
        try:
            row["launches_per_pass"] = len(kernel_events(lambda: e.eval_forward(img, use_graph=False)))
        except Exception as ex:                           # a side figure: a profiler that cannot attach does not end the run
            row["launches_per_pass"], row["launch_count_error"] = None, str(ex)[:200]
        rows.append(row)
        e.close()
        print(json.dumps(row), flush=True)
    return {"image": [H, W], "protocol": "Engine.detect + torch.cuda.synchronize() per image, replayed graph", "results": rows}


def mode_kernels(a):
    cap, Cc, S = 320, 128, 32
    rng = np.random.default_rng(0)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()     # noqa: E731
    head = [dev(x) for x in CR.RT._head(rng, Cc)]
    boxes = dev(CR.RT.clustered(cap, rng))
    out = []
    for parts in (S, 0):
        h = dev((rng.standard_normal((parts, cap, Cc)) / np.sqrt(parts)).astype(np.float32)) if parts else \
            dev(np.abs(rng.standard_normal((cap, Cc))).astype(np.float32))
        bias = dev(np.zeros(Cc, np.float32)) if parts else None
        st = {}

        def refine():
            st["r"] = orehip.roi_cascade_refine(h, *head, boxes, CR.REG_W[0], (640.0, 640.0), parts=parts, bias=bias)

        refine()
        nb, ssum, dead = st["r"]

        def tail():
            orehip.roi_predict(h, *head, nb, CR.REG_W[1], (640.0, 640.0), 0.05, 0.9, 100, parts=parts, bias=bias, score_sum=ssum, dead=dead, n_stages=2)

        def single():
            orehip.roi_predict(h, *head, boxes, CR.REG_W[0], (640.0, 640.0), 0.05, 0.9, 100, parts=parts, bias=bias)

        row = {"cap": cap, "C": Cc, "parts": parts}
        for name, fn in (("refine", refine), ("cascade_tail", tail), ("single_stage_tail", single)):
            per = {}
            for _ in range(a.iters):
                for kn, us in kernel_events(fn):
                    m = re.search(r"\b(k_\w+)", kn)
                    if m:
                        per.setdefault(m[1], []).append(us)
            row[name + "_us"] = {k: round(statistics.median(v), 2) for k, v in per.items()}
        out.append(row)
        print(json.dumps(row), flush=True)
    return {"protocol": "median of torch.profiler kernel events per launch", "results": out}


def mode_train(a):
    from detectron2.modeling import build_model
    from detectron2.structures import Boxes, Instances
    from fewx.config import get_cfg
    from fewx.solver import GraphedTrainStep, build_optimizer
    from oracle import ref_train as T
    shots = 4
    rows = []
    for K in (1, 3):
        for B in (1, 16):
            for mode in ("eager", "replayed"):
                cfg = get_cfg()
                cfg.merge_from_file(os.path.join(ROOT, "faster-orefsdet_amd", "configs", "fsod",
                                                 "finetune_vovnet_cascade.yaml" if K == 3 else "finetune_vovnet.yaml"))
                cfg.merge_from_list(["MODEL.DEVICE", "cuda", "INPUT.FS.SUPPORT_SHOT", shots])
                cfg.freeze()
                torch.manual_seed(0)
                m = build_model(cfg)
                sd = state(0.02)
                sd["proposal_generator.centernet_head.agn_hm.bias"] = torch.full((1,), -2.0)
                m.load_state_dict({k: v for k, v in sd.items() if K == 3 or (".1." not in k and ".2." not in k) or not k.startswith("roi_heads.box_")},
                                  strict=False)
                m.train()
                items = []
                for b in range(B):
                    img, gt, sup, sbox = T.synth_train_inputs(2 + b, (320, 320), n_gt=5, shots=shots, support_hw=96)
                    inst = Instances((320, 320))
                    inst.gt_boxes, inst.gt_classes = Boxes(gt), torch.zeros(len(gt), dtype=torch.int64)
                    items.append({"image": img, "instances": inst, "support_images": sup, "support_bboxes": sbox.numpy()})
                opt = build_optimizer(cfg, m)
                opt.set_lr_factor(0.02)
                stepper = GraphedTrainStep(m, opt, warmup=2) if mode == "replayed" else None

                def step():
                    if stepper is not None:
                        stepper(items)
                    else:
                        losses = m(items)
                        opt.zero_grad()
                        sum(losses.values()).backward()
                        opt.step()
                ms, mn = timed(step, max(a.iters // 5, 5), 4)
                row = {"stages": K, "images": B, "mode": mode, "step_ms": round(ms, 3), "step_min_ms": round(mn, 3),
                       "images_per_s": round(B * 1e3 / ms, 2)}
                if stepper is not None:
                    row["replays"], row["error"] = stepper.replays, stepper.error
                rows.append(row)
                print(json.dumps(row), flush=True)
                del m, opt, stepper
                torch.cuda.empty_cache()
    return {"image": [320, 320], "shots": shots, "protocol": "one step + torch.cuda.synchronize() per timed step", "results": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("eval", "kernels", "train"), required=True)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    res = {"eval": mode_eval, "kernels": mode_kernels, "train": mode_train}[a.mode](a)
    res.update(iters=a.iters, warmup=a.warmup, device=torch.cuda.get_device_name(0), precision="fp32")
    print(json.dumps({a.mode: res}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        doc = {"bench": "cascade"}
        if os.path.exists(a.out):
            with open(a.out) as f:
                doc = json.load(f)
        doc[a.mode] = res
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
