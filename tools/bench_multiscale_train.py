#!/usr/bin/env python3
"""Train-step benchmark on the reference's multi-scale schedule: per image a seeded draw from cfg.INPUT.MIN_SIZE_TRAIN (the short side;
the raw aspect ratio is fixed, so seven sizes occur), 25-shot, at --batch 1 and --batch 16.  Each batch size is run three ways in one
process, every one behind its own warm-up on the same schedule:
    eager     the plain step
    default   fewx.solver.GraphedTrainStep() as it comes: one graph, captured again whenever the shapes change
    cached    GraphedTrainStep(max_graphs=..., recur=1, mixed_sizes=True): a bounded cache of graphs, mixed sizes staged as one slab
and, at 16 images, the launch that builds the batch canvases (ore_batch_canvas_fwd) is timed beside the torch composition it replaces
and a device copy of the bytes it writes.  Synthetic data and weights; raw uint8 images and crops, as the dataset mapper hands them over.

    python tools/bench_multiscale_train.py --steps 40 --warmup 40
Writes profiles/multiscale_train_bench.json and prints it."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "faster-orefsdet_amd"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def build(cfg_file, shots):
    from fewx.config import get_cfg
    from detectron2.modeling import build_model
    from fewx.solver import build_optimizer
    from oracle import ref_model as R                      # synthetic weights / inputs only (not the thing measured)
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "faster-orefsdet_amd", "configs", "fsod", cfg_file))
    cfg.merge_from_list(["MODEL.DEVICE", "cuda", "INPUT.FS.SUPPORT_SHOT", shots])
    cfg.freeze()
    torch.manual_seed(0)
    m = build_model(cfg)
    sd = R.synth_roi_state(R.synth_state_dict(0), 0)
    sd["roi_heads.box_head.0.fc1.weight"] *= 0.02
    m.load_state_dict(sd, strict=False)
    m.train()
    opt = build_optimizer(cfg, m)
    opt.set_lr_factor(0.01)
    return cfg, m, opt


def templates(cfg, shots, aspect, support_hw):
    """One synthetic sample per size of the schedule: (image uint8 [3,h,w], gt boxes, support crops uint8 [shots,3,s,s], support boxes)."""
    from oracle import ref_train as T
    out = []
    for i, short in enumerate(cfg.INPUT.MIN_SIZE_TRAIN):
        hw = (int(short), min(int(short * aspect + 0.5), int(cfg.INPUT.MAX_SIZE_TRAIN)))
        img, gt, sup, sbox = T.synth_train_inputs(100 + i, hw, n_gt=8, shots=shots, support_hw=support_hw)
        out.append((hw, img.to(torch.uint8), gt, sup.clamp(0, 255).to(torch.uint8), sbox.numpy()))
    return out


def schedule(tpl, batch, steps, seed):
    """`steps` batches of `batch` items, the size of every image drawn with a seeded generator."""
    from detectron2.structures import Boxes, Instances
    g = torch.Generator().manual_seed(seed)
    draws = torch.randint(0, len(tpl), (steps, batch), generator=g).tolist()
    items = []
    for hw, img, gt, sup, sbox in tpl:
        inst = Instances(hw)
        inst.gt_boxes, inst.gt_classes = Boxes(gt), torch.zeros(len(gt), dtype=torch.int64)
        items.append({"image": img, "instances": inst, "support_images": sup, "support_bboxes": sbox})
    return [[items[k] for k in row] for row in draws]


def run_mode(mode, cfg_file, shots, warm, timed, max_graphs):
    from fewx.solver import GraphedTrainStep
    cfg, m, opt = build(cfg_file, shots)
    stepper = None
    if mode == "default":
        stepper = GraphedTrainStep(m, opt)
    elif mode == "cached":
        stepper = GraphedTrainStep(m, opt, max_graphs=max_graphs, recur=1, mixed_sizes=True)

    def step(items):
        if stepper is not None:
            return stepper(items)
        losses = m(items)
        opt.zero_grad()
        sum(losses.values()).backward()
        opt.step()
        return losses

    for items in warm:
        step(items)
    torch.cuda.synchronize()
    before = stepper.stats() if stepper is not None else None
    t0 = time.perf_counter()
    for items in timed:
        losses = step(items)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    res = {"ms_per_step": 1e3 * el / len(timed), "steps": len(timed), "warmup_steps": len(warm),
           "finite": all(bool(torch.isfinite(v)) for v in losses.values())}
    if stepper is not None:
        s = stepper.stats()
        res.update(error=stepper.error, captures_total=s["captures"], captures_in_timed_window=s["captures"] - before["captures"],
                   eager_steps_in_timed_window=s["eager_steps"] - before["eager_steps"], replays_in_timed_window=s["replays"] - before["replays"],
                   graphs_alive=s["graphs"], cache_full=s["full"], reserved_bytes_per_capture=s["reserved_bytes"],
                   reserved_bytes_total=torch.cuda.memory_reserved())
    del stepper, m, opt
    import gc
    gc.collect()
    torch.cuda.empty_cache()
    return res


def compose(imgs, sups, mean, std, div):
    """The mixed-size branch of train_forward.train_core on device tensors (the composition the canvas kernel replaces)."""
    from fewx.modeling.fsod.train_forward import _normalise_pad
    imgs = [i.float() for i in imgs]
    Hm, Wm = max(i.shape[-2] for i in imgs), max(i.shape[-1] for i in imgs)
    xq = torch.cat([F.pad(_normalise_pad(i[None], mean, std, 1), (0, Wm - i.shape[-1], 0, Hm - i.shape[-2])) for i in imgs], 0)
    xq = F.pad(xq, (0, (Wm + div - 1) // div * div - Wm, 0, (Hm + div - 1) // div * div - Hm)).contiguous()
    xs = _normalise_pad(torch.cat(sups, 0), mean, std, div)
    return xq, xs


def time_events(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps                       # ms, launch to launch


def canvas_bench(cfg_file, shots, items, reps):
    import orehip
    cfg, m, opt = build(cfg_file, shots)
    div = m.backbone.size_divisibility
    mean, std = m.pixel_mean.view(-1), m.pixel_std.view(-1)
    plan = orehip.batch_canvas_plan([i["image"] for i in items], [i["support_images"] for i in items], div=div, full_slab=True)
    buf = torch.empty(plan.host.numel(), dtype=torch.uint8, device="cuda")
    buf[:plan.used].copy_(plan.host[:plan.used])
    out = torch.empty(plan.geom.out_floats, device="cuda")
    imgs, sups = [i["image"].cuda() for i in items], [i["support_images"].cuda() for i in items]
    xq, xs = orehip.batch_canvas(buf, plan.geom, mean, std, out=out)
    rq, rs = compose(imgs, sups, mean, std, div)
    equal = bool(torch.equal(xq, rq) and torch.equal(xs, rs))
    src = torch.empty_like(out)
    res = {"images": len(items), "sizes": [list(i["image"].shape[1:]) for i in items], "query_canvas": list(plan.geom.q_canvas),
           "support_canvas": list(plan.geom.s_canvas), "jobs": plan.geom.n_query + plan.geom.n_support,
           "bytes_written": 4 * plan.geom.out_floats, "bytes_read": plan.used - plan.geom.table_bytes, "upload_bytes": plan.used,
           "equals_torch_composition": equal,
           "kernel_ms": time_events(lambda: orehip.batch_canvas(buf, plan.geom, mean, std, out=out), reps),
           "torch_composition_ms": time_events(lambda: compose(imgs, sups, mean, std, div), reps),
           "device_copy_same_bytes_ms": time_events(lambda: out.copy_(src), reps)}
    t0 = time.perf_counter()
    for _ in range(10):
        orehip.batch_canvas_plan([i["image"] for i in items], [i["support_images"] for i in items], div=div, full_slab=True)
    res["host_plan_ms"] = 1e2 * (time.perf_counter() - t0)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--max-graphs", type=int, default=8)
    ap.add_argument("--shots", type=int, default=24, help="INPUT.FS.SUPPORT_SHOT (24 = the 25-shot config)")
    ap.add_argument("--support-hw", type=int, default=240)
    ap.add_argument("--aspect", type=float, default=4.0 / 3.0, help="raw width / height of every image")
    ap.add_argument("--canvas-reps", type=int, default=50)
    ap.add_argument("--config", default="finetune_vovnet.yaml")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multiscale_train_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_multiscale_train.py measures on a GPU; none found")
    cfg = build(a.config, a.shots)[0]
    tpl = templates(cfg, a.shots, a.aspect, a.support_hw)
    res = {"tool": "tools/bench_multiscale_train.py", "date": time.strftime("%Y-%m-%d"), "device": torch.cuda.get_device_name(0),
           "config": a.config, "shots": a.shots, "support_hw": a.support_hw, "sizes": [list(t[0]) for t in tpl], "raw_dtype": "uint8",
           "max_graphs": a.max_graphs, "recur": 1, "batch": {}}
    for B in a.batches:
        warm, timed = schedule(tpl, B, a.warmup, 11), schedule(tpl, B, a.steps, 12)
        res["batch"][str(B)] = {mode: run_mode(mode, a.config, a.shots, warm, timed, a.max_graphs) for mode in ("eager", "default", "cached")}
        print(json.dumps({B: res["batch"][str(B)]}), flush=True)
    res["canvas_kernel"] = canvas_bench(a.config, a.shots, schedule(tpl, 16, 1, 13)[0], a.canvas_reps)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
