"""Time the detection overlay and the demo's predictors on the device.

  overlay      ore_overlay_draw_fwd alone (prepare + draw) at 480x640 and 1080x1920 with 20 and 100 rows, in place and out of place:
               the median over rounds of the mean of `launches` back-to-back calls between two device events, after a warm-up; the
               bytes a perfect kernel would move (out of place: the frame read and written; in place: the touched 1024-pixel runs read and
               written) against the measured HBM copy rate; and overlay_host on the same frames, for scale
  demo         VisualizationDemo.run_on_image per frame against DefaultPredictor alone, alternating round by round in one process
  async        AsyncPredictor frames/s at inflight 1, 2 and 4, with and without the overlay, against the one-image protocol
               (DefaultPredictor, one frame at a time), alternating round by round in the same process

The detector is the synthetic-weight model of the test suite (the time does not depend on the weights' values).  Every drawn frame
is checked against overlay_host once, byte for byte, before anything is timed.  Prints one JSON line.

    python tools/bench_overlay.py [--frames 64] [--rounds 5] [--launches 400] [--out profiles/overlay_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "faster-orefsdet_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_COPY_BYTES_PER_S = 6.29e12            # the measured HBM copy rate of the MI355X this project prices memory-bound kernels with
FRAME_SIZES = [(480, 640), (1080, 1920)]
ROWS = [20, 100]
RUN_PIXELS = 1024                         # pixels of one draw block (csrc/ore_overlay.hip: 256 threads x 4)


def load_synthetic(model):
    from oracle import ref_model as R
    sd = R.synth_state_dict(0)
    sd2 = R.synth_roi_state(sd)
    sd2["roi_heads.box_head.0.fc1.weight"] = sd2["roi_heads.box_head.0.fc1.weight"] * 0.01
    model.load_state_dict(sd, strict=False)
    model.load_state_dict({k: v for k, v in sd2.items() if k.startswith("roi_heads.")}, strict=False)
    rc8 = torch.randn(24, 128, 8, 8, generator=torch.Generator().manual_seed(9)) * 0.1
    model.set_support_dict({**{k: {0: v} for k, v in R.synth_support(0).items()}, "rcnn_8": {0: rc8}, "rcnn_4": {0: torch.zeros(24, 128, 4, 4)}})
    return model.eval()


def demo_cfg():
    from fewx.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "faster-orefsdet_amd", "configs", "fsod", "finetune_vovnet.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", "cuda", "MODEL.WEIGHTS", "", "INPUT.MAX_SIZE_TEST", 1000])
    return cfg


def random_rows(h, w, n, seed):
    """n detection-like rows: sides of 5 % .. 35 % of the frame, scores descending."""
    rng = np.random.default_rng(seed)
    bw, bh = rng.uniform(0.05, 0.35, n) * w, rng.uniform(0.05, 0.35, n) * h
    x0, y0 = rng.uniform(0, w - bw), rng.uniform(0, h - bh)
    boxes = np.stack([x0, y0, x0 + bw, y0 + bh], 1).astype(np.float32)
    return boxes, np.sort(rng.uniform(0.05, 1.0, n).astype(np.float32))[::-1].copy(), rng.integers(0, 5, n).astype(np.int64)


def touched_runs(orehip, boxes, scores, classes, h, w, kw):
    """How many of the frame's 1024-pixel runs hold a drawn pixel -- an outline band or a label -- (what an in-place draw has to read
    and write), of how many, and the fraction of the frame's pixels that are drawn."""
    L = kw["line_width"]
    tab = orehip.overlay_instance_table(boxes, scores, classes, None, h, w, 0.0, kw["text_scale"], orehip.OVERLAY_PALETTE, 0,
                                        orehip.overlay_names_table(kw["names"]))
    hit = np.zeros((h, w), bool)
    for q in tab:
        X0, Y0, X1, Y1 = q["rect"]
        box = np.ones((Y1 - Y0 + 1, X1 - X0 + 1), bool)
        box[L:-L, L:-L] = False
        hit[Y0:Y1 + 1, X0:X1 + 1] |= box
        lx, ly, lw, lh = q["label"]
        hit[ly:ly + lh, lx:lx + lw] = True
    flat = hit.reshape(-1)
    pad = (-len(flat)) % RUN_PIXELS
    runs = np.concatenate([flat, np.zeros(pad, bool)]).reshape(-1, RUN_PIXELS).any(1)
    return int(runs.sum()), int(len(runs)), float(hit.mean())


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


def overlay_cases(orehip, args):
    from detectron2.utils.visualizer import default_overlay_params
    names = ["stone", "pebble", "rock", "boulder", "gravel"]
    orehip.overlay_atlas()                                    # built once per process: not part of a frame's time
    out = []
    for h, w in FRAME_SIZES:
        img = np.random.default_rng(h).integers(0, 256, (h, w, 3), dtype=np.uint8)
        dev = torch.from_numpy(img).cuda()
        for n in ROWS:
            boxes, scores, classes = random_rows(h, w, n, h + n)
            kw = dict(default_overlay_params(h, w), names=names)
            want = orehip.overlay_host(img, boxes, scores, classes, **kw)
            t0 = time.perf_counter()
            for _ in range(3):
                orehip.overlay_host(img, boxes, scores, classes, **kw)
            host_ms = (time.perf_counter() - t0) * 1e3 / 3
            d = [torch.from_numpy(a).cuda() for a in (boxes, scores, classes)]
            n_dev = torch.tensor([n], dtype=torch.int32, device="cuda")
            equal = np.array_equal(orehip.overlay_draw(dev, *d, n_dev, **kw).cpu().numpy(), want)
            work = dev.clone()
            equal = equal and np.array_equal(orehip.overlay_draw(work, *d, n_dev, out=work, **kw).cpu().numpy(), want)
            runs, total, frac = touched_runs(orehip, boxes, scores, classes, h, w, kw)
            rec = {"frame_hw": [h, w], "rows": n, **default_overlay_params(h, w), "equals_overlay_host": bool(equal), "overlay_host_ms": host_ms,
                   "touched_runs": runs, "runs": total, "drawn_pixel_fraction": frac}
            if not equal:
                print(json.dumps(rec))
                sys.exit("the device overlay differs from overlay_host")
            dst = torch.empty_like(dev)
            # in place every call draws over the last one's picture: the bytes change, the work per call does not
            for name, fn, moved in (("out_of_place", lambda: orehip.overlay_draw(dev, *d, n_dev, out=dst, **kw), 2 * img.size),
                                    ("in_place", lambda: orehip.overlay_draw(work, *d, n_dev, out=work, **kw), 2 * runs * RUN_PIXELS * 3)):
                us, spread = event_us(fn, args.launches, args.rounds)
                rec[f"{name}_us"], rec[f"{name}_round_spread_us"] = us, spread
                rec[f"{name}_bytes_moved"] = moved
                rec[f"{name}_hbm_fraction"] = moved / (us * 1e-6) / HBM_COPY_BYTES_PER_S
            empty = torch.tensor([0], dtype=torch.int32, device="cuda")
            rec["in_place_no_rows_us"], _ = event_us(lambda: orehip.overlay_draw(work, *d, empty, out=work, **kw), args.launches, args.rounds)
            out.append(rec)
    return out


def loop_ms(fn, images):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for img in images:
        fn(img)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / len(images)


def async_fps(ap, images, draw):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pending = 0
    for img in images:
        if pending == ap.default_buffer_size:
            ap.get()
            pending -= 1
        ap.put(img, draw=draw)
        pending += 1
    while pending:
        ap.get()
        pending -= 1
    torch.cuda.synchronize()
    return len(images) / (time.perf_counter() - t0)


def predictor_cases(args):
    from detectron2.engine.defaults import DefaultPredictor
    from predictor import AsyncPredictor, VisualizationDemo
    cfg = demo_cfg()
    pred = DefaultPredictor(cfg)
    load_synthetic(pred.model)
    demo = VisualizationDemo(cfg)
    load_synthetic(demo.predictor.model)
    aps = {}
    for k in (1, 2, 4):
        aps[k] = AsyncPredictor(cfg, inflight=k)
        load_synthetic(aps[k].model)
    out = []
    for h, w in FRAME_SIZES:
        rng = np.random.default_rng(h + 1)
        raws = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(4)]
        images = [raws[i % len(raws)] for i in range(args.frames)]
        loops = {"default_predictor_ms_per_frame": pred, "run_on_image_ms_per_frame": demo.run_on_image,
                 "run_on_image_to_host_ms_per_frame": lambda im: demo.run_on_image(im)[1].get_image()}
        rates = {"one_image_protocol_fps": lambda: 1e3 / loop_ms(pred, images)}
        for k, ap in aps.items():
            rates[f"async_inflight{k}_fps"] = lambda ap=ap: async_fps(ap, images, None)
            rates[f"async_inflight{k}_drawn_fps"] = lambda ap=ap: async_fps(ap, images, True)
        for fn in loops.values():                             # warm-up: engines, graphs, tables, staging buffers at this size
            loop_ms(fn, images[:8])
        for fn in rates.values():
            fn()
        ms = {k: [] for k in loops}
        fps = {k: [] for k in rates}
        for _ in range(args.rounds):
            for k, fn in loops.items():
                ms[k].append(loop_ms(fn, images))
            for k, fn in rates.items():
                fps[k].append(fn())
        rec = {"frame_hw": [h, w], "detections": len(pred(raws[0])["instances"])}
        for k, v in {**ms, **fps}.items():
            rec[k] = float(np.median(v))
            rec[k + "_round_spread"] = [float(np.min(v)), float(np.max(v))]
        rec["overlay_cost_ms_per_frame"] = rec["run_on_image_ms_per_frame"] - rec["default_predictor_ms_per_frame"]
        out.append(rec)
    for ap in aps.values():
        ap.shutdown()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64, help="frames per round and loop")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=400, help="overlay calls between the two events (>= 200)")
    ap.add_argument("--out", default="", help="also write the record to this file")
    ap.add_argument("--kernel-only", action="store_true", help="only the overlay calls (for a kernel-trace run of a profiler)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_overlay needs the GPU"
    assert args.launches >= 200
    import PIL
    import orehip
    orehip.lib()
    out = {"workload": "detection_overlay", "device": torch.cuda.get_device_name(0), "pillow": PIL.__version__,
           "host_cpus_used": len(os.sched_getaffinity(0)), "date": time.strftime("%Y-%m-%d"), "frames_per_round": args.frames,
           "rounds": args.rounds, "launches": args.launches, "hbm_copy_bytes_per_s": HBM_COPY_BYTES_PER_S,
           "command": "python tools/bench_overlay.py" + "".join(f" --{k} {v}" for k, v in (("frames", args.frames), ("rounds", args.rounds),
                                                                                             ("launches", args.launches))),
           "overlay": overlay_cases(orehip, args), "predictors": [] if args.kernel_only else predictor_cases(args)}
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
