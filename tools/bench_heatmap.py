"""Time the heat maps of a detection pass on the device.

  kernels      orehip.heatmap_draw from a pass's buffers ("objectness": 2 launches, "attention": 3) at 480x640 and 1080x1920 frames, and
               the render launch alone from maps already quantised: the median over rounds of the mean of `launches` back-to-back calls
               between two device events, after a warm-up.  The render's bytes (the frame read and written once) over its time, next
               to the rate of a device-to-device copy of the same frame and of a 1 GiB buffer measured in the same process.
  demo         VisualizationDemo(heatmap=kind).run_on_image per frame against the host composition in the same process: the same pass,
               the kind's buffers copied to the host, heatmap_levels_host + heatmap_host + overlay_host
  async        AsyncPredictor frames/s with heat map + boxes against boxes only, alternating round by round in the same process

The detector is the synthetic-weight model of the test suite (the time does not depend on the weights' values).  Every drawn frame is
checked against heatmap_host once, byte for byte, before anything is timed.  Prints one JSON line.

    python tools/bench_heatmap.py [--frames 64] [--rounds 5] [--launches 400] [--out profiles/heatmap_bench.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_heatmap.py --kernel-only      (kernel times, a run of its own)
    python tools/bench_heatmap.py --summarise-trace DIR > profiles/heatmap_kernel_stats.txt     (that run, per kernel and grid)
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "faster-orefsdet_amd"), ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_overlay import FRAME_SIZES, demo_cfg, event_us, load_synthetic, loop_ms  # noqa: E402

KINDS = ["objectness", "attention"]


def copy_rate(n_bytes, launches, rounds):
    """Bytes read + written per second of a device-to-device copy of n_bytes."""
    a = torch.empty(n_bytes, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    us, _ = event_us(lambda: b.copy_(a), launches, rounds)
    return 2 * n_bytes / (us * 1e-6)


def host_levels(orehip, engine, kind, slot=0):
    """The kind's buffers copied out of the engine, quantised on the host: [(uint8 map, stride)], in_hw."""
    what, geo = orehip.heat_kind(kind), engine.last_geometry()
    vals, strides = [], []
    for name in what["buffers"]:
        h, w, s = geo["levels"][int(name[-1]) - 3]
        vals.append(engine.buffer(name).float().cpu().numpy().reshape(geo["B"], h, w, -1)[slot])
        strides.append(s)
    maps = orehip.heatmap_levels_host(vals, channel=what["channel"], transform=what["transform"], norm=what["norm"])
    return list(zip(maps, strides)), (geo["H"], geo["W"])


def kernel_cases(orehip, pred, args):
    out = []
    stream_rate = copy_rate(1 << 30, 20, args.rounds)
    for h, w in FRAME_SIZES:
        img = np.random.default_rng(h).integers(0, 256, (h, w, 3), dtype=np.uint8)
        dev = torch.from_numpy(img).cuda()
        dst = torch.empty_like(dev)
        pred(img)                                             # the pass whose buffers are drawn
        e = pred.model._engine
        frame_rate = copy_rate(img.size, args.launches, args.rounds)
        for kind in KINDS:
            src = e.heat_source(kind)
            levels, in_hw = host_levels(orehip, e, kind)
            want = orehip.heatmap_host(img, levels, in_hw, channel_order="BGR")
            got = orehip.heatmap_draw(dev, src, channel_order="BGR")
            equal = bool(np.array_equal(got.cpu().numpy(), want))
            rec = {"frame_hw": [h, w], "kind": kind, "input_hw": list(in_hw), "level_hw": [list(m.shape) for m, _ in levels],
                   "launches_per_frame": 2 if src.norm == "unit" else 3, "equals_heatmap_host": equal,
                   "map_nonzero_fraction": float(np.mean([float((m > 0).mean()) for m, _ in levels]))}
            if not equal:
                print(json.dumps(rec))
                sys.exit("the device heat map differs from heatmap_host")
            rec["draw_us"], rec["draw_round_spread_us"] = event_us(lambda: orehip.heatmap_draw(dev, src, out=dst, channel_order="BGR"),
                                                                   args.launches, args.rounds)
            rec["levels_us"], _ = event_us(lambda: orehip.heatmap_levels(src), args.launches, args.rounds)
            maps = orehip.heatmap_levels(src)
            for name, fn in (("render_us", lambda: orehip.heatmap_draw(dev, maps, out=dst, channel_order="BGR")),
                             ("render_in_place_us", lambda: orehip.heatmap_draw(dst, maps, out=dst, channel_order="BGR"))):
                rec[name], rec[name.replace("_us", "_round_spread_us")] = event_us(fn, args.launches, args.rounds)
            rec["render_bytes_moved"] = 2 * img.size
            rec["render_bytes_per_s"] = 2 * img.size / (rec["render_us"] * 1e-6)
            rec["frame_copy_bytes_per_s"], rec["stream_copy_1gib_bytes_per_s"] = frame_rate, stream_rate
            out.append(rec)
    return out


def async_fps(ap, images, heatmap):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pending = 0
    for img in images:
        if pending == ap.default_buffer_size:
            ap.get()
            pending -= 1
        ap.put(img, draw=True, heatmap=heatmap)
        pending += 1
    while pending:
        ap.get()
        pending -= 1
    torch.cuda.synchronize()
    return len(images) / (time.perf_counter() - t0)


def predictor_cases(orehip, pred, args):
    from detectron2.utils.visualizer import default_overlay_params
    from predictor import AsyncPredictor, VisualizationDemo
    cfg = demo_cfg()
    demos = {}
    for kind in KINDS:
        demos[kind] = VisualizationDemo(cfg, heatmap=kind)
        load_synthetic(demos[kind].predictor.model)
    ap = AsyncPredictor(cfg, inflight=4)
    load_synthetic(ap.model)

    def host_composition(kind):
        def run(im):
            res = pred(im)["instances"]
            levels, in_hw = host_levels(orehip, pred.model._engine, kind)
            heat = orehip.heatmap_host(im, levels, in_hw, channel_order="BGR")
            return orehip.overlay_host(heat, res.pred_boxes.tensor.cpu(), res.scores.cpu(), res.pred_classes.cpu(),
                                       palette=np.ascontiguousarray(orehip.OVERLAY_PALETTE[:, ::-1]), **default_overlay_params(*im.shape[:2]))
        return run

    out = []
    for h, w in FRAME_SIZES:
        rng = np.random.default_rng(h + 1)
        raws = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(4)]
        images = [raws[i % len(raws)] for i in range(args.frames)]
        few = images[:max(args.frames // 8, 4)]                # the host composition is slow: fewer frames per round
        loops = {"default_predictor_ms_per_frame": (pred, images)}
        for kind in KINDS:
            loops[f"run_on_image_{kind}_ms_per_frame"] = (lambda im, d=demos[kind]: d.run_on_image(im)[1].img.cpu(), images)
            loops[f"host_composition_{kind}_ms_per_frame"] = (host_composition(kind), few)
        rates = {"async_boxes_fps": lambda: async_fps(ap, images, None)}
        for kind in KINDS:
            rates[f"async_{kind}_and_boxes_fps"] = lambda kind=kind: async_fps(ap, images, kind)
        for fn, ims in loops.values():                         # warm-up: engines, graphs, tables, workspaces at this size
            loop_ms(fn, ims[:4])
        for fn in rates.values():
            fn()
        ms, fps = {k: [] for k in loops}, {k: [] for k in rates}
        for _ in range(args.rounds):
            for k, (fn, ims) in loops.items():
                ms[k].append(loop_ms(fn, ims))
            for k, fn in rates.items():
                fps[k].append(fn())
        rec = {"frame_hw": [h, w], "detections": len(pred(raws[0])["instances"])}
        for k, v in {**ms, **fps}.items():
            rec[k] = float(np.median(v))
            rec[k + "_round_spread"] = [float(np.min(v)), float(np.max(v))]
        for kind in KINDS:
            rec[f"async_{kind}_cost_us_per_frame"] = 1e6 / rec[f"async_{kind}_and_boxes_fps"] - 1e6 / rec["async_boxes_fps"]
        out.append(rec)
    ap.shutdown()
    return out


def summarise_trace(d):
    """Per kernel name and grid of a rocprofv3 --kernel-trace run of `--kernel-only`: launches and the median / min / max duration.
    The grid tells the cases apart: the render's is the frame's, the other two's the model input's."""
    import collections
    import csv
    import glob
    files = glob.glob(os.path.join(d, "**", "*_kernel_trace.csv"), recursive=True)
    assert files, f"no *_kernel_trace.csv under {d}"
    per = collections.defaultdict(list)
    for r in csv.DictReader(open(files[0])):
        name = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        if "heatmap" in name:
            per[(name, int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"]))].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    print(f"{'kernel':44s} {'blocks':>7s} {'launches':>9s} {'median us':>10s} {'min us':>8s} {'max us':>8s}")
    for (name, grid), v in sorted(per.items()):
        print(f"{name:44s} {grid:7d} {len(v):9d} {float(np.median(v)):10.2f} {min(v):8.2f} {max(v):8.2f}")


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--summarise-trace":
        return summarise_trace(sys.argv[2])
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64, help="frames per round and loop")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=400, help="heat-map calls between the two events (>= 200)")
    ap.add_argument("--out", default="", help="also write the record to this file")
    ap.add_argument("--kernel-only", action="store_true", help="only the heat-map calls (for a kernel-trace run of a profiler)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_heatmap needs the GPU"
    assert args.launches >= 200
    import orehip
    from detectron2.engine.defaults import DefaultPredictor
    orehip.lib()
    pred = DefaultPredictor(demo_cfg())
    load_synthetic(pred.model)
    out = {"workload": "heatmap", "device": torch.cuda.get_device_name(0), "host_cpus_used": len(os.sched_getaffinity(0)),
           "date": time.strftime("%Y-%m-%d"), "frames_per_round": args.frames, "rounds": args.rounds, "launches": args.launches,
           "command": "python tools/bench_heatmap.py" + "".join(f" --{k} {v}" for k, v in (("frames", args.frames), ("rounds", args.rounds),
                                                                                             ("launches", args.launches))),
           "kernels": kernel_cases(orehip, pred, args), "predictors": [] if args.kernel_only else predictor_cases(orehip, pred, args)}
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
