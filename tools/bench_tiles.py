"""Time tiled inference on the device: TiledInference's device path (one upload, one gather launch, one device resize, one engine
replay per pass with the rows collected behind it, one merge, one host wait) against the same sources through the means the package
had before it (numpy crops and Pillow's resize on the host, `model.inference` / `model.inference_many` per source with its host syncs,
seam rule, transform and merge on the host), and against the bare engine replays of the same passes back to back with nothing between
them.  Frames of 1080x1920 and 2160x3840 uint8 from host memory, tile 640, overlap 128, one and eight tiles per pass; the detector is
the synthetic-weight model of the test suite.  The three loops alternate frame by frame in one process; each figure is the median over
the frames of one call's wall time (every call ends in a device synchronisation).  The two results are compared once, before anything
is timed.  The gather kernel is timed on its own: device events around back-to-back launches, its bytes (every tile read once and
written once) over that time, against the 6.3 TB/s a streaming kernel achieves on this part.  Prints one JSON line.

    python tools/bench_tiles.py [--frames 30] [--warmup 3] [--out profiles/tiles_bench.json]
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

FRAME_SIZES = [(1080, 1920), (2160, 3840)]
TILE, OVERLAP, MARGIN, FOLDS = 640, 128, 2.0, (1, 8)
HBM_ACHIEVABLE = 6.3e12


def timed(fn, arg):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn(arg)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def gather_time_ms(orehip, frame_dev, plan, reps=200):
    out = orehip.tile_gather_u8(frame_dev, plan)
    for _ in range(10):
        orehip.tile_gather_u8(frame_dev, plan, out=out)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        orehip.tile_gather_u8(frame_dev, plan, out=out)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30, help="timed frames per case and loop")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="", help="also write the record to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_tiles needs the GPU"
    assert args.frames >= 10
    from PIL import Image
    import PIL
    import orehip
    from bench_tta import build_model
    from detectron2.modeling.test_time_augmentation import merge_detections_host
    from fewx.modeling import TiledInference
    from oracle import decode as odec
    orehip.lib()
    cfg, model = build_model(1000)
    thr, topk = cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST, cfg.TEST.DETECTIONS_PER_IMAGE
    cases = []
    for h, w in FRAME_SIZES:
        rng = np.random.default_rng(h)
        raws = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(3)]
        for fold in FOLDS:
            tiled = TiledInference(cfg, model, tile=TILE, overlap=OVERLAP, margin=MARGIN, fold=fold)
            plan, full_hw = tiled.plan(h, w)
            n_tiles, th, tw = plan["ny"] * plan["nx"], plan["th"], plan["tw"]

            def device_path(raw):
                return tiled([{"image_raw": raw}])[0]

            def composition(raw):
                full = np.asarray(Image.fromarray(raw).resize((full_hw[1], full_hw[0]), Image.BILINEAR))
                srcs = [(full.transpose(2, 0, 1), dict(sx=w * 1.0 / full_hw[1], sy=h * 1.0 / full_hw[0], ox=0.0, oy=0.0, src_hw=full_hw, edges=0))]
                for i, (y0, x0) in enumerate(plan["origins"]):
                    srcs.append((raw[y0:y0 + th, x0:x0 + tw].transpose(2, 0, 1),
                                 dict(sx=1.0, sy=1.0, ox=float(x0), oy=float(y0), src_hw=(th, tw), edges=orehip.tile_edges(plan, i, h, w))))
                reqs = [{"image": torch.from_numpy(np.ascontiguousarray(img))} for img, _ in srcs]
                if fold > 1:
                    res = [model.inference(reqs[:1], do_postprocess=False)[0]] + model.inference_many(reqs[1:], do_postprocess=False, max_fold=fold)
                else:
                    res = [model.inference([r], do_postprocess=False)[0] for r in reqs]
                rows = [orehip.tile_collect_host(r.pred_boxes.tensor.cpu().numpy(), r.scores.cpu().numpy(), r.pred_classes.cpu().numpy(),
                                                 margin=MARGIN, **kw)[:3] for r, (_, kw) in zip(res, srcs)]
                return merge_detections_host(np.concatenate([r[0] for r in rows]), np.concatenate([r[1] for r in rows]),
                                             np.concatenate([r[2] for r in rows]), (h, w), 1e-8, thr, topk, nms=odec.nms)

            got, want = device_path(raws[0]), composition(raws[0])
            i = got["instances"]
            equal = (np.array_equal(i.pred_boxes.tensor.cpu().numpy(), want[0]) and np.array_equal(i.scores.cpu().numpy(), want[1]) and
                     np.array_equal(i.pred_classes.cpu().numpy(), want[2]))
            dev_raw = torch.from_numpy(raws[0]).cuda()
            dev_tiles = orehip.tile_gather_u8(dev_raw, plan)
            dev_full = orehip.resize_bilinear_u8(dev_raw, full_hw[0], full_hw[1])
            e_tile, e_full = tiled._slots["tile"].engine, tiled._slots["full"].engine

            def engine_sum(_):
                e_full.eval_forward(dev_full, use_graph=True)
                for j in range(0, n_tiles, fold):
                    if fold > 1:
                        e_tile.eval_forward_batch(dev_tiles[j:j + fold], use_graph=True)
                    else:
                        e_tile.eval_forward(dev_tiles[j], use_graph=True)

            loops = {"tiled_ms": device_path, "composition_ms": composition, "engine_sum_ms": engine_sum}
            times = {k: [] for k in loops}
            for n in range(args.warmup + args.frames):
                for k, fn in loops.items():
                    ms, _ = timed(fn, raws[n % len(raws)])
                    if n >= args.warmup:
                        times[k].append(ms)
            g_ms = gather_time_ms(orehip, dev_raw, plan)
            g_bytes = 2 * n_tiles * 3 * th * tw
            rec = {"frame_hw": [h, w], "fold": fold, "tiles": n_tiles, "tile_hw": [th, tw], "full_frame_hw": list(full_hw),
                   "passes": 1 + -(-n_tiles // fold), "equals_composition": bool(equal), "detections": int(len(i))}
            for k, v in times.items():
                rec[k] = float(np.median(v))
                rec[k.replace("_ms", "") + "_p10_p90_ms"] = [float(np.percentile(v, 10)), float(np.percentile(v, 90))]
            rec["tiled_over_engine_sum"] = rec["tiled_ms"] / rec["engine_sum_ms"]
            rec["composition_over_tiled"] = rec["composition_ms"] / rec["tiled_ms"]
            rec["tiled_faster_than_composition"] = rec["tiled_ms"] < rec["composition_ms"]
            rec["gather_us"] = g_ms * 1e3
            rec["gather_bytes"] = g_bytes
            rec["gather_bytes_per_s"] = g_bytes / (g_ms * 1e-3)
            rec["gather_share_of_6.3TBps"] = rec["gather_bytes_per_s"] / HBM_ACHIEVABLE
            cases.append(rec)
            if not equal:
                print(json.dumps(rec))
                sys.exit("the device path differs from the host composition")
            for s in tiled._slots.values():
                s.engine.close()
    for h, w in FRAME_SIZES:
        one, many = (next(c for c in cases if c["frame_hw"] == [h, w] and c["fold"] == f) for f in FOLDS)
        many["fold_gain_over_fold_1"] = one["tiled_ms"] / many["tiled_ms"]
    out = {"workload": "tiled_inference_640_128", "device": torch.cuda.get_device_name(0), "pillow": PIL.__version__,
           "host_cpus_used": len(os.sched_getaffinity(0)), "date": time.strftime("%Y-%m-%d"), "frames": args.frames, "warmup": args.warmup,
           "tile": TILE, "overlap": OVERLAP, "margin": MARGIN, "cases": cases}
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))
    if not all(c["tiled_faster_than_composition"] for c in cases):
        sys.exit("tiled_ms >= composition_ms in at least one case")


if __name__ == "__main__":
    main()
