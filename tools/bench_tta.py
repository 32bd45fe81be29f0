"""Time test-time augmentation on the device: GeneralizedRCNNWithTTA's device path (one upload, device resizes, one engine replay per
variant with the rows collected behind it, one merge, one host wait) against the same variants through the means the package had
before it (Pillow's resize on the host, `model.inference` per variant with its host sync, inverse transforms and merge on the host),
and against the bare engine replays of the V variant shapes back to back with nothing between them.  Raw 480x640 and 300x300 uint8
images under the default TEST.AUG (MIN_SIZES 400 .. 1200, MAX_SIZE 4000, flip: 18 variants); the detector is the synthetic-weight
model of the test suite.  The three loops alternate image by image in one process; each figure is the median over the images of one
call's wall time (every call ends in a device synchronisation).  The two results are compared once, before anything is timed.
Prints one JSON line.

    python tools/bench_tta.py [--images 50] [--warmup 5] [--out profiles/tta_bench.json]
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

RAW_SIZES = [(480, 640), (300, 300)]


def build_model(max_size):
    from detectron2.modeling import build_model as build
    from fewx.config import get_cfg
    from oracle import ref_model as R
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "faster-orefsdet_amd", "configs", "fsod", "finetune_vovnet.yaml"))
    # the model's own engine (the composition's per-variant path) has to take the largest variant
    cfg.merge_from_list(["MODEL.DEVICE", "cuda", "MODEL.WEIGHTS", "", "INPUT.MAX_SIZE_TEST", max_size])
    model = build(cfg).eval()
    sd = R.synth_state_dict(0)
    sd2 = R.synth_roi_state(sd)
    sd2["roi_heads.box_head.0.fc1.weight"] = sd2["roi_heads.box_head.0.fc1.weight"] * 0.01
    model.load_state_dict(sd, strict=False)
    model.load_state_dict({k: v for k, v in sd2.items() if k.startswith("roi_heads.")}, strict=False)
    rc8 = torch.randn(24, 128, 8, 8, generator=torch.Generator().manual_seed(9)) * 0.1
    model.set_support_dict({**{k: {0: v} for k, v in R.synth_support(0).items()}, "rcnn_8": {0: rc8}, "rcnn_4": {0: torch.zeros(24, 128, 4, 4)}})
    return cfg, model


def timed(fn, arg):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn(arg)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=50, help="timed images per case and loop (>= 50)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="", help="also write the record to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_tta needs the GPU"
    assert args.images >= 50
    from PIL import Image
    import PIL
    import orehip
    from detectron2.modeling import GeneralizedRCNNWithTTA
    from detectron2.modeling import test_time_augmentation as T
    from oracle import decode as odec
    orehip.lib()
    cfg, model = build_model(1600)
    aug = (list(cfg.TEST.AUG.MIN_SIZES), cfg.TEST.AUG.MAX_SIZE, cfg.TEST.AUG.FLIP)
    thr, topk = cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST, cfg.TEST.DETECTIONS_PER_IMAGE
    tta = GeneralizedRCNNWithTTA(cfg, model)
    cases = []
    for h, w in RAW_SIZES:
        variants = T.tta_variants(h, w, *aug)
        T.check_variant_limits((h, w), variants)
        rng = np.random.default_rng(h)
        raws = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(4)]

        def device_path(raw):
            return tta([{"image_raw": raw}])[0]

        def composition(raw):
            boxes, scores, classes = [], [], []
            for v in variants:
                img = np.asarray(Image.fromarray(raw).resize((v["w"], v["h"]), Image.BILINEAR))
                img = img[:, ::-1] if v["flip"] else img
                r = model.inference([{"image": torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1)))}], do_postprocess=False)[0]
                boxes.append(T.inverse_boxes(r.pred_boxes.tensor.cpu().numpy(), T.variant_transforms((h, w), (h, w), v)))
                scores.append(r.scores.cpu().numpy())
                classes.append(r.pred_classes.cpu().numpy())
            return T.merge_detections_host(np.concatenate(boxes), np.concatenate(scores), np.concatenate(classes), (h, w), 1e-8, thr, topk,
                                           nms=odec.nms)

        got, want = device_path(raws[0]), composition(raws[0])
        i = got["instances"]
        equal = (np.array_equal(i.pred_boxes.tensor.cpu().numpy(), want[0]) and np.array_equal(i.scores.cpu().numpy(), want[1]) and
                 np.array_equal(i.pred_classes.cpu().numpy(), want[2]))
        dev_raw = torch.from_numpy(raws[0]).cuda()
        dev_variants = [orehip.resize_bilinear_u8(dev_raw, v["h"], v["w"]) for v in variants]
        engine = tta._tta_engine

        def engine_sum(_):
            for img in dev_variants:
                engine.eval_forward(img, use_graph=True)

        loops = {"tta_ms": device_path, "composition_ms": composition, "engine_sum_ms": engine_sum}
        times = {k: [] for k in loops}
        for n in range(args.warmup + args.images):
            for k, fn in loops.items():
                ms, _ = timed(fn, raws[n % len(raws)])
                if n >= args.warmup:
                    times[k].append(ms)
        rec = {"raw_hw": [h, w], "variants": len(variants), "largest_variant_hw": [variants[-1]["h"], variants[-1]["w"]],
               "equals_composition": bool(equal), "detections": int(len(i))}
        for k, v in times.items():
            rec[k] = float(np.median(v))
            rec[k.replace("_ms", "") + "_p10_p90_ms"] = [float(np.percentile(v, 10)), float(np.percentile(v, 90))]
        rec["tta_over_engine_sum"] = rec["tta_ms"] / rec["engine_sum_ms"]
        rec["composition_over_tta"] = rec["composition_ms"] / rec["tta_ms"]
        rec["tta_faster_than_composition"] = rec["tta_ms"] < rec["composition_ms"]
        cases.append(rec)
        if not equal:
            print(json.dumps(rec))
            sys.exit("the device path differs from the host composition")
    out = {"workload": "tta_default_test_aug", "device": torch.cuda.get_device_name(0), "pillow": PIL.__version__,
           "host_cpus_used": len(os.sched_getaffinity(0)), "date": time.strftime("%Y-%m-%d"), "images": args.images, "warmup": args.warmup,
           "min_sizes": aug[0], "max_size": aug[1], "flip": aug[2], "cases": cases}
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))
    if not all(c["tta_faster_than_composition"] for c in cases):
        sys.exit("tta_ms >= composition_ms in at least one case")


if __name__ == "__main__":
    main()
