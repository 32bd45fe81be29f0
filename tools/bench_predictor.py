"""Time the raw-image path on the device: DefaultPredictor (host image -> pinned copy -> device resize -> detector) against what a
caller had to do without it (Pillow's BILINEAR resize on the host, then the same detector), and the resize kernel alone against its
roofline.  Raw 480x640 and 1080x1920 uint8 images under the test sizes of finetune_vovnet.yaml (320 / 1000) and of Base-FSOD-C4.yaml
(600 / 1000); the detector is the synthetic-weight model of the test suite (the ore weights are not shipped; the time does not depend
on the weights' values).  The three loops alternate round by round in one process; each figure is the median over rounds of the
round's mean.  Every resized image is checked against Pillow once, byte for byte, before anything is timed.  Prints one JSON line.

    python tools/bench_predictor.py [--images 40] [--rounds 5] [--launches 400] [--out profiles/predictor_bench.json]
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
RAW_SIZES = [(480, 640), (1080, 1920)]
TEST_SIZES = [(320, 1000), (600, 1000)]


def build_predictor(min_size, max_size):
    from detectron2.engine.defaults import DefaultPredictor
    from fewx.config import get_cfg
    from oracle import ref_model as R
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "faster-orefsdet_amd", "configs", "fsod", "finetune_vovnet.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", "cuda", "MODEL.WEIGHTS", "", "INPUT.MIN_SIZE_TEST", min_size, "INPUT.MAX_SIZE_TEST", max_size])
    pred = DefaultPredictor(cfg)
    sd = R.synth_state_dict(0)
    sd2 = R.synth_roi_state(sd)
    sd2["roi_heads.box_head.0.fc1.weight"] = sd2["roi_heads.box_head.0.fc1.weight"] * 0.01
    pred.model.load_state_dict(sd, strict=False)
    pred.model.load_state_dict({k: v for k, v in sd2.items() if k.startswith("roi_heads.")}, strict=False)
    rc8 = torch.randn(24, 128, 8, 8, generator=torch.Generator().manual_seed(9)) * 0.1
    pred.model.set_support_dict({**{k: {0: v} for k, v in R.synth_support(0).items()}, "rcnn_8": {0: rc8}, "rcnn_4": {0: torch.zeros(24, 128, 4, 4)}})
    return pred


def kernel_us(orehip, dev_img, nh, nw, form, launches):
    """Mean time of one resize over `launches` back-to-back launches between two device events, after a warm-up of the same length / 4."""
    out = torch.empty(3, nh, nw, dtype=torch.uint8, device="cuda")
    for _ in range(max(launches // 4, 10)):
        orehip.resize_bilinear_u8(dev_img, nh, nw, out=out, form=form)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(launches):
        orehip.resize_bilinear_u8(dev_img, nh, nw, out=out, form=form)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / launches


def loop_ms(fn, images):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for img in images:
        fn(img)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / len(images)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=40, help="images per round and loop")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=400, help="resize launches between the two events (>= 200)")
    ap.add_argument("--out", default="", help="also write the record to this file")
    ap.add_argument("--kernel-only", action="store_true", help="only the resize launches (for a kernel-trace run of a profiler)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_predictor needs the GPU"
    assert args.launches >= 200
    import PIL
    from PIL import Image
    import orehip
    orehip.lib()
    cases = []
    for min_size, max_size in TEST_SIZES:
        pred = None if args.kernel_only else build_predictor(min_size, max_size)
        model = pred.model if pred is not None else None
        for h, w in RAW_SIZES:
            rng = np.random.default_rng(h + min_size)
            raws = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(4)]
            images = [raws[i % len(raws)] for i in range(args.images)]
            nh, nw = orehip.resize_shortest_edge_shape(h, w, min_size, max_size)
            dev_raw = torch.from_numpy(raws[0]).cuda()
            want = np.asarray(Image.fromarray(raws[0]).resize((nw, nh), Image.BILINEAR)).transpose(2, 0, 1)
            form = orehip.resize_form(h, w, nh, nw)
            equal = all(np.array_equal(orehip.resize_bilinear_u8(dev_raw, nh, nw, form=f).cpu().numpy(), want)
                        for f in (orehip.RESIZE_FORM_LDS, orehip.RESIZE_FORM_WORKSPACE))
            resized_dev = orehip.resize_bilinear_u8(dev_raw, nh, nw)

            def host_pil(raw):
                img = np.ascontiguousarray(np.asarray(Image.fromarray(raw).resize((nw, nh), Image.BILINEAR)).transpose(2, 0, 1))
                return model([{"image": torch.from_numpy(img), "height": h, "width": w}])

            def model_only(_):
                return model([{"image": resized_dev, "height": h, "width": w}])

            def pil_only(raw):
                return np.ascontiguousarray(np.asarray(Image.fromarray(raw).resize((nw, nh), Image.BILINEAR)).transpose(2, 0, 1))

            stage = torch.empty(h * w * 3, dtype=torch.uint8, pin_memory=True)
            dst = torch.empty(h, w, 3, dtype=torch.uint8, device="cuda")

            def copy_only(raw):                                    # the predictor's upload: host copy into pinned memory, then the device copy
                torch.cuda.current_stream().synchronize()
                stage.view(h, w, 3).copy_(torch.from_numpy(raw))
                dst.copy_(stage.view(h, w, 3), non_blocking=True)

            loops = {"predictor_ms_per_image": pred, "host_pil_ms_per_image": host_pil, "model_only_ms_per_image": model_only,
                     "host_pil_resize_only_ms": pil_only, "upload_only_ms": copy_only}
            if args.kernel_only:
                loops = {}
            n_det = len(pred(raws[0])["instances"]) if pred is not None else -1
            for fn in loops.values():                              # warm-up: engine build and graph capture at this size, tables, pinned buffers
                loop_ms(fn, images[:8])
            per_round = {k: [] for k in loops}
            for _ in range(args.rounds):
                for k, fn in loops.items():
                    per_round[k].append(loop_ms(fn, images))
            rec = {"raw_hw": [h, w], "min_size_test": min_size, "max_size_test": max_size, "resized_hw": [nh, nw], "form": form,
                   "equals_pillow": bool(equal), "detections": n_det}
            for k, v in per_round.items():
                rec[k] = float(np.median(v))
                rec[k.replace("_ms_per_image", "").replace("_ms", "") + "_round_spread_ms"] = [float(np.min(v)), float(np.max(v))]
            bytes_moved = 3 * h * w + 3 * nh * nw
            for name, f in (("lds", orehip.RESIZE_FORM_LDS), ("two_launch", orehip.RESIZE_FORM_WORKSPACE)):
                us = kernel_us(orehip, dev_raw, nh, nw, f, args.launches)
                rec[f"resize_kernel_us_{name}"] = us
                rec[f"resize_hbm_fraction_{name}"] = bytes_moved / (us * 1e-6) / HBM_COPY_BYTES_PER_S
            rec["resize_kernel_us"] = rec["resize_kernel_us_lds" if form == orehip.RESIZE_FORM_LDS else "resize_kernel_us_two_launch"]
            rec["resize_bytes_moved"] = bytes_moved
            rec["predictor_faster_than_host_pil"] = args.kernel_only or rec["predictor_ms_per_image"] < rec["host_pil_ms_per_image"]
            cases.append(rec)
            if not equal:
                print(json.dumps(rec))
                sys.exit("the device resize differs from Pillow")
    out = {"workload": "default_predictor_raw_image", "device": torch.cuda.get_device_name(0), "pillow": PIL.__version__,
           "host_cpus_used": len(os.sched_getaffinity(0)), "date": time.strftime("%Y-%m-%d"), "images_per_round": args.images,
           "rounds": args.rounds, "launches": args.launches, "hbm_copy_bytes_per_s": HBM_COPY_BYTES_PER_S, "cases": cases}
    line = json.dumps(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(line)
    if not all(c["predictor_faster_than_host_pil"] for c in cases):
        sys.exit("predictor_ms_per_image >= host_pil_ms_per_image in at least one case")


if __name__ == "__main__":
    main()
