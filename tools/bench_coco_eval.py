"""Time COCO box AP on the device: COCOEvaluator.evaluate() (gather, grouping, per-image matching, accumulation, copy-back, summary)
and the ore_coco_eval launch sequence alone, with device events after a warm-up, on a synthetic set shaped like the ore val set
(1060 images, 18825 GTs, 100 detections per image, one category).  Next to it: the CPU reference (tests/coco_ref.py) on the
same images (by default all of them), timed, with the device result on those images checked bit for bit against it -- the script
exits with status 1 when they differ.  Prints one JSON line.

    python tools/bench_coco_eval.py [--reps 10] [--ref-images 1060]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "faster-orefsdet_amd"), ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def synth(n_img=1060, n_gt=18825, per_img=100, seed=0):
    rng = np.random.default_rng(seed)
    gts_per = np.full(n_img, n_gt // n_img)
    gts_per[: n_gt - gts_per.sum()] += 1
    images, annos, dets = [], [], []
    for i in range(n_img):
        images.append({"id": i + 1, "width": 1333, "height": 800, "file_name": f"{i}.png"})
        boxes = []
        for _ in range(gts_per[i]):
            w, h = rng.uniform(8, 200, 2)
            x, y = rng.uniform(0, 1333 - w), rng.uniform(0, 800 - h)
            boxes.append((x, y, w, h))
            annos.append({"id": len(annos) + 1, "image_id": i + 1, "category_id": 1, "bbox": [x, y, w, h], "area": w * h, "iscrowd": 0})
        for _ in range(per_img):
            if rng.random() < 0.3:
                x, y, w, h = boxes[int(rng.integers(len(boxes)))]
                j = rng.normal(0, 0.08, 4) * np.array([w, h, w, h])
                x0, y0, x1, y1 = x + j[0], y + j[1], x + w + j[2], y + h + j[3]
            else:
                w, h = rng.uniform(8, 200, 2)
                x0, y0 = rng.uniform(0, 1333 - w), rng.uniform(0, 800 - h)
                x1, y1 = x0 + w, y0 + h
            dets.append((i + 1, [x0, y0, max(x1, x0 + 1), max(y1, y0 + 1)], float(rng.random())))
    return {"images": images, "annotations": annos, "categories": [{"id": 1, "name": "ore"}]}, dets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--ref-images", type=int, default=1060, help="images the CPU reference evaluates and the device is checked on "
                                                                 "(the first N; 0: skip the reference)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_coco_eval needs the GPU"
    import orehip
    from detectron2.data import MetadataCatalog
    from detectron2.evaluation import COCOEvaluator
    from detectron2.evaluation.coco_evaluation import AREA_RNG, IOU_THRS, MAX_DETS, REC_THRS
    from detectron2.structures import Boxes, Instances
    orehip.lib()
    gt, dets = synth()
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "gt.json")
    json.dump(gt, open(path, "w"))
    MetadataCatalog.get("bench_coco_eval").set(json_file=path)
    ev = COCOEvaluator("bench_coco_eval", distributed=False)
    dev = torch.device("cuda")
    per_image = {}
    for im, b, s in dets:
        per_image.setdefault(im, []).append((b, s))
    outputs = []
    for im in sorted(per_image):
        inst = Instances((800, 1333))
        inst.pred_boxes = Boxes(torch.tensor([b for b, _ in per_image[im]], dtype=torch.float32, device=dev))
        inst.scores = torch.tensor([s for _, s in per_image[im]], dtype=torch.float32, device=dev)
        inst.pred_classes = torch.zeros(len(per_image[im]), dtype=torch.int64, device=dev)
        outputs.append(({"image_id": im}, {"instances": inst}))
    torch.cuda.synchronize()

    def run_evaluate():
        ev.reset()
        for inp, out in outputs:
            ev.process([inp], [out])
        return ev.evaluate()

    res = run_evaluate()                                       # warm-up: code objects, device copy of the GT, workspace
    t_eval = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        run_evaluate()
        b.record()
        torch.cuda.synchronize()
        t_eval.append(a.elapsed_time(b))
    # the launch sequence alone, inputs already on the device
    g = ev._gt
    boxes = torch.cat([o["instances"].pred_boxes.tensor for _, o in outputs])
    scores = torch.cat([o["instances"].scores for _, o in outputs])
    img = torch.repeat_interleave(torch.arange(len(outputs), dtype=torch.int32), 100).to(dev)
    cat = torch.zeros_like(img)
    gd = g.device(dev)
    ws = ev._workspace
    orehip.coco_eval(boxes, scores, img, cat, gd, len(g.img_ids), 1, IOU_THRS, REC_THRS, AREA_RNG, MAX_DETS, workspace=ws)
    t_kern = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        orehip.coco_eval(boxes, scores, img, cat, gd, len(g.img_ids), 1, IOU_THRS, REC_THRS, AREA_RNG, MAX_DETS, workspace=ws)
        b.record()
        torch.cuda.synchronize()
        t_kern.append(a.elapsed_time(b))
    out = {"workload": "coco_bbox_eval", "images": len(gt["images"]), "gts": len(gt["annotations"]), "dets": len(dets),
           "evaluate_ms_median": float(np.median(t_eval)), "evaluate_ms_min": float(np.min(t_eval)),
           "device_eval_ms_median": float(np.median(t_kern)), "device_eval_ms_min": float(np.min(t_kern)), "reps": args.reps,
           "AP": res["bbox"]["AP"], "AP50": res["bbox"]["AP50"], "AP75": res["bbox"]["AP75"]}
    if args.ref_images > 0:
        import coco_ref
        keep = set(range(1, args.ref_images + 1))
        sub = {"images": [i for i in gt["images"] if i["id"] in keep], "annotations": [a for a in gt["annotations"] if a["image_id"] in keep],
               "categories": gt["categories"]}
        rows = []
        for im, b, s in dets:
            if im in keep:
                x0, y0, x1, y1 = np.float32(b)
                rows.append({"image_id": im, "category_id": 1, "bbox": [float(x0), float(y0), float(x1 - x0), float(y1 - y0)], "score": float(np.float32(s))})
        t0 = time.perf_counter()
        ref = coco_ref.evaluate(sub, rows)
        t_ref = time.perf_counter() - t0
        MetadataCatalog.get("bench_coco_eval_sub").set(json_file=os.path.join(tmp, "sub.json"))
        json.dump(sub, open(os.path.join(tmp, "sub.json"), "w"))
        ev2 = COCOEvaluator("bench_coco_eval_sub", distributed=False)
        ev2.reset()
        for inp, o in outputs[: args.ref_images]:
            ev2.process([inp], [o])
        ev2.evaluate()
        same = all(getattr(ev2, k).tobytes() == ref[k].tobytes() for k in ("precision", "recall", "scores"))
        out.update({"ref_images": args.ref_images, "ref_cpu_s": t_ref, "ref_bitwise_equal": same})
        if args.ref_images < len(gt["images"]):
            out["ref_cpu_s_scaled_to_full_set"] = t_ref * len(gt["images"]) / args.ref_images     # linear extrapolation, not measured
        print(json.dumps(out))
        if not same:
            sys.exit("device precision / recall / scores differ from tests/coco_ref.py")
        return
    print(json.dumps(out))


if __name__ == "__main__":
    main()
