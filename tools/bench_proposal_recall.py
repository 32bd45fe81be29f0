"""Time proposal recall on the device: COCOEvaluator.evaluate() on proposals only (gather, concatenation, launches, copy-back, the eight
AR numbers) and the ore_proposal_recall launch sequence alone, with device events after a warm-up, on a synthetic set shaped like the
ore val set (1060 images, up to 35 GTs and up to 256 proposals per image).  Next to it: the CPU restatement
(tests/proposal_recall_ref.py) on the same set, timed, with the device result checked bit for bit against it -- the script exits with
status 1 when they differ.  Prints one JSON line; --out also writes it to a file.

    python tools/bench_proposal_recall.py [--reps 10] [--out profiles/proposal_recall_bench.json]
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


def synth(n_img=1060, max_gt=35, max_prop=256, seed=0):
    rng = np.random.default_rng(seed)
    images, annos, entries = [], [], []
    for i in range(n_img):
        images.append({"id": i + 1, "width": 1333, "height": 800, "file_name": f"{i}.png"})
        boxes = []
        for _ in range(int(rng.integers(1, max_gt + 1))):
            w, h = rng.uniform(8, 200, 2)
            x, y = rng.uniform(0, 1333 - w), rng.uniform(0, 800 - h)
            boxes.append((x, y, w, h))
            annos.append({"id": len(annos) + 1, "image_id": i + 1, "category_id": 1, "bbox": [x, y, w, h], "area": w * h,
                          "iscrowd": int(rng.random() < 0.02)})
        props = []
        for _ in range(int(rng.integers(max_prop // 2, max_prop + 1))):
            if rng.random() < 0.3:
                x, y, w, h = boxes[int(rng.integers(len(boxes)))]
                j = rng.normal(0, 0.08, 4) * np.array([w, h, w, h])
                x0, y0, x1, y1 = x + j[0], y + j[1], x + w + j[2], y + h + j[3]
            else:
                w, h = rng.uniform(8, 200, 2)
                x0, y0 = rng.uniform(0, 1333 - w), rng.uniform(0, 800 - h)
                x1, y1 = x0 + w, y0 + h
            props.append([x0, y0, max(x1, x0 + 1), max(y1, y0 + 1)])
        entries.append((i + 1, np.array(props, dtype=np.float32), rng.normal(size=len(props)).astype(np.float32)))
    return {"images": images, "annotations": annos, "categories": [{"id": 1, "name": "ore"}]}, entries


def _timed(fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_proposal_recall needs the GPU"
    import orehip
    import proposal_recall_ref as R
    from detectron2.data import MetadataCatalog
    from detectron2.evaluation import COCOEvaluator
    from detectron2.evaluation.coco_evaluation import AREA_RNG, PROPOSAL_LIMITS, proposal_iou_thrs, proposal_recalls
    from detectron2.structures import Boxes, Instances
    orehip.lib()
    gt, entries = synth()
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "gt.json")
    json.dump(gt, open(path, "w"))
    MetadataCatalog.get("bench_proposal_recall").set(json_file=path)
    ev = COCOEvaluator("bench_proposal_recall", distributed=False)
    dev = torch.device("cuda")
    outputs = []
    for im, b, s in entries:
        p = Instances((800, 1333))
        p.proposal_boxes = Boxes(torch.from_numpy(b).to(dev))
        p.objectness_logits = torch.from_numpy(s).to(dev)
        outputs.append(({"image_id": im}, {"proposals": p}))
    torch.cuda.synchronize()

    def run_evaluate():
        ev.reset()
        for inp, out in outputs:
            ev.process([inp], [out])
        return ev.evaluate()

    res = run_evaluate()                                       # warm-up: code objects, device copy of the GT, workspace
    t_eval = _timed(run_evaluate, args.reps)
    # the launch sequence alone, inputs already on the device
    g = ev._gt
    boxes = torch.cat([o["proposals"].proposal_boxes.tensor for _, o in outputs])
    logits = torch.cat([o["proposals"].objectness_logits for _, o in outputs])
    counts = [len(e[2]) for e in entries]
    img_idx = [g.img_index[e[0]] for e in entries]
    gd, thr, ws = g.device_images(dev), proposal_iou_thrs().numpy(), ev._proposal_workspace
    call = lambda per_image=False: orehip.proposal_recall(boxes, logits, counts, img_idx, gd, g.img_off, AREA_RNG, PROPOSAL_LIMITS, thr,
                                                          per_image=per_image, workspace=ws)
    call()
    t_kern = _timed(call, args.reps)
    got = {k: v.cpu().numpy() for k, v in call(True).items()}
    t0 = time.perf_counter()
    ref = R.evaluate_all(gt, entries)
    t_ref = time.perf_counter() - t0
    same = int(got["status"][0]) == 0
    for c, (key, r) in enumerate(ref.items()):
        n = r["num_pos"]
        recalls, ar = proposal_recalls(torch.from_numpy(got["counts"][c]), int(got["num_pos"][c]))
        same = same and int(got["num_pos"][c]) == n and got["gt_overlaps"][c, :n].tobytes() == r["gt_overlaps"].tobytes() and \
            recalls.numpy().tobytes() == r["recalls"].tobytes() and ar.numpy().tobytes() == r["ar"].tobytes() and \
            res["box_proposals"][key] == float(r["ar"].item() * 100)
    out = {"workload": "proposal_recall", "images": len(gt["images"]), "gts": len(gt["annotations"]), "proposals": int(sum(counts)),
           "evaluate_ms_median": float(np.median(t_eval)), "evaluate_ms_min": float(np.min(t_eval)),
           "device_call_ms_median": float(np.median(t_kern)), "device_call_ms_min": float(np.min(t_kern)), "reps": args.reps,
           "ref_cpu_s": t_ref, "ref_bitwise_equal": bool(same), **{k: v for k, v in res["box_proposals"].items()}}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    if not same:
        sys.exit("the device result differs from tests/proposal_recall_ref.py")


if __name__ == "__main__":
    main()
