"""Writes tests/golden/box_proposals_ref.npz: a seeded set of images with ground truth and proposals, and what the reference's own
_evaluate_box_proposals returns for them in the eight (limit, area) calls of "box_proposals".  Recorded data only.

    python tools/gen_box_proposals_fixture.py /path/to/reference/checkout [--out tests/golden/box_proposals_ref.npz]

The function is taken at run time from <checkout>/fewx/evaluation/coco_evaluation.py (the one function definition is compiled out of
the file; its module's imports -- pycocotools, fvcore -- are not needed) and runs on the CPU with this package's Boxes / Instances /
pairwise_iou.  The two coco_api calls it makes (getAnnIds, loadAnns) and BoxMode.convert are stubs over the generated json rows.
Logits are distinct within an image (the reference's tie order is unspecified); boxes lie on a quantised grid so exact IoU ties occur.
Never imported by a test."""
import argparse
import ast
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "faster-orefsdet_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

AREAS = ["all", "small", "medium", "large"]
LIMITS = [100, 1000]


class _BoxMode:
    XYWH_ABS, XYXY_ABS = 1, 0

    @staticmethod
    def convert(box, from_mode, to_mode):
        assert (from_mode, to_mode) == (_BoxMode.XYWH_ABS, _BoxMode.XYXY_ABS)
        x, y, w, h = (float(v) for v in box)
        return [x, y, x + w, y + h]


class _CocoApi:
    def __init__(self, annos):
        self.by_id = {a["id"]: a for a in annos}
        self.by_img = {}
        for a in annos:
            self.by_img.setdefault(a["image_id"], []).append(a["id"])

    def getAnnIds(self, imgIds):
        return list(self.by_img.get(imgIds, []))

    def loadAnns(self, ids):
        return [self.by_id[i] for i in ids]


def load_reference_function(checkout):
    from detectron2.structures import Boxes, pairwise_iou
    path = os.path.join(checkout, "fewx", "evaluation", "coco_evaluation.py")
    with open(path) as f:
        tree = ast.parse(f.read(), path)
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "_evaluate_box_proposals"]
    assert len(fn) == 1, path
    ns = {"torch": torch, "Boxes": Boxes, "BoxMode": _BoxMode, "pairwise_iou": pairwise_iou}
    exec(compile(ast.Module(body=fn, type_ignores=[]), path, "exec"), ns)
    return ns["_evaluate_box_proposals"]


def dataset(seed=0, n_img=36):
    """Images 0..: kinds by position -- GTs but no proposals, proposals but only crowd GTs, proposals and no GT at all, G > P,
    P > 100, one image with P > 1000; crowd GTs sprinkled everywhere; areas around the 32^2 and 96^2 bounds."""
    rng = np.random.default_rng(seed)
    img_ids = sorted(int(v) for v in rng.choice(900, n_img, replace=False) + 1)
    annos, entries = [], []
    q = 4.0
    for n, im in enumerate(img_ids):
        n_gt = int(rng.integers(1, 13))
        n_pr = int(rng.integers(1, 21))
        crowd_p = 0.1
        if n % 9 == 1:
            n_pr = 0
        elif n % 9 == 2:
            crowd_p = 1.0
        elif n % 9 == 3:
            n_gt = 0
        elif n % 9 == 4:
            n_gt, n_pr = 12, int(rng.integers(2, 6))
        elif n % 9 == 5:
            n_pr = int(rng.integers(101, 160))
        if n == 7:
            n_pr, n_gt = 1040, 9
        mine = []
        for _ in range(n_gt):
            x, y = rng.integers(0, 40, 2) * q
            w, h = rng.choice([8, 16, 32, 48, 96, 128, 24, 40], 2).astype(np.float64)
            area = float(w * h) if rng.random() < 0.8 else float(w * h * rng.choice([0.5, 0.25]))
            a = {"id": len(annos) + 1, "image_id": im, "category_id": int(rng.integers(1, 3)), "bbox": [float(x), float(y), float(w), float(h)],
                 "area": area, "iscrowd": int(rng.random() < crowd_p)}
            annos.append(a)
            mine.append(a)
        boxes = []
        for _ in range(n_pr):
            if mine and rng.random() < 0.6:
                a = mine[int(rng.integers(len(mine)))]
                x0, y0 = a["bbox"][0] + rng.integers(-2, 3) * q, a["bbox"][1] + rng.integers(-2, 3) * q
                x1, y1 = x0 + a["bbox"][2] + rng.integers(-2, 3) * q, y0 + a["bbox"][3] + rng.integers(-2, 3) * q
            else:
                x0, y0 = rng.integers(0, 40, 2) * q
                x1, y1 = x0 + rng.integers(1, 30) * q, y0 + rng.integers(1, 30) * q
            boxes.append([x0, y0, max(x1, x0 + q), max(y1, y0 + q)])
        logits = rng.permutation(4 * max(n_pr, 1))[:n_pr].astype(np.float32) / 8 - 20         # distinct within the image
        entries.append((im, np.array(boxes, dtype=np.float32).reshape(-1, 4), logits))
    order = rng.permutation(len(entries))
    return {"images": [{"id": i} for i in img_ids], "annotations": annos,
            "categories": [{"id": 1, "name": "ore"}, {"id": 2, "name": "gangue"}]}, [entries[i] for i in order]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("checkout", help="path of the reference checkout")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "box_proposals_ref.npz"))
    args = ap.parse_args()
    from detectron2.structures import Boxes, Instances
    fn = load_reference_function(args.checkout)
    gt, entries = dataset()
    preds = []
    for im, b, s in entries:
        p = Instances((800, 800))
        p.proposal_boxes = Boxes(torch.from_numpy(b))
        p.objectness_logits = torch.from_numpy(s)
        preds.append({"image_id": im, "proposals": p})
    api = _CocoApi(gt["annotations"])
    out = {"image_ids": np.array([i["id"] for i in gt["images"]], dtype=np.int64),
           "category_ids": np.array([c["id"] for c in gt["categories"]], dtype=np.int64),
           "ann_id": np.array([a["id"] for a in gt["annotations"]], dtype=np.int64),
           "ann_image_id": np.array([a["image_id"] for a in gt["annotations"]], dtype=np.int64),
           "ann_category_id": np.array([a["category_id"] for a in gt["annotations"]], dtype=np.int64),
           "ann_bbox": np.array([a["bbox"] for a in gt["annotations"]], dtype=np.float64),
           "ann_area": np.array([a["area"] for a in gt["annotations"]], dtype=np.float64),
           "ann_iscrowd": np.array([a["iscrowd"] for a in gt["annotations"]], dtype=np.int64),
           "entry_image_id": np.array([e[0] for e in entries], dtype=np.int64),
           "entry_count": np.array([len(e[2]) for e in entries], dtype=np.int64),
           "boxes": np.concatenate([e[1] for e in entries]), "logits": np.concatenate([e[2] for e in entries])}
    recalls, ars, num_pos, n = [], [], [], 0
    for limit in LIMITS:
        for area in AREAS:
            r = fn(preds, api, area=area, limit=limit)
            out[f"gt_overlaps_{n}"] = r["gt_overlaps"].numpy()
            recalls.append(r["recalls"].numpy())
            ars.append(r["ar"].numpy())
            num_pos.append(int(r["num_pos"]))
            n += 1
    out["thresholds"] = r["thresholds"].numpy()
    out["recalls"], out["ar"], out["num_pos"] = np.stack(recalls), np.stack(ars), np.array(num_pos, dtype=np.int64)
    np.savez_compressed(args.out, **out)
    print(f"{args.out}: {len(entries)} entries, {len(out['logits'])} proposals, {len(gt['annotations'])} annotations, "
          f"num_pos {num_pos}, ar {[float(a) for a in ars]}, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
