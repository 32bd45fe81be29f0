"""The support set of a dataset: from detectron2-format records (DatasetCatalog.get(name); fewx/data/datasets/register_coco.py loads
them from a COCO json) to the support dataframe and the crop files that DatasetMapperWithSupport, CenterNet2Detector.init_model and
build_support_from_dataframe read: columns id / image_id / category_id / file_path / support_box, crops of 240 x 240.

The reference does not ship the script that makes them (it is part of upstream FewX's dataset tooling), so the crop is a contract of
this package, "support crop v1" (include/ore_hip.h): a square window around the box with 16 pixels of context at the crop's scale,
Pillow's BILINEAR, computed on the device by orehip.support_crops, frame by frame."""
import os

import numpy as np

COLUMNS = ["id", "image_id", "category_id", "file_path", "support_box"]
XYWH_ABS = 1          # BoxMode.XYWH_ABS


def _xyxy(ann):
    b = [float(v) for v in ann["bbox"]]
    if ann.get("bbox_mode", XYWH_ABS) == XYWH_ABS:
        b[2], b[3] = b[0] + b[2], b[1] + b[3]
    return np.asarray(b, dtype=np.float32)


def _integer_sides(box, h, w):
    """(bw, bh) of the contract's integer box: floor / ceil of the corners, intersected with the frame."""
    x1, y1, x2, y2 = (float(v) for v in box)
    return (min(int(w), int(np.ceil(x2))) - max(0, int(np.floor(x1))), min(int(h), int(np.ceil(y2))) - max(0, int(np.floor(y1))))


def select_support_annotations(records, shot=None, seed=None, one_per_image=False, min_side=1):
    """The (record, annotation, box) triples of the support set, category by category in ascending id.  Annotations are walked in
    (image id, annotation id) order; crowd annotations and boxes whose integer side is below min_side are skipped; one_per_image keeps
    the first eligible annotation of a category in an image.  Per category: every eligible annotation (shot=None), the first `shot`
    (seed=None), or `shot` of them in the order np.random.default_rng(seed).permutation draws (one generator, categories ascending)."""
    per_cat = {}
    for rec in sorted(records, key=lambda r: r["image_id"]):
        seen = set()
        for ann in sorted(rec.get("annotations", []), key=lambda a: a["id"]):
            if ann.get("iscrowd", 0):
                continue
            box = _xyxy(ann)
            if min(_integer_sides(box, rec["height"], rec["width"])) < max(int(min_side), 1):
                continue
            cat = ann["category_id"]
            if one_per_image and cat in seen:
                continue
            seen.add(cat)
            per_cat.setdefault(cat, []).append((rec, ann, box))
    rng = np.random.default_rng(seed) if seed is not None else None
    out = []
    for cat in sorted(per_cat):
        pool = per_cat[cat]
        if shot is not None:
            pool = [pool[i] for i in rng.permutation(len(pool))[:shot]] if rng is not None else pool[:shot]
        out += pool
    return out


def build_support_df(records, shot=None, image_root="./datasets/coco", out_dir="support", seed=None, one_per_image=False, min_side=1,
                     read_image=None, write=True, format="BGR", size=240, context=16, fill=None, device=None):
    """The support dataframe of `records` in the reference's columns, one row per selected annotation (select_support_annotations):
    file_path = <out_dir>/<category_id>/<annotation id>.png relative to image_root, support_box = the box inside its crop (float32 [4]).
    write=True crops every frame's boxes on the device in one call per frame (read_image(record["file_name"], format=format), default
    Pillow) and writes each crop as a PNG under image_root -- lossless, and stored so that a reader of `format` (cfg.INPUT.FORMAT) gets
    the crop's bytes back.  write=False plans on the host alone: the same dataframe, no GPU, no files.  fill defaults to
    orehip.SUPPORT_FILL (round(cfg.MODEL.PIXEL_MEAN))."""
    import pandas as pd
    import orehip
    picked = select_support_annotations(records, shot, seed, one_per_image, min_side)
    rows = []
    for rec, ann, box in picked:
        plan = orehip.support_crop_plan(rec["height"], rec["width"], box, size, context)
        rows.append({"id": ann["id"], "image_id": rec["image_id"], "category_id": ann["category_id"],
                     "file_path": "/".join((out_dir, str(ann["category_id"]), f"{ann['id']}.png")), "support_box": plan["box"]})
    df = pd.DataFrame(rows, columns=COLUMNS)
    if not write or not rows:
        return df
    import torch
    from PIL import Image
    if read_image is None:
        from .dataset_mapper import _pil_read_image as read_image
    fill = orehip.SUPPORT_FILL if fill is None else fill
    by_image = {}
    for i, (rec, _, _) in enumerate(picked):
        by_image.setdefault(rec["image_id"], []).append(i)
    for idx in by_image.values():
        rec = picked[idx[0]][0]
        frame = np.ascontiguousarray(read_image(rec["file_name"], format=format))
        if frame.shape[:2] != (rec["height"], rec["width"]):
            raise ValueError(f"{rec['file_name']}: the image is {frame.shape[0]}x{frame.shape[1]}, its record says {rec['height']}x{rec['width']}")
        crops, _ = orehip.support_crops(torch.from_numpy(frame), np.stack([picked[i][2] for i in idx]), size=size, context=context,
                                            fill=fill, device=device)
        crops = crops.permute(0, 2, 3, 1).cpu().numpy()                       # [k, S, S, 3], the frame's channel order
        for j, i in enumerate(idx):
            path = os.path.join(image_root, rows[i]["file_path"])
            os.makedirs(os.path.dirname(path), exist_ok=True)
            Image.fromarray(np.ascontiguousarray(crops[j][:, :, ::-1] if format == "BGR" else crops[j])).save(path)
    return df


def enrol_from_records(model, records, shot=None, seed=None, one_per_image=False, min_side=1, read_image=None, format=None):
    """Enrols every category of `records` in `model` (CenterNet2Detector.enrol) straight from the annotated frames: the selection of
    build_support_df, one enrol call per category over the frames that hold its shots.  Nothing is written.  Returns
    {category id: number of shots}."""
    if read_image is None:
        from .dataset_mapper import _pil_read_image as read_image
    format = format or model.input_format
    frames, per_cat = {}, {}
    for rec, ann, box in select_support_annotations(records, shot, seed, one_per_image, min_side):
        if rec["image_id"] not in frames:
            frames[rec["image_id"]] = np.ascontiguousarray(read_image(rec["file_name"], format=format))
        per_cat.setdefault(ann["category_id"], []).append((rec["image_id"], box))
    for cat, shots in per_cat.items():
        ids = list(dict.fromkeys(i for i, _ in shots))
        model.enrol([frames[i] for i in ids], np.stack([b for _, b in shots]), cls_id=cat, frame_index=[ids.index(i) for i, _ in shots])
    return {cat: len(shots) for cat, shots in per_cat.items()}
