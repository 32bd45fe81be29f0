"""Proposal recall (AR@100 .. ARl@1000 of "box_proposals") restated from its contract, in numpy fp32 operations one by one;
the last two fp32 steps (recalls, ar) with torch, as the contract allows.  What csrc/ore_proposal_recall.hip is pinned against, and
itself pinned against the reference's recorded results in tests/golden/box_proposals_ref.npz.

For one prediction entry, one area range [lo, hi] and one limit:
  proposals by logit descending, ties in input order; the image's non-crowd annotations in json order, every category, as
  fp32(x), fp32(y), fp32(x + w), fp32(y + h) (sums in fp64) with area fp32(area); no such GT or no proposal: nothing.  The valid GTs
  are those with fp32(lo) <= area <= fp32(hi); their count goes to num_pos; none: nothing more.  Proposals cut to the first `limit`;
  IoU in fp32 as detectron2's pairwise_iou; min(P', G) times the largest remaining entry (ties: lowest GT, then lowest proposal) is
  recorded and its row and column retired; the rest of the G-long vector is 0."""
import numpy as np
import torch

AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
AREA_LBL = ["all", "small", "medium", "large"]
AREA_SUFFIX = ["", "s", "m", "l"]
LIMITS = [100, 1000]
KEYS = ["AR{}@{:d}".format(s, l) for l in LIMITS for s in AREA_SUFFIX]


def thresholds():
    return torch.arange(0.5, 0.95 + 1e-5, 0.05, dtype=torch.float32)


def image_gts(gt_json):
    """{image id: (XYXY fp32 [G, 4], area fp32 [G])} of the non-crowd annotations, json order, every category."""
    out = {}
    for a in gt_json.get("annotations", []):
        if a.get("iscrowd", 0) != 0:
            continue
        x, y, w, h = (float(v) for v in a["bbox"])
        b, ar = out.setdefault(a["image_id"], ([], []))
        b.append([np.float32(x), np.float32(y), np.float32(x + w), np.float32(y + h)])
        ar.append(np.float32(float(a["area"])))
    return {k: (np.array(b, dtype=np.float32).reshape(-1, 4), np.array(ar, dtype=np.float32)) for k, (b, ar) in out.items()}


def pairwise_iou(p, g):
    """detectron2's pairwise_iou on fp32 arrays: [P, 4] x [G, 4] -> [P, G]."""
    ap = (p[:, 2] - p[:, 0]) * (p[:, 3] - p[:, 1])
    ag = (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1])
    iw = np.maximum(np.minimum(p[:, None, 2], g[None, :, 2]) - np.maximum(p[:, None, 0], g[None, :, 0]), np.float32(0))
    ih = np.maximum(np.minimum(p[:, None, 3], g[None, :, 3]) - np.maximum(p[:, None, 1], g[None, :, 1]), np.float32(0))
    inter = iw * ih
    union = ap[:, None] + ag[None, :] - inter
    out = np.zeros_like(inter)
    np.divide(inter, union, out=out, where=inter > 0)
    assert out.dtype == np.float32
    return out


def entry_vector(boxes, logits, gt_xyxy, gt_area, area_range, limit):
    """(the recorded vector fp32 [valid GTs] or None when the entry records nothing, what it adds to num_pos)."""
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    logits = np.asarray(logits, dtype=np.float32).reshape(-1)
    if len(gt_xyxy) == 0 or len(logits) == 0:
        return None, 0
    order = np.argsort(-logits, kind="stable")
    lo, hi = np.float32(area_range[0]), np.float32(area_range[1])
    g = gt_xyxy[(gt_area >= lo) & (gt_area <= hi)]
    if len(g) == 0:
        return None, 0
    p = boxes[order][:limit] if limit is not None else boxes[order]
    m = pairwise_iou(p, g)
    vec = np.zeros(len(g), dtype=np.float32)
    for j in range(min(len(p), len(g))):
        v = m.max()
        ps, gs = np.nonzero(m == v)
        gi = gs.min()
        pi = ps[gs == gi].min()
        vec[j] = v
        m[pi, :] = -1
        m[:, gi] = -1
    return vec, len(g)


def evaluate(gt_json, entries, area="all", limit=None):
    """entries: [(image id, boxes [P, 4] XYXY fp32, logits [P] fp32)].  Returns gt_overlaps (sorted fp32), recalls, ar (fp32), num_pos,
    counts (overlaps >= threshold, int64) and per_entry (the recorded vector of every entry, None where it records nothing)."""
    gts = image_gts(gt_json)
    rng = AREA_RNG[AREA_LBL.index(area)] if isinstance(area, str) else area
    empty = (np.zeros((0, 4), np.float32), np.zeros(0, np.float32))
    per_entry, num_pos = [], 0
    for img, boxes, logits in entries:
        gx, ga = gts.get(img, empty)
        vec, n = entry_vector(boxes, logits, gx, ga, rng, limit)
        per_entry.append(vec)
        num_pos += n
    vecs = [v for v in per_entry if v is not None]
    ov = np.sort(np.concatenate(vecs)) if vecs else np.zeros(0, np.float32)
    t_ov = torch.from_numpy(ov)
    thr = thresholds()
    recalls = torch.zeros_like(thr)
    counts = np.zeros(len(thr), dtype=np.int64)
    for i, t in enumerate(thr):
        counts[i] = int((t_ov >= t).sum())
        recalls[i] = (t_ov >= t).float().sum() / float(num_pos)
    return {"gt_overlaps": ov, "recalls": recalls.numpy(), "ar": recalls.mean().numpy(), "num_pos": num_pos, "counts": counts,
            "per_entry": per_entry}


def evaluate_all(gt_json, entries):
    """The eight (limit, area) calls in the key order of "box_proposals": {key: evaluate(...)}."""
    return {"AR{}@{:d}".format(s, l): evaluate(gt_json, entries, a, l) for l in LIMITS for a, s in zip(AREA_LBL, AREA_SUFFIX)}


def box_proposals(gt_json, entries):
    """results["box_proposals"] of the evaluator: float(ar) * 100 per key."""
    return {k: float(r["ar"].item() * 100) for k, r in evaluate_all(gt_json, entries).items()}


def load_fixture(path):
    """tests/golden/box_proposals_ref.npz -> (gt json, entries, the recorded arrays)."""
    z = dict(np.load(path))
    annos = [{"id": int(i), "image_id": int(im), "category_id": int(c), "bbox": [float(v) for v in b], "area": float(ar), "iscrowd": int(cr)}
             for i, im, c, b, ar, cr in zip(z["ann_id"], z["ann_image_id"], z["ann_category_id"], z["ann_bbox"], z["ann_area"], z["ann_iscrowd"])]
    gt = {"images": [{"id": int(i)} for i in z["image_ids"]], "annotations": annos,
          "categories": [{"id": int(c), "name": f"c{int(c)}"} for c in z["category_ids"]]}
    off = np.concatenate([[0], np.cumsum(z["entry_count"])])
    entries = [(int(im), z["boxes"][off[i]:off[i + 1]], z["logits"][off[i]:off[i + 1]]) for i, im in enumerate(z["entry_image_id"])]
    return gt, entries, z
