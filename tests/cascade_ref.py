"""The cascade of CustomCascadeROIHeads (K = len(ROI_BOX_CASCADE_HEAD.IOUS) > 1 stages; csrc/ore_roi.hip: k_roi_cascade_mb<*, CASC_REFINE |
CASC_LAST>, k_cascade_relabel): its reference and its case table.

The reference is COMPOSED from the existing C twin (oracle/ref_decode.c::oracle_roi_predict, oracle_nms), nothing is added to oracle/:
for stage k the twin's raw_boxes / raw_scores on (h_k, the stage's weights, the stage's boxes) are the next stage's boxes and the stage's
foreground probability; the final candidates are scored with the numpy-fp32 mean `(s_0 + ... + s_{K-1}) * float32(1.0 / K)` (fp32 sum in
stage order, fp32-rounded reciprocal: ref:fewx/modeling/fsod/fsod_roi_heads.py:442-445), then oracle.decode.nms and keep[:topk].  K-split
partial sums go through roitail_ref.sum_parts, detector_postprocess and the record through roitail_ref.postprocess / fill_record.

The training seam (`relabel`) decodes with the same twin (deltas through an identity box head, so apply_deltas, the log(1000/16)
clamp, ore_expf and the clip are the twin's own) and restates the rest -- non-empty test, pairwise_iou, the match and the label -- in
numpy float32, one IEEE operation per step.  `fault` seeds one error in either; tests/test_cascade_host.py shows that every fault
changes at least one case of the table.
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

import roitail_ref as RT
from oracle import decode as odec

F32 = np.float32
# detectron2's published cascade values (configs/fsod/finetune_vovnet_cascade.yaml)
REG_W = ((10.0, 10.0, 5.0, 5.0), (20.0, 20.0, 10.0, 10.0), (30.0, 30.0, 15.0, 15.0))
IOUS = (0.6, 0.7, 0.8)
EVAL_FAULTS = ("stage0_weights", "mean_before_sum", "inv_k_double")
TRAIN_FAULTS = ("keep_empty", "iou_gt", "tie_last")
FAULTS = EVAL_FAULTS + TRAIN_FAULTS


def synth_cascade_state(sd: Dict, seed: int = 0, stages: int = 3, C: int = 128) -> Dict:
    """oracle.ref_model.synth_roi_state's second stage plus seeded box_head.k / box_predictor.k for the stages k >= 1 (reference shapes)."""
    import torch
    g = torch.Generator().manual_seed(seed + 7000)

    def u(*shape, b):
        return (torch.rand(*shape, generator=g) * 2 - 1) * b
    sd = dict(sd)
    p = "roi_heads."
    for k in range(1, stages):
        sd[p + f"box_head.{k}.fc1.weight"], sd[p + f"box_head.{k}.fc1.bias"] = u(128, C * 64, b=(C * 64) ** -0.5 * 3), u(128, b=0.1)
        sd[p + f"box_predictor.{k}.cls_score.weight"], sd[p + f"box_predictor.{k}.cls_score.bias"] = u(2, 128, b=0.5), u(2, b=0.1)
        sd[p + f"box_predictor.{k}.bbox_pred.weight"], sd[p + f"box_predictor.{k}.bbox_pred.bias"] = u(4, 128, b=0.3), u(4, b=0.1)
    return sd


# ---- eval ---------------------------------------------------------------------------------------------------------------------------
def _twin_rows(h, head, boxes, reg_w, img):
    """The twin's per-row outputs with the filter and the NMS switched off: (raw boxes, raw scores, finite mask)."""
    n = len(h)
    tw = odec.roi_predict(h, head[0], head[1], head[2], head[3], np.asarray(boxes, F32).reshape(-1, 4)[:n] if n else np.zeros((0, 4), F32),
                          reg_w, img, -1.0, 2.0, -1)
    fin = np.zeros(n, bool)
    fin[tw["src"]] = True
    return tw["raw_boxes"].copy(), tw["raw_scores"].copy(), fin


def refine(h, head, boxes, reg_w, img, score_sum=None, dead=None):
    """One intermediate stage on n rows: (next boxes [n,4], score_sum [n], dead [n] bool).  A dead row (unclipped box or score not
    finite, now or in an earlier stage) has next box (0,0,0,0) and sum 0."""
    rb, rs, fin = _twin_rows(h, head, boxes, reg_w, img)
    d = ~fin if dead is None else (np.asarray(dead, bool) | ~fin)
    with np.errstate(invalid="ignore", over="ignore"):
        s = rs if score_sum is None else (np.asarray(score_sum, F32) + rs)
    assert s.dtype == F32
    rb[d] = 0
    s = s.copy()
    s[d] = 0
    return rb, s, d


def cascade_eval(hs: Sequence[np.ndarray], heads: Sequence[Tuple], boxes: np.ndarray, reg_ws: Sequence, img, score_thresh, nms_thresh, topk,
                 fault: Optional[str] = None) -> Dict[str, object]:
    """K = len(hs) stages on n = len(hs[0]) rows; hs[k] the fc1 rows of stage k (the caller pooled stage k's boxes, or, for the
    kernel tests, drew them), heads[k] = (cls_w, cls_b, box_w, box_b).  Returns the per-stage input boxes, score_sum / dead in front of
    the last stage, the last stage's raw boxes and mean scores, and the detections (boxes, scores, src)."""
    K = len(hs)
    n = len(hs[0])
    cur = np.asarray(boxes, F32).reshape(-1, 4)[:n].copy()
    stage_boxes = [cur]
    ssum = dead = None
    for k in range(K - 1):
        kk = 0 if fault == "stage0_weights" else k
        nxt, s2, dead = refine(hs[k], heads[kk], cur, reg_ws[kk], img, ssum, dead)
        ssum, cur = s2, nxt
        stage_boxes.append(cur)
    kl = 0 if fault == "stage0_weights" else K - 1
    rb, rs, fin = _twin_rows(hs[K - 1], heads[kl], cur, reg_ws[kl], img)
    with np.errstate(invalid="ignore", over="ignore"):
        if K == 1:
            score = rs
        elif fault == "mean_before_sum":                       # every stage scaled first, then added
            inv = F32(1.0 / K)
            parts = _per_stage_scores(hs, heads, stage_boxes, reg_ws, img)
            score = parts[0] * inv
            for k in range(1, K):
                score = score + parts[k] * inv
        elif fault == "inv_k_double":                          # the product carried out in double
            score = ((ssum + rs).astype(np.float64) * (1.0 / K)).astype(F32)
        else:
            score = (ssum + rs) * F32(1.0 / K)
    assert score.dtype == F32
    alive = fin if dead is None else (fin & ~dead)
    with np.errstate(invalid="ignore"):
        ok = alive & (score > F32(score_thresh))
    comp = np.nonzero(ok)[0]
    keep = odec.nms(rb[comp], score[comp], nms_thresh) if len(comp) else np.zeros(0, np.int64)
    if topk >= 0:
        keep = keep[:topk]
    return {"stage_boxes": stage_boxes, "score_sum": ssum, "dead": dead, "raw_boxes": rb, "raw_scores": score, "ok": ok,
            "boxes": rb[comp][keep], "scores": score[comp][keep], "src": comp[keep].astype(np.int64)}


def _per_stage_scores(hs, heads, stage_boxes, reg_ws, img):
    return [_twin_rows(hs[k], heads[k], stage_boxes[k], reg_ws[k], img)[1] for k in range(len(hs))]


# ---- the training seam --------------------------------------------------------------------------------------------------------------
_EYE = (np.zeros((2, 4), F32), np.zeros(2, F32), np.eye(4, dtype=F32), np.zeros(4, F32))
PAD_BOX = np.array([0.0, 0.0, 8.0, 8.0], F32)


def relabel(boxes, deltas, valid, img_hw, gtp, gt_n, reg_w, thr, fault: Optional[str] = None):
    """boxes / deltas [B,R,4], valid [B,R] bool, img_hw [B,2] (h, w), gtp [B,G,4], gt_n [B] -> (boxes' [B,R,4], labels [B,R] int64,
    matched gt [B,R,4], valid' [B,R] bool, matched index [B,R] int64 (-1: none))."""
    boxes, deltas = np.asarray(boxes, F32), np.asarray(deltas, F32)
    B, R, _ = boxes.shape
    ob = np.tile(PAD_BOX, (B, R, 1))
    og = np.zeros((B, R, 4), F32)
    ol = np.ones((B, R), np.int64)
    ov = np.zeros((B, R), bool)
    oi = np.full((B, R), -1, np.int64)
    thr = F32(thr)
    for b in range(B):
        nb, _, fin = _twin_rows(deltas[b], _EYE, boxes[b], reg_w, (float(img_hw[b][0]), float(img_hw[b][1])))
        w, h = nb[:, 2] - nb[:, 0], nb[:, 3] - nb[:, 1]
        ok = np.asarray(valid[b], bool) & fin
        if fault != "keep_empty":
            ok = ok & (w > 0) & (h > 0)
        gn = int(min(max(int(gt_n[b]), 0), gtp.shape[1]))
        g = np.asarray(gtp[b][:gn], F32).reshape(-1, 4)
        ga = (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1])
        ac = w * h
        ob[b][ok] = nb[ok]
        ov[b] = ok
        if gn == 0 or not ok.any():
            continue
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            # pairwise_iou, [R][G]: every line one fp32 operation per element
            iw = np.maximum(np.minimum(g[None, :, 2], nb[:, None, 2]) - np.maximum(g[None, :, 0], nb[:, None, 0]), F32(0))
            ih = np.maximum(np.minimum(g[None, :, 3], nb[:, None, 3]) - np.maximum(g[None, :, 1], nb[:, None, 1]), F32(0))
            inter = iw * ih
            den = (ga[None, :] + ac[:, None]) - inter
            iou = np.where(inter > 0, inter / den, F32(0))
        assert iou.dtype == F32
        bi = (gn - 1 - np.argmax(iou[:, ::-1], 1)) if fault == "tie_last" else np.argmax(iou, 1)     # argmax: the first maximum
        best = iou[np.arange(R), bi]
        fg = (best > thr) if fault == "iou_gt" else (best >= thr)
        ol[b][ok] = np.where(fg, 0, 1)[ok]
        og[b][ok] = g[bi][ok]
        oi[b][ok] = bi[ok]
    return ob, ol, og, ov, oi


# ---- the eval case table ------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    cap: int
    C: int
    parts: int
    K: int
    n: int
    hs: List[np.ndarray]                 # per stage [cap][C] or [parts][cap][C]
    bias: List[Optional[np.ndarray]]
    heads: List[Tuple]
    boxes: np.ndarray                    # [cap][4]
    reg_ws: Tuple
    img: Tuple[float, float] = (640.0, 640.0)
    score_thresh: float = 0.05
    nms_thresh: float = 0.5
    topk: int = 100
    post: Optional[np.ndarray] = None
    record: str = "none"
    n_on_device: bool = False
    prop: Dict[str, object] = field(default_factory=dict)
    _cache: Dict[str, object] = field(default_factory=dict, repr=False)


def rows_of(case: Case, k: int) -> np.ndarray:
    r = RT.sum_parts(case.hs[k], case.bias[k]) if case.parts >= 1 else case.hs[k]
    return np.ascontiguousarray(r[:case.n])


def expected(case: Case, fault: Optional[str] = None) -> Dict[str, object]:
    key = "exp" if fault is None else "exp-" + fault
    if key not in case._cache:
        out = cascade_eval([rows_of(case, k) for k in range(case.K)], case.heads, case.boxes, case.reg_ws, case.img, case.score_thresh,
                           case.nms_thresh, case.topk, fault)
        if case.post is not None:
            out["fin_boxes"], out["fin_scores"] = RT.postprocess(out["boxes"], out["scores"], case.post)
            if case.record == "rec":
                out["record"] = RT.fill_record(case.cap, out["fin_boxes"], out["fin_scores"], 0xA5)
        case._cache[key] = out
    return case._cache[key]


def _rng(name: str) -> np.random.Generator:
    return np.random.default_rng(zlib.crc32(name.encode()))


def make_case(cap: int, C: int, parts: int, count: str, K: int, nonfinite: bool = False, post=None, record: str = "none",
              n_on_device: bool = False) -> Case:
    name = f"cap{cap}-C{C}-S{parts}-n{count}-K{K}" + ("-nonfinite" if nonfinite else "") + ("-post" if post is not None else "")
    rng = _rng(name)
    n = {"0": 0, "1": 1, "cap": cap}[count]
    hs, bias, heads = [], [], []
    for k in range(K):
        heads.append(RT._head(rng, C))
        if parts >= 1:
            h = (rng.standard_normal((parts, cap, C)) * (1.2 / np.sqrt(parts))).astype(F32)
            h[:, n:] = np.nan                                       # rows at and beyond the count: summed, never used
            bias.append((rng.standard_normal(C) * 0.3).astype(F32) if k % 2 == 0 else None)
        else:
            h = np.abs(rng.standard_normal((cap, C))).astype(F32)
            h[n:] = np.nan
            bias.append(None)
        hs.append(h)
    boxes = RT._pad_rows(RT.clustered(n, rng), cap) if n else np.full((cap, 4), np.nan, F32)
    c = Case(name, cap, C, parts, K, n, hs, bias, heads, boxes, REG_W[:K], post=None if post is None else np.array(post, F32),
             record=record, n_on_device=n_on_device)
    if nonfinite and n > 70:
        # a non-finite delta in an intermediate stage (row 5: +inf in a channel the box head weights) and in the last (row 70: NaN):
        # both rows leave the result, every other row is untouched
        c.hs[0][..., 5, 3] = np.inf
        c.hs[K - 1][..., 70, 3] = np.nan
        c.prop["nonfinite"] = (5, 70)
    return c


CAPS = (1, 63, 64, 65, 320, 512)
WIDTHS = (16, 128, 208)
PARTS = (0, 2, 7)
COUNTS = ("0", "1", "cap")
STAGES = (2, 3)


def _build() -> List[Case]:
    """Every value of every axis, each pair of (cap, C) and of (parts, count), K alternating; the mid shape walks parts x count x K."""
    cs: List[Case] = []
    i = 0
    for cap in CAPS:
        for C in WIDTHS:
            cs.append(make_case(cap, C, PARTS[i % 3], COUNTS[2 - (i // 3) % 3] if cap > 1 else COUNTS[i % 3], STAGES[i % 2], n_on_device=bool(i & 1)))
            i += 1
    for parts in PARTS:
        for count in COUNTS:
            for K in STAGES:
                cs.append(make_case(320, 128, parts, count, K, n_on_device=bool(i & 1)))
                i += 1
    for parts in PARTS:
        cs.append(make_case(320, 128, parts, "cap", 3, nonfinite=True))
        cs.append(make_case(320, 128, parts, "cap", 2 + (parts == 2), post=RT.POSTS["nonuniform"], record="rec", n_on_device=True))
    cs.append(make_case(512, 16, 2, "cap", 2, post=RT.POSTS["down"], record="rec"))
    names = [c.name for c in cs]
    out, seen = [], set()
    for c in cs:
        if c.name not in seen:
            seen.add(c.name)
            out.append(c)
    assert len(names) >= len(out)
    return out


_CASES: Optional[List[Case]] = None


def cases() -> List[Case]:
    global _CASES
    if _CASES is None:
        _CASES = _build()
    return _CASES


def case_names() -> List[str]:
    return [c.name for c in cases()]


def case(name: str) -> Case:
    return next(c for c in cases() if c.name == name)


# ---- the relabel case table ---------------------------------------------------------------------------------------------------------
@dataclass
class RelabelCase:
    name: str
    boxes: np.ndarray
    deltas: np.ndarray
    valid: np.ndarray
    img_hw: np.ndarray
    gtp: np.ndarray
    gt_n: np.ndarray
    reg_w: Tuple
    thr: float
    prop: Dict[str, object] = field(default_factory=dict)


SIZES = ((160.0, 192.0), (97.0, 131.0), (640.0, 480.0))


def relabel_case(B: int, R: int, G: int, k: int = 1) -> RelabelCase:
    """B images of different sizes, R rows: proposals jittered around the image's ground truth (IoUs on both sides of the threshold),
    some far outside the image (they clip to nothing), some padding rows; deltas of stage k - 1's scale."""
    name = f"B{B}-R{R}-G{G}-k{k}"
    rng = _rng(name)
    Gd = max(G, 1)
    boxes, deltas = np.zeros((B, R, 4), F32), np.zeros((B, R, 4), F32)
    valid = np.ones((B, R), bool)
    gtp = np.zeros((B, Gd, 4), F32)
    gt_n = np.zeros(B, np.int64)
    hw = np.array(SIZES[:B], F32)
    reg_w = REG_W[k - 1]
    for b in range(B):
        H, W = hw[b]
        gn = G if b != 1 else max(G - 1, 0)                      # the second image has one ground truth fewer
        gt_n[b] = gn
        wh = rng.uniform(12, 60, (Gd, 2))
        ctr = rng.uniform(0, 1, (Gd, 2)) * (np.array([W, H]) - wh) + wh / 2
        gtp[b] = np.concatenate([ctr - wh / 2, ctr + wh / 2], 1).astype(F32)
        src = gtp[b][rng.integers(0, Gd, R)] + rng.standard_normal((R, 4)).astype(F32) * 4.0
        src[:, 2:] = np.maximum(src[:, 2:], src[:, :2] + 2.0)
        boxes[b] = src
        deltas[b] = (rng.standard_normal((R, 4)) * np.array(reg_w) * 0.05).astype(F32)
        far = rng.random(R) < 0.15
        boxes[b][far] += np.array([W + 300, H + 300, W + 300, H + 300], F32)     # beyond the image: the clip empties them
        valid[b] = rng.random(R) > 0.1
    return RelabelCase(name, boxes, deltas, valid, hw, gtp, gt_n, reg_w, IOUS[k])


def relabel_exact_case(kind: str) -> RelabelCase:
    """Zero deltas and even integer coordinates: the decode returns the box bit for bit, so the IoU is the chosen fraction exactly.
      "at_threshold"  a 10 x 10 box against ground truth [0,0,10,h]: IoU = h/10 (h <= 10) -- 0.5 and 0.75 exactly representable;
      "ties"          two ground-truth boxes mirrored around the row's box: the same IoU, the first index wins (rows 0 and 1);
      "empty"         boxes that the clip leaves with zero width or zero height (on the image's border and beyond it)."""
    if kind == "at_threshold":
        gtp = np.array([[[0, 0, 10, 5], [100, 100, 110, 107.5], [200, 0, 210, 6]]], F32)
        boxes = np.array([[[0, 0, 10, 10], [100, 100, 110, 110], [200, 0, 210, 10], [0, 0, 10, 10]]], F32)
        thr, prop = 0.5, {"ious": (0.5, 0.75, 0.6000000238418579, 0.5)}
        c = RelabelCase("at-threshold-0.5", boxes, np.zeros_like(boxes), np.ones((1, 4), bool), np.array([[400.0, 400.0]], F32), gtp,
                        np.array([3], np.int64), REG_W[0], thr, prop)
        return c
    if kind == "at_threshold_075":
        c = relabel_exact_case("at_threshold")
        return RelabelCase("at-threshold-0.75", c.boxes, c.deltas, c.valid, c.img_hw, c.gtp, c.gt_n, c.reg_w, 0.75, c.prop)
    if kind == "ties":
        gtp = np.array([[[0, 0, 20, 40], [20, 0, 40, 40], [300, 300, 320, 340]]], F32)    # left half, right half, one far away
        boxes = np.array([[[10, 0, 30, 40], [0, 0, 40, 40], [12, 0, 32, 40]]], F32)        # row 2 prefers the right half
        return RelabelCase("ties", boxes, np.zeros_like(boxes), np.ones((1, 3), bool), np.array([[400.0, 400.0]], F32), gtp,
                           np.array([3], np.int64), REG_W[1], 0.3, {"matched": (0, 0, 1)})
    assert kind == "empty"
    boxes = np.array([[[100, 10, 120, 30], [96, 10, 120, 30], [10, 64, 30, 90], [-30, 10, -10, 30], [10, 10, 30, 30], [90, 60, 96, 64]]], F32)
    gtp = np.array([[[8, 8, 32, 32]]], F32)
    return RelabelCase("empty", boxes, np.zeros_like(boxes), np.ones((1, 6), bool), np.array([[64.0, 96.0]], F32), gtp,
                       np.array([1], np.int64), REG_W[0], 0.6, {"valid": (False, False, False, False, True, True)})


def relabel_cases() -> List[RelabelCase]:
    cs = [relabel_case(B, R, G, 1 + (i % 2)) for i, (B, R, G) in enumerate(
        [(B, R, G) for B in (1, 3) for R in (1, 64, 512) for G in (0, 1, 7, 256)])]
    cs += [relabel_exact_case(k) for k in ("at_threshold", "at_threshold_075", "ties", "empty")]
    return cs
