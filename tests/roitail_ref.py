"""The second stage's tail (csrc/ore_roi.hip: k_roi_predict / k_roi_predict_mb<64|8> / k_roi_tail / k_roi_finalize, and the NMS kernels of
csrc/ore_detect.hip behind the general path): its reference and its case table.

The reference is the C twin (oracle/ref_decode.c::oracle_roi_predict, oracle_nms): every comparison of tests/test_hip_roitail.py is
np.array_equal on the bits.  What the twin does not cover is restated here in numpy float32, one IEEE operation per step: the sum of
the K-split partials (`sum_parts`), detector_postprocess (`postprocess`, the arithmetic tests/test_nway_host.py::merge_classes shares)
and the result record (`record_views`).  `emulate` is a numpy model of the tail with seedable faults: tests/test_roitail_host.py
shows that it equals the twin on every case and that every fault changes at least one case, i.e. that the table can see it.
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np

from oracle import decode as odec

REG_W = (10.0, 10.0, 5.0, 5.0)
F32 = np.float32

# ---- the launcher's rule (oreroi::roi_predict_post; tests/test_roitail_host.py reads the constants back from the source) ----------
FUSED_CAP = 512          # ROI_FUSED_CAP
FUSED_C = 210            # C * 4 * 71 + 6 * 64 * 4 <= 60 * 1024 (the engine takes multiples of 16: 208 is the widest head it accepts)
GENERAL_C = 145          # (256 * (C + 1) + 6 * C) * 4 <= 150 * 1024
FUSED64, FUSED8, GENERAL, REFUSED = "FUSED64", "FUSED8", "GENERAL", "REFUSED"


def form(cap: int, C: int, parts: int) -> str:
    """Which kernels a call launches: FUSED64 = k_roi_predict_mb<64> + k_roi_tail, FUSED8 = k_roi_predict_mb<8> + k_roi_tail (the
    engine's form: fc1 rows in K-split partials), GENERAL = k_roi_predict + ore_nms_device_n_fwd + k_roi_finalize."""
    if cap < 1 or C < 1:
        return REFUSED
    if cap <= FUSED_CAP and C <= FUSED_C:
        return FUSED8 if parts >= 1 else FUSED64
    if parts >= 1 or C > GENERAL_C:
        return REFUSED
    return GENERAL


# ---- references ---------------------------------------------------------------------------------------------------------------------
def sum_parts(parts: np.ndarray, bias: Optional[np.ndarray], fault: Optional[str] = None) -> np.ndarray:
    """[S][cap][C] raw sums -> [cap][C] rows: v = bias (or 0), v += parts[z] for z = 0, 1, ..., max(v, 0) with NaN -> 0 (fmaxf)."""
    parts = np.asarray(parts, F32)
    S = parts.shape[0]
    b = np.zeros(parts.shape[-1], F32) if bias is None else np.asarray(bias, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        if fault == "parts_pairwise":
            lvl = [parts[z] for z in range(S)]
            while len(lvl) > 1:
                lvl = [lvl[i] + lvl[i + 1] if i + 1 < len(lvl) else lvl[i] for i in range(0, len(lvl), 2)]
            v = np.broadcast_to(b, parts.shape[1:]) + lvl[0]
        elif fault == "bias_last":
            v = np.zeros(parts.shape[1:], F32)
            for z in range(S):
                v = v + parts[z]
            v = v + b
        else:
            v = np.broadcast_to(b, parts.shape[1:]).astype(F32)
            for z in (range(S - 1, -1, -1) if fault == "parts_reverse" else range(S)):
                v = v + parts[z]
    assert v.dtype == F32
    return np.fmax(v, F32(0))


def predict(h, case, score_thresh=None, nms_thresh=None, topk=None) -> Dict[str, np.ndarray]:
    """The C twin on rows h [n][C] and the case's weights and first n proposals."""
    n = len(h)
    return odec.roi_predict(h, case.cls_w, case.cls_b, case.box_w, case.box_b, case.boxes[:n].reshape(-1, 4) if n else np.zeros((0, 4), F32),
                            REG_W, case.img, case.score_thresh if score_thresh is None else score_thresh,
                            case.nms_thresh if nms_thresh is None else nms_thresh, case.topk if topk is None else topk)


def scale_clip_drop(B: np.ndarray, sx, sy, ow, oh, fault: Optional[str] = None) -> Tuple[np.ndarray, np.ndarray]:
    """detector_postprocess (d2z:modeling/postprocessing.py:10-75) in fp32: scale, clip to the output size, rows whose width or height
    is not > 0 dropped.  Returns (boxes of ALL rows after scale + clip, keep mask)."""
    B = np.array(B, F32).reshape(-1, 4)
    sx, sy, ow, oh = F32(sx), F32(sy), F32(ow), F32(oh)

    def clip(B):
        B[:, 0::2] = np.minimum(np.maximum(B[:, 0::2], F32(0)), ow)
        B[:, 1::2] = np.minimum(np.maximum(B[:, 1::2], F32(0)), oh)
        return B
    if fault == "clip_first":
        B = clip(B) * np.array([sx, sy, sx, sy], F32)
    else:
        B = clip(B * np.array([sx, sy, sx, sy], F32))
    keep = ((B[:, 2] - B[:, 0]) > 0) & ((B[:, 3] - B[:, 1]) > 0)
    return B, keep


def postprocess(boxes, scores, post, fault: Optional[str] = None) -> Tuple[np.ndarray, np.ndarray]:
    """post = {sx, sy, out_w, out_h}; order kept."""
    B, keep = scale_clip_drop(boxes, post[0], post[1], post[2], post[3], fault)
    return B[keep], np.asarray(scores, F32).reshape(-1)[keep]


def record_views(cap: int, fill: int = 0, fault: Optional[str] = None):
    """The caller's result record: boxes [cap][4] f32 at byte 0 | scores [cap] f32 at cap * 16 | classes [cap] i64 at cap * 20."""
    assert cap % 2 == 0, "the int64 classes sit at cap * 20 bytes: even caps only"
    buf = np.full(cap * 28, fill, np.uint8)
    so = cap * 20 if fault == "rec_scores_20" else cap * 16
    return buf, buf[:cap * 16].view(F32).reshape(cap, 4), buf[so:so + cap * 4].view(F32), buf[cap * 20:].view(np.int64)


def fill_record(cap, fin_boxes, fin_scores, fill: int, fault: Optional[str] = None) -> np.ndarray:
    buf, rb, rs, rc = record_views(cap, fill, fault)
    k = len(fin_scores)
    rb[:k] = fin_boxes
    rc[:k] = 0                                        # one foreground class
    rs[:k] = fin_scores
    return buf


# ---- cases --------------------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    classes: Tuple[str, ...]
    cap: int
    C: int
    parts: int
    h: np.ndarray                        # [cap][C], or [parts][cap][C]
    bias: Optional[np.ndarray]
    cls_w: np.ndarray
    cls_b: np.ndarray
    box_w: np.ndarray
    box_b: np.ndarray
    boxes: np.ndarray                    # [cap][4]
    n: int                               # the count handed over (may exceed cap: the kernels clamp)
    n_on_device: bool
    img: Tuple[float, float]             # (h, w)
    score_thresh: float
    nms_thresh: float
    topk: int
    post: Optional[np.ndarray] = None
    record: str = "none"                 # "none": no pin word | "zero": pin with record address 0 | "rec": pin + record
    prop: Dict[str, object] = field(default_factory=dict)
    _cache: Dict[str, object] = field(default_factory=dict, repr=False)

    @property
    def form(self) -> str:
        return form(self.cap, self.C, self.parts)

    @property
    def n_eff(self) -> int:
        return min(max(self.n, 0), self.cap)


def rows_of(case: Case, fault: Optional[str] = None) -> np.ndarray:
    r = sum_parts(case.h, case.bias, fault) if case.parts >= 1 else case.h
    return np.ascontiguousarray(r[:case.n_eff])


def expected(case: Case) -> Dict[str, np.ndarray]:
    """What the launch must leave behind, from the twin: det_* and, with post, fin_* and the record."""
    if "exp" not in case._cache:
        tw = predict(rows_of(case), case)
        out = {"boxes": tw["boxes"], "scores": tw["scores"], "src": tw["src"], "raw_boxes": tw["raw_boxes"], "raw_scores": tw["raw_scores"]}
        if case.post is not None:
            out["fin_boxes"], out["fin_scores"] = postprocess(tw["boxes"], tw["scores"], case.post)
        case._cache["exp"] = out
    return case._cache["exp"]


def finite_rows(case: Case, rows: np.ndarray) -> Tuple[np.ndarray, Dict[str, np.ndarray]]:
    """The twin's per-row verdict "box and score are finite": with the score filter and the NMS switched off (threshold -1 and IoU
    threshold 2) the twin's detections are exactly the finite rows."""
    tw = predict(rows, case, score_thresh=-1.0, nms_thresh=2.0, topk=-1)
    fin = np.zeros(len(rows), bool)
    fin[tw["src"]] = True
    return fin, tw


def sup_matrix(sb: np.ndarray, thr, fault: Optional[str] = None) -> np.ndarray:
    """[i][j]: box i suppresses box j, the twin's fp32 operations."""
    sb = np.asarray(sb, F32)
    thr = F32(thr)
    area = (sb[:, 2] - sb[:, 0]) * (sb[:, 3] - sb[:, 1])
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ww = np.maximum(F32(0), np.minimum(sb[:, None, 2], sb[None, :, 2]) - np.maximum(sb[:, None, 0], sb[None, :, 0]))
        hh = np.maximum(F32(0), np.minimum(sb[:, None, 3], sb[None, :, 3]) - np.maximum(sb[:, None, 1], sb[None, :, 1]))
        inter = ww * hh
        uni = (area[:, None] + area[None, :]) - inter
        assert inter.dtype == F32 and uni.dtype == F32
        if fault == "iou_nodiv":
            return inter > (thr * uni) * F32(1.00000095367431640625)
        ovr = inter / uni
        return ovr >= thr if fault == "iou_ge" else ovr > thr


def band_stats(a: np.ndarray, b: np.ndarray, thr) -> Dict[str, np.ndarray]:
    """Per pair (a[i], b[i]): where k_roi_tail's IoU test lands -- decided without the division (clear) or inside the 2^-20 band, where
    the exact quotient decides."""
    a, b, thr = np.asarray(a, F32), np.asarray(b, F32), F32(thr)
    aa, ab = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]), (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    ww = np.maximum(F32(0), np.minimum(a[:, 2], b[:, 2]) - np.maximum(a[:, 0], b[:, 0]))
    hh = np.maximum(F32(0), np.minimum(a[:, 3], b[:, 3]) - np.maximum(a[:, 1], b[:, 1]))
    inter = ww * hh
    uni = (aa + ab) - inter
    tu = thr * uni
    clear_above = inter > tu * F32(1.00000095367431640625)
    band = ~clear_above & (inter >= tu * F32(0.99999904632568359375))
    above = inter / uni > thr
    return {"clear_above": clear_above, "clear_below": ~clear_above & ~band, "band_above": band & above, "band_below": band & ~above,
            "above": above}


def emulate(case: Case, fault: Optional[str] = None) -> Dict[str, object]:
    """The tail as the kernels run it, in numpy: filter, ordered compaction, stable rank, IoU bits, greedy resolution per 64-row block
    as a fixpoint of at most 64 rounds, stop once topk survivors are known, keep[:topk], postprocess, record.  `fault` seeds one error."""
    rows = rows_of(case, fault)
    fin, tw = finite_rows(case, rows)
    score, st = tw["raw_scores"], F32(case.score_thresh)
    with np.errstate(invalid="ignore"):
        ok = fin & ((score >= st) if fault == "filter_ge" else (score > st))
    comp = np.nonzero(ok)[0]
    cs, cb = score[comp], tw["raw_boxes"][comp]
    m = len(comp)
    idx = np.arange(m)
    order = np.lexsort((-idx if fault == "ties_desc" else idx, -cs.astype(np.float64)))
    sb = cb[order]
    S = sup_matrix(sb, case.nms_thresh, fault) & (idx[:, None] < idx[None, :])
    kept = np.zeros(m, bool)
    nk, walked, rounds = 0, 0, 0
    for lo in range(0, m, 64):
        hi = min(m, lo + 64)
        walked += 1
        cand = ~(S[:lo, lo:hi] & kept[:lo, None]).any(0)
        D = S[lo:hi, lo:hi]
        if fault == "early_unresolved" and case.topk >= 0 and nk + int(cand.sum()) >= case.topk:
            k = cand                                   # stops on the candidates' count: the block's own suppressions are not applied
        else:
            k = cand.copy()
            for it in range(8 if fault == "fix8" else 64):
                kn = cand & ~(D & k[:, None]).any(0)
                if np.array_equal(kn, k):
                    break
                k = kn
                rounds = max(rounds, it + 1)
        kept[lo:hi] = k
        nk += int(k.sum())
        if case.topk >= 0 and nk >= case.topk:
            break
    rows_k = np.nonzero(kept)[0]
    if case.topk >= 0:
        rows_k = rows_k[:case.topk]
    out = {"boxes": sb[rows_k], "scores": cs[order][rows_k], "src": comp[order][rows_k].astype(np.int64), "m": m, "walked": walked,
           "rounds": rounds, "blocks": (m + 63) // 64}
    if case.post is not None:
        out["fin_boxes"], out["fin_scores"] = postprocess(out["boxes"], out["scores"], case.post, fault)
        if case.record == "rec":
            out["record"] = fill_record(case.cap, out["fin_boxes"], out["fin_scores"], 0xA5, fault)
    return out


def same(a: Dict[str, object], b: Dict[str, object]) -> bool:
    """Bitwise equality of two results on the keys both hold."""
    for k in ("boxes", "scores", "src", "fin_boxes", "fin_scores", "record"):
        if k in a and k in b:
            x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
            if x.shape != y.shape or x.dtype != y.dtype or x.tobytes() != y.tobytes():
                return False
    return True


# ---- input builders -----------------------------------------------------------------------------------------------------------------
def _rng(name: str) -> np.random.Generator:
    return np.random.default_rng(zlib.crc32(name.encode()))


def clustered(n: int, rng) -> np.ndarray:
    """Clustered proposals as in test_column_scan_vs_oracle_every_ring_position: a centre per ~12 boxes, 3 px jitter, 25-45 px sides;
    most rows are suppressed by an earlier survivor, which as a rule sits in another 64-row block."""
    centres = rng.random((max(n // 12, 1), 2)) * 560 + 40
    ctr = centres[rng.integers(0, len(centres), n)] + rng.standard_normal((n, 2)) * 3.0
    wh = np.exp(rng.random((n, 2)) * 0.6 + 3.2)
    return np.concatenate([ctr - wh / 2, ctr + wh / 2], 1).astype(F32)


def _head(rng, C: int):
    """A random predictor head with logits and deltas of order one at any width."""
    s = 1.0 / np.sqrt(C)
    return ((rng.standard_normal((2, C)) * 1.5 * s).astype(F32), (rng.standard_normal(2) * 0.1).astype(F32),
            (rng.standard_normal((4, C)) * 0.5 * s).astype(F32), (rng.standard_normal(4) * 0.05).astype(F32))


def _exact_head(C: int):
    """score = softmax(h[0], 0)[0], boxes pass through: zero box head, so dx = dy = dw = dh = 0, exp(0) = 1 and a box with even integer
    coordinates below 2^24 comes back bit for bit (cx = x0 + w / 2 and cx -+ w / 2 are exact)."""
    cls_w = np.zeros((2, C), F32)
    cls_w[0, 0] = 1.0
    return cls_w, np.zeros(2, F32), np.zeros((4, C), F32), np.zeros(4, F32)


def _desc_logits(n: int) -> np.ndarray:
    """Strictly descending, non-negative, exact in fp32: row order = score order."""
    assert n <= 1024
    return (F32(4.0) - np.arange(n, dtype=F32) * F32(1.0 / 256)).astype(F32)


def _far(n: int, first: int = 0) -> np.ndarray:
    """n boxes that overlap nothing (even integers; 20 x 20 on a diagonal far from everything else)."""
    o = (F32(1 << 20) + (np.arange(n, dtype=F32) + first) * 64).astype(F32)
    return np.stack([o, o, o + 20, o + 20], 1).astype(F32)


def chain(L: int, start: int, tail: int = 6):
    """L boxes 100 x 100 stepped by 4 px: neighbours overlap 96 / 104 = 0.923 > 0.9, second neighbours 92 / 108 = 0.852 < 0.9; scores
    strictly descending along the chain, which sits at sorted rows start .. start + L - 1 between boxes that overlap nothing.  Greedy
    keeps every other link, and the block fixpoint fixes one more link per round: L = 64 at start 0 needs 63 rounds."""
    x = np.arange(L, dtype=F32) * 4
    ch = np.stack([x, np.zeros(L, F32), x + 100, np.full(L, 100, F32)], 1)
    boxes = np.concatenate([_far(start), ch, _far(tail, start)]).astype(F32)
    return boxes, _desc_logits(len(boxes)), {"chain": (start, L), "nms_thresh": 0.9}


THR_FRACTION = {0.9: (9, 10), 0.6: (3, 5), 0.5: (1, 2), 0.7: (7, 10), 0.3: (3, 10)}
NEAR_K = (1, 3, 1000, 1 << 16, 1 << 18, 1 << 19, 1 << 20, 1500000)


def near_threshold(thr: float, scale: int = 1):
    """Pairs of nested integer boxes [0, y, q k, y + H] and [0, y, p k + d, y + H] with p / q the threshold's fraction: IoU = p / q +
    d / (q k) sits on, just above and just below the threshold, at magnitudes where inter and union carry 1 to 24 significant bits.
    Pair i lives at y = 512 i, so different pairs never overlap.  scale = 2 doubles x (an exact operation on every product and sum of
    the IoU, so each decision is the one of the undoubled pair) and makes every coordinate even: the form that survives the predictor.
    Pairs whose width passes 2^24 are skipped.  Returns (a [P][4], b [P][4])."""
    p, q = THR_FRACTION[thr]
    a, b = [], []
    for k in NEAR_K:
        if scale * q * k > (1 << 24):
            continue
        for d in (-2, -1, 0, 1, 2):
            if p * k + d <= 0:
                continue
            for H in (2, 6, 250):
                y = 512.0 * len(a)
                a.append([0.0, y, scale * q * k, y + H])
                b.append([0.0, y, scale * (p * k + d), y + H])
    return np.array(a, F32), np.array(b, F32)


def near_rows(thr: float, scale: int):
    """The family as a box list: pair i at rows 2 i (the outer box, ranked first) and 2 i + 1."""
    a, b = near_threshold(thr, scale)
    boxes = np.stack([a, b], 1).reshape(-1, 4)
    return boxes, _desc_logits(len(boxes)), {"near": thr, "nms_thresh": thr}


def cancelling_parts(S: int, cap: int, C: int, rng) -> np.ndarray:
    """Partials of magnitude 1e4 with alternating sign and a small residual: every partial sum rounds at 1e-3, so the order of the
    additions (and where the bias enters) changes the bits of the row."""
    base = rng.uniform(0.5e4, 1.5e4, ((S + 1) // 2, cap, C))
    p = np.empty((S, cap, C), np.float64)
    p[0::2] = base[:(S + 1) // 2]
    p[1::2] = -base[:S // 2]
    if S % 2:
        p[-1] = 0.0
    return (p + rng.uniform(-0.05, 0.25, (S, cap, C))).astype(F32)


def _pad_rows(a: np.ndarray, cap: int, fill=np.nan) -> np.ndarray:
    out = np.full((cap,) + a.shape[1:], fill, F32)
    out[:min(len(a), cap)] = a[:cap]
    return out


def _to_parts(rows_cap: np.ndarray, S: int, n_eff: int) -> np.ndarray:
    """Rows as S partials whose ordered sum is exact: slice S // 2 carries the row, the others 0; rows at and beyond the count NaN."""
    p = np.zeros((S,) + rows_cap.shape, F32)
    p[S // 2] = rows_cap
    p[:, n_eff:] = np.nan
    return p


def _thresh_for(case: Case, m: int) -> float:
    """A score threshold that exactly m rows pass (strict >): the (m + 1)-th largest finite score of the twin's rows."""
    rows = rows_of(case)
    fin, tw = finite_rows(case, rows)
    s = np.sort(tw["raw_scores"][fin])[::-1]
    if m >= len(s):
        assert m == len(s) and s[-1] > 0
        return 0.0
    assert m == 0 or s[m - 1] > s[m], "scores tie at the cut"
    return float(s[m])


def random_case(name: str, classes, cap: int, C: int, S: int = 0, bias: bool = False, n: Optional[int] = None, on_dev: bool = False,
                m: Optional[int] = None, topk: int = 100, thr: float = 0.5, post=None, record: str = "none", cancelling: bool = False,
                ties: bool = False, score_thresh: float = 0.05) -> Case:
    rng = _rng(name)
    n = cap if n is None else n
    n_eff = min(max(n, 0), cap)
    cls_w, cls_b, box_w, box_b = _head(rng, C)
    boxes = _pad_rows(clustered(n_eff, rng), cap) if n_eff else np.full((cap, 4), np.nan, F32)
    b = (rng.standard_normal(C) * 0.3).astype(F32) if bias else None
    if S >= 1:
        h = cancelling_parts(S, cap, C, rng) if cancelling else (rng.standard_normal((S, cap, C)) * (1.2 / np.sqrt(S))).astype(F32)
        if ties:
            h[:, 1::3] = h[:, 0:-1:3][:, :len(h[0, 1::3])]
        h[:, n_eff:] = np.nan
    else:
        h = np.abs(rng.standard_normal((cap, C))).astype(F32)
        if ties:
            h[1::3] = h[0:-1:3][:len(h[1::3])]
        h[n_eff:] = np.nan
    c = Case(name, tuple(classes), cap, C, S, h, b, cls_w, cls_b, box_w, box_b, boxes, n, on_dev, (640.0, 640.0), score_thresh, thr, topk,
             None if post is None else np.array(post, F32), record)
    if m is not None:
        c.score_thresh = _thresh_for(c, m)
        c.prop["m"] = m
    return c


def exact_case(name: str, classes, frm: str, boxes: np.ndarray, logits: np.ndarray, prop: dict, C: int = 16, topk: int = -1,
               score_thresh: float = 0.0, S: int = 17) -> Case:
    """Boxes that pass the predictor unchanged (zero box head), scored by their logits, in the launch form `frm`."""
    n = len(boxes)
    cap = {FUSED64: max(n + (n & 1), 2), FUSED8: max(n + (n & 1), 2), GENERAL: max(n + 3, 513)}[frm]
    assert cap <= 1024
    rows = np.zeros((n, C), F32)
    rows[:, 0] = logits
    rows = _pad_rows(rows, cap)
    parts = S if frm == FUSED8 else 0
    h = _to_parts(rows, S, n) if parts else rows
    cls_w, cls_b, box_w, box_b = _exact_head(C)
    c = Case(name, tuple(classes), cap, C, parts, h, None, cls_w, cls_b, box_w, box_b, _pad_rows(boxes, cap), n, False,
             (float(1 << 24), float(1 << 24)), score_thresh, float(prop["nms_thresh"]), topk, None, "none", dict(prop))
    assert c.form == frm, (name, c.form, frm)
    return c


# ---- the case table -----------------------------------------------------------------------------------------------------------------
THRESHOLDS = (0.3, 0.5, 0.6, 0.7, 0.9)
TOPKS = (-1, 0, 1, 63, 64, 65, 100, 1000)
PARTS = (2, 15, 16, 17, 32, 33)
POSTS = {"identity": (1.0, 1.0, 640.0, 640.0), "up": (2.5, 2.5, 1600.0, 1600.0), "down": (0.3, 0.3, 192.0, 192.0),
         "nonuniform": (1.7, 0.45, 1088.0, 288.0),
         # scaled by 0.004 a 30 px box is 0.12 px wide and the image 2.56 px; the 1.9 px output clips the boxes beyond it to nothing,
         # interleaved with the rest
         "emptying": (0.004, 0.004, 1.9, 1.9)}
# the three cap / width pairs at which the axes common to all forms are walked
MID = {FUSED64: dict(cap=320, C=128), FUSED8: dict(cap=320, C=128, S=32, bias=True), GENERAL: dict(cap=600, C=128)}


def _build() -> List[Case]:
    cs: List[Case] = []
    add = cs.append
    # -- the shape axes of every form
    i = 0
    for cap in (1, 2, 63, 64, 65, 320, 511, 512):
        for C in (1, 16, 128, 208):
            add(random_case(f"f64-cap{cap}-C{C}", ("shape",), cap, C, thr=THRESHOLDS[i % 5], topk=TOPKS[i % 8], on_dev=bool(i & 1)))
            i += 1
    for C in (209, 210):                  # the launcher's own bound (the engine stops at 208, a multiple of 16)
        add(random_case(f"f64-cap64-C{C}", ("shape",), 64, C))
    for cap in (1, 7, 8, 9, 320, 510):
        for C in (16, 128, 208):
            add(random_case(f"f8-cap{cap}-C{C}-S{PARTS[i % 6]}", ("shape",), cap, C, S=PARTS[i % 6], bias=bool(i & 1), thr=THRESHOLDS[i % 5],
                            topk=TOPKS[i % 8], on_dev=bool(i & 2)))
            i += 1
    for S in PARTS:
        for bias in (False, True):
            add(random_case(f"f8-cap9-C128-S{S}-b{int(bias)}", ("parts",), 9, 128, S=S, bias=bias, n=7, on_dev=bias))
            add(random_case(f"f8-cancel-S{S}-b{int(bias)}", ("cancelling",), 40, 16, S=S, bias=bias, cancelling=True))
    for cap in (513, 600, 1024):
        for j, C in enumerate((1, 128, 145)):
            add(random_case(f"gen-cap{cap}-C{C}", ("shape",), cap, C, n=(255, 256, 257, 513)[i % 4], thr=THRESHOLDS[i % 5], topk=TOPKS[i % 8],
                            on_dev=bool(i & 1)))
            i += 1
    for n in (255, 256, 257, 513):
        add(random_case(f"gen-cap600-n{n}", ("pass",), 600, 16, n=n))
    add(random_case("gen-cap1024-full", ("pass",), 1024, 16, n=1024, thr=0.6))
    # -- the axes common to all forms
    for frm, kw in MID.items():
        cap = kw["cap"]
        for on_dev in (False, True):
            for tag, n in (("below", cap - 37), ("equal", cap), ("above", cap + 3), ("zero", 0)):
                add(random_case(f"{frm}-count-{'dev' if on_dev else 'host'}-{tag}", ("count",), n=n, on_dev=on_dev, **kw))
        for m in (0, 1, 64, 65, 200):
            add(random_case(f"{frm}-m{m}", ("filter",), m=m, thr=0.9, topk=-1, **kw))
        for topk in TOPKS:
            add(random_case(f"{frm}-topk{topk}", ("topk",), topk=topk, thr=0.7, m=250, **kw))
        add(random_case(f"{frm}-earlystop", ("earlystop",), m=200, topk=16, thr=0.6, **kw))
        for thr in THRESHOLDS:
            add(random_case(f"{frm}-thr{thr}", ("threshold",), thr=thr, topk=-1, **kw))
            add(exact_case(f"{frm}-near{thr}", ("near",), frm, *near_rows(thr, 2)))
        add(random_case(f"{frm}-ties", ("ties",), ties=True, thr=0.6, topk=-1, **kw))
        add(exact_case(f"{frm}-chain64-at0", ("chain",), frm, *chain(64, 0)))
        add(exact_case(f"{frm}-chain64-at32", ("chain",), frm, *chain(64, 32)))
        add(exact_case(f"{frm}-chain40-at100", ("chain",), frm, *chain(40, 100)))
        # rows whose two logits are equal score exactly 0.5: the strict filter rejects them at score_thresh = 0.5
        lg = _desc_logits(90)
        lg[2::3] = 0.0
        c = exact_case(f"{frm}-on-threshold", ("on_threshold",), frm, _far(90), lg, {"nms_thresh": 0.5, "on_threshold": 30}, score_thresh=0.5)
        add(c)
        # one row with +inf and one with NaN in a channel the box head weights, between valid rows
        c = random_case(f"{frm}-nonfinite", ("nonfinite",), thr=0.9, topk=-1, **kw)
        for r, v in ((5, np.inf), (70, np.nan)):
            c.h[..., r, 3] = v
        c.prop["nonfinite"] = (5, 70)
        add(c)
    # -- postprocess and record (the fused forms)
    for frm in (FUSED64, FUSED8):
        kw = MID[frm]
        for j, (pname, post) in enumerate(POSTS.items()):
            for record in ("none", "zero", "rec"):
                add(random_case(f"{frm}-post-{pname}-{record}", ("post", "record-" + record), post=post, record=record, thr=0.7,
                                topk=(100, -1, 64)[j % 3], **kw))
        add(random_case(f"{frm}-post-empty-list", ("post",), post=POSTS["up"], record="rec", m=0, **kw))
        add(random_case(f"{frm}-post-cap2", ("post",), 2, 16, S=kw.get("S", 0), post=POSTS["up"], record="rec"))
        add(random_case(f"{frm}-post-cap512", ("post",), 512, 16, S=2 if frm == FUSED8 else 0, post=POSTS["down"], record="rec", thr=0.9, topk=-1))
    names = [c.name for c in cs]
    assert len(set(names)) == len(names)
    return cs


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


FAULTS = ("filter_ge", "iou_ge", "iou_nodiv", "ties_desc", "fix8", "early_unresolved", "parts_reverse", "parts_pairwise", "bias_last",
          "clip_first", "rec_scores_20")

# refusals: (name, cap, C, parts, post, outputs given, workspace given); every one returns before any launch
REFUSALS = (("C211-cap64", 64, 211, 0, False, True, True), ("C146-cap513", 513, 146, 0, False, True, True),
            ("parts-cap513", 513, 16, 2, False, True, True), ("post-cap513", 513, 16, 0, True, True, True),
            ("post-without-outputs", 64, 16, 0, True, False, True), ("small-workspace", 64, 16, 0, False, True, False),
            ("parts-C211", 64, 211, 2, False, True, True))


# ---- NMS inputs (ore_nms_fwd / ore_nms_device_n_fwd) ---------------------------------------------------------------------------------
def nms_inputs(n: int, seed: int):
    """Clustered boxes with score ties (every fifth score repeats its neighbour's)."""
    rng = np.random.default_rng(seed)
    boxes = clustered(n, rng)
    scores = (rng.random(n) * 0.98 + 0.01).astype(F32)
    scores[0:n - 1:5] = scores[1::5][:len(scores[0:n - 1:5])]
    return boxes, scores


def near_nms_inputs(thr: float, n: int):
    """The near-threshold family (odd coordinates included: no predictor in front) padded to n rows with boxes that overlap nothing."""
    a, b = near_threshold(thr, 1)
    fam = np.stack([a, b], 1).reshape(-1, 4)
    assert len(fam) <= n
    pad = n - len(fam)
    o = (F32(1 << 20) + np.arange(pad, dtype=F32) * 64).astype(F32)
    far = np.stack([o, F32(1 << 22) + np.zeros(pad, F32), o + 20, F32(1 << 22) + 20 + np.zeros(pad, F32)], 1).astype(F32)
    boxes = np.concatenate([fam, far]).astype(F32)
    scores = np.linspace(0.99, 0.01, n).astype(F32)
    return boxes, scores
