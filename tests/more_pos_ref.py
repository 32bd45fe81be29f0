"""float64 restatement of MORE_POS (csrc/ore_more_pos.hip; ref:fewx/modeling/fsod/fsod_rpn.py:1213-1343) over the
running-error number X = (v, m, d) of tests/trainloss_ref.py, and the margin every fixture's seed has to keep.

The rule, per object n of image b with box (x1, y1, x2, y2), level l (stride s, map H x W) and neighbour k = 0..8
(dx = k % 3 - 1, dy = k // 3 - 1):
    centre cell   cx = trunc(((x1 + x2) / 2) / s), cy likewise                  (fp32, k_cn_pos_inds' expression)
    centre reg    (gx - x1, gy - y1, x2 - gx, y2 - gy) / s,  gx = cx s + s // 2
    candidate     row = row0[l] + b H W + (cy + dy) W + (cx + dx);  target = centre reg shifted by (dx, dy): l + dx, r - dx, t + dy, b - dy
    valid         the neighbour is inside the map and every side of the target is >= 0
    level mask    every side of the centre reg >= 0 and SOI_lo[l] <= sqrt(w^2 + h^2) / 2 <= SOI_hi[l]
    loss          GIoU loss (fewx/layers/iou_loss.py, 'giou') of head[row, :4] against the target; 1e8 where invalid; 0 at k = 4 of a
                  level whose mask holds AND whose centre cell is inside the map (the one departure from the reference, which indexes
                  out of range there)
    threshold     min(TOPK-th smallest of the object's 9 L losses -- NaN above every number --, THRESH)
    kept          loss < threshold, strictly; the list is the kept rows in (image, object, level, k) order, duplicates kept.

Exactness.  Boxes of the fixtures lie on the 1/8 px grid and strides are powers of two, so the centre cell, the centre regression, the
shifted targets, validity and `min(reg) >= 0` are exact in fp32 and in float64 alike; the size-of-interest comparison keeps the margin
CN_MARGIN of tests/trainloss_ref.py.  What is NOT exact is a loss against its threshold: both are rounded fp32 expressions.  The seed
condition: outside the zero-width case no candidate may have |loss - threshold| within the SUM of the two first-order bounds
2 d u m (candidate and threshold; the fp32 constant THRESH is exact and has bound 0), and the TOPK-th loss keeps the same distance from
THRESH.  With it fp32 torch, this restatement and the kernel select the same candidates: the tests compare the lists exactly.

Test infrastructure (used by tests/ and tools/gen_more_pos_golden.py only)."""
import numpy as np

import trainloss_ref as TL
from trainloss_ref import F32, F64, X, xmax, xmin

INF = 100000000.0
DX = np.array([-1, 0, 1, -1, 0, 1, -1, 0, 1])
DY = np.array([-1, -1, -1, 0, 0, 0, 1, 1, 1])
CASES = ("a", "b", "c", "d", "e", "f", "g1", "g27", "h", "i", "i27", "j")   # tests/golden/cn_more_pos_<case>.npz (tools/gen_more_pos_golden.py)
NO_MARGIN = ("i", "i27")                                 # the zero-width box: NaN losses, the list is whatever the reference returned


def candidates(gt, counts, shapes, strides, soi):
    """The geometry of every candidate of every object, in (image, object) order: dict of
    rows [N, L, 9] int64 (-1 outside the map), target [N, L, 9, 4] float32 (exact), valid [N, L, 9], level_mask [N, L],
    centre_in [N, L], soi_margin (smallest relative distance of a size criterion from a limit it is compared with)."""
    gt = np.asarray(gt, dtype=F32)
    B, L = gt.shape[0], len(strides)
    boxes, img = [], []
    for b in range(B):
        n = int(counts[b])
        boxes.append(gt[b, :n]); img += [b] * n
    bx = np.concatenate(boxes, 0).reshape(-1, 4) if boxes else np.zeros((0, 4), F32)
    img = np.asarray(img, dtype=np.int64)
    N = bx.shape[0]
    rows = np.full((N, L, 9), -1, dtype=np.int64)
    target = np.zeros((N, L, 9, 4), dtype=F32)
    valid = np.zeros((N, L, 9), dtype=bool)
    level_mask = np.zeros((N, L), dtype=bool)
    centre_in = np.zeros((N, L), dtype=bool)
    x1, y1, x2, y2 = (bx[:, i] for i in range(4))
    w, h = (x2 - x1).astype(F64), (y2 - y1).astype(F64)
    crit = np.sqrt(w * w + h * h) / 2.0
    soi_margin, row0 = np.inf, 0
    for l, (s, (H, W)) in enumerate(zip(strides, shapes)):
        fs = F32(s)
        with np.errstate(invalid="ignore"):
            cx = np.trunc(((x1 + x2) / F32(2)) / fs).astype(np.int64)
            cy = np.trunc(((y1 + y2) / F32(2)) / fs).astype(np.int64)
        gx, gy = cx.astype(F32) * fs + F32(s // 2), cy.astype(F32) * fs + F32(s // 2)
        reg = np.stack([(gx - x1) / fs, (gy - y1) / fs, (x2 - gx) / fs, (y2 - gy) / fs], 1)          # [N, 4] fp32
        lo, hi = F64(F32(soi[l][0])), F64(F32(soi[l][1]))
        for lim in (lo, hi):
            if N and lim > 0:
                d = np.abs(crit / lim - 1.0)
                soi_margin = min(soi_margin, float(d[d > 0].min()) if (d > 0).any() else np.inf)
        with np.errstate(invalid="ignore"):
            level_mask[:, l] = (reg >= 0).all(1) & (crit >= lo) & (crit <= hi)
        centre_in[:, l] = (cx >= 0) & (cx < W) & (cy >= 0) & (cy < H)
        nx, ny = cx[:, None] + DX[None], cy[:, None] + DY[None]
        inside = (nx >= 0) & (nx < W) & (ny >= 0) & (ny < H)
        rows[:, l] = np.where(inside, row0 + img[:, None] * (H * W) + ny * W + nx, -1)
        t = np.repeat(reg[:, None, :], 9, 1)
        t[:, :, 0] += DX.astype(F32); t[:, :, 2] -= DX.astype(F32)
        t[:, :, 1] += DY.astype(F32); t[:, :, 3] -= DY.astype(F32)
        target[:, l] = t
        with np.errstate(invalid="ignore"):
            valid[:, l] = inside & (t >= 0).all(2)
        row0 += B * H * W
    return dict(rows=rows, target=target, valid=valid, level_mask=level_mask, centre_in=centre_in, soi_margin=soi_margin, image=img,
                total_rows=row0)


def giou_loss(P, T):
    """1 - giou of k_cn_loss_partial / iou_loss.py for X-able arrays P, T [..., 4] (ltrb), operation for operation."""
    pl, pt, pr, pb = (X(P[..., k]) for k in range(4))
    tl, tt, tr, tb = (X(T[..., k]) for k in range(4))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ta, pa = (tl + tr) * (tt + tb), (pl + pr) * (pt + pb)
        wi, hi = xmin(pl, tl) + xmin(pr, tr), xmin(pb, tb) + xmin(pt, tt)
        gw, gh = xmax(pl, tl) + xmax(pr, tr), xmax(pb, tb) + xmax(pt, tt)
        ac, ai = gw * gh, wi * hi
        au = ta + pa - ai
        iou = (ai + 1.0) / (au + 1.0)
        return 1.0 - (iou - (ac - au) / ac)


def more_pos_ref(gt, counts, head, shapes, strides, soi, thresh=0.2, topk=9):
    """-> dict(pos_inds int64 [P] in (image, object, level, k) order, loss X [N, L * 9], thresh_eff [N], kth [N] (value, bound),
    worst: the largest  (bound_loss + bound_threshold) / |loss - threshold|  over every candidate that is not exact and is not the
    TOPK-th element itself, and of the TOPK-th loss against THRESH -- the seed condition is worst < 1 --, near: how many are >= 1)."""
    c = candidates(gt, counts, shapes, strides, soi)
    N, L = c["valid"].shape[:2]
    hd = np.asarray(head, dtype=F32)[:, :4]
    P = hd[np.where(c["valid"], c["rows"], 0)].astype(F64)                                            # [N, L, 9, 4]
    loss = giou_loss(P, c["target"].astype(F64))
    real = c["level_mask"][:, :, None] & c["centre_in"][:, :, None] & (np.arange(9) == 4)[None, None, :]
    exact = ~c["valid"] | real
    v = np.where(real, 0.0, np.where(c["valid"], loss.v, INF)).reshape(N, L * 9)
    m = np.where(exact, 0.0, loss.m).reshape(N, L * 9)
    bound = 2.0 * loss.d * TL.U * m                                                                  # 0 for the exact entries
    order = np.argsort(v, axis=1, kind="stable")                                                     # NaN last, like torch.kthvalue
    ki = order[:, topk - 1] if N else np.zeros(0, dtype=np.int64)
    ar = np.arange(N)
    kth, kth_b = v[ar, ki], bound[ar, ki]
    t32 = F64(F32(thresh))
    clamp = kth > t32                                                                                 # False for a NaN: it stays
    th = np.where(clamp, t32, kth)
    th_b = np.where(clamp, 0.0, kth_b)
    with np.errstate(invalid="ignore"):
        sel = v < th[:, None]
        diff = np.abs(v - th[:, None])
        tot = bound + th_b[:, None]
        own = np.zeros_like(sel); own[ar, ki] = ~clamp
        ratio = np.where(own | (tot == 0) | np.isnan(diff), 0.0, tot / np.maximum(diff, 1e-300))
        kr = np.where((kth_b == 0) | np.isnan(kth), 0.0, kth_b / np.maximum(np.abs(kth - t32), 1e-300))
    worst = max(float(ratio.max()) if ratio.size else 0.0, float(kr.max()) if kr.size else 0.0)
    near = int((ratio >= 1).sum() + (kr >= 1).sum())
    pos = c["rows"].reshape(N, L * 9)[sel]
    return dict(pos_inds=pos.astype(np.int64), sel=sel, loss=X(v, m, loss.d), thresh_eff=th, kth=(kth, kth_b), worst=worst, near=near,
                soi_margin=c["soi_margin"], cand=c)


def load_case(path):
    """A fixture as a dict of numpy arrays and Python scalars / tuples."""
    z = np.load(path)
    d = {k: z[k] for k in z.files}
    d["shapes"] = [tuple(int(x) for x in r) for r in d["shapes"]]
    d["strides"] = tuple(int(x) for x in d["strides"])
    d["soi"] = tuple((float(a), float(b)) for a, b in d["soi"])
    d["thresh"], d["topk"], d["seed"] = float(d["thresh"]), int(d["topk"]), int(d["seed"])
    return d
