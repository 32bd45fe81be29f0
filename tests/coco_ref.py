"""CPU reference for COCO box AP: pycocotools' COCOeval (iouType "bbox", useCats 1) restated in numpy from its published definition
(COCO.loadRes, COCOeval._prepare / computeIoU / evaluateImg / accumulate, maskApi.c bbIou).  Neither pycocotools nor detectron2's
COCOeval_opt is available here, so this restatement is the reference the device kernels (csrc/ore_coco_eval.hip) are pinned to bit
for bit.  Like NMS and ROIAlign it is parity *unpinned* by the reference project: nothing here was run against pycocotools itself.

The loops follow the published code line by line on purpose (no vectorised shortcut of the greedy match), so that this file can be
read next to it."""
import numpy as np

IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
AREA_LBL = ["all", "small", "medium", "large"]
MAX_DETS = [1, 10, 100]


def bb_iou(d, g, iscrowd):
    """maskApi.c bbIou: d [m][4], g [n][4] XYWH doubles -> [m][n]."""
    m, n = len(d), len(g)
    o = np.zeros((m, n))
    for j in range(n):
        G = g[j]
        ga = G[2] * G[3]
        crowd = bool(iscrowd[j])
        for i in range(m):
            D = d[i]
            da = D[2] * D[3]
            w = min(D[2] + D[0], G[2] + G[0]) - max(D[0], G[0])
            if w <= 0:
                continue
            h = min(D[3] + D[1], G[3] + G[1]) - max(D[1], G[1])
            if h <= 0:
                continue
            i_ = w * h
            u = da if crowd else da + ga - i_
            o[i, j] = i_ / u
    return o


def load_res(results):
    """COCO.loadRes for bbox results: area = w * h, id = row + 1, iscrowd = 0."""
    anns = []
    for i, r in enumerate(results):
        bb = r["bbox"]
        anns.append({"image_id": r["image_id"], "category_id": r["category_id"], "bbox": list(bb), "score": r["score"],
                     "area": bb[2] * bb[3], "id": i + 1, "iscrowd": 0})
    return anns


def evaluate(gt_json, results, iou_thrs=IOU_THRS, rec_thrs=REC_THRS, area_rng=AREA_RNG, max_dets=MAX_DETS):
    """-> dict(precision [T,R,K,A,M], recall [T,K,A,M], scores [T,R,K,A,M], eval_imgs {(k, a, i): evaluateImg dict or None},
    img_ids, cat_ids)."""
    img_ids = sorted(im["id"] for im in gt_json["images"])
    cat_ids = sorted(c["id"] for c in gt_json["categories"])
    img_set, cat_set = set(img_ids), set(cat_ids)
    assert set(r["image_id"] for r in results) <= img_set, "Results do not correspond to current coco set"
    gts, dts = {}, {}
    # _prepare: getAnnIds(imgIds, catIds) walks imgToAnns image by image, json order inside an image
    by_img = {}
    for a in gt_json["annotations"]:
        by_img.setdefault(a["image_id"], []).append(a)
    for im in img_ids:
        for a in by_img.get(im, []):
            if a["category_id"] in cat_set:
                g = dict(a)
                g["iscrowd"] = int(g.get("iscrowd", 0))
                g["ignore"] = g["iscrowd"]
                gts.setdefault((im, a["category_id"]), []).append(g)
    res = load_res(results)
    res_by_img = {}
    for d in res:
        res_by_img.setdefault(d["image_id"], []).append(d)
    for im in img_ids:
        for d in res_by_img.get(im, []):
            if d["category_id"] in cat_set:
                dts.setdefault((im, d["category_id"]), []).append(d)

    maxDet = max_dets[-1]

    def compute_iou(imgId, catId):
        gt, dt = gts.get((imgId, catId), []), dts.get((imgId, catId), [])
        if len(gt) == 0 and len(dt) == 0:
            return []
        inds = np.argsort([-d["score"] for d in dt], kind="mergesort")
        dt = [dt[i] for i in inds]
        if len(dt) > maxDet:
            dt = dt[0:maxDet]
        if len(gt) == 0 or len(dt) == 0:
            return []
        return bb_iou([d["bbox"] for d in dt], [g["bbox"] for g in gt], [int(o["iscrowd"]) for o in gt])

    ious = {(i, c): compute_iou(i, c) for i in img_ids for c in cat_ids}

    def evaluate_img(imgId, catId, aRng):
        gt, dt = gts.get((imgId, catId), []), dts.get((imgId, catId), [])
        if len(gt) == 0 and len(dt) == 0:
            return None
        for g in gt:
            g["_ignore"] = 1 if (g["ignore"] or (g["area"] < aRng[0] or g["area"] > aRng[1])) else 0
        gtind = np.argsort([g["_ignore"] for g in gt], kind="mergesort")
        gt = [gt[i] for i in gtind]
        dtind = np.argsort([-d["score"] for d in dt], kind="mergesort")
        dt = [dt[i] for i in dtind[0:maxDet]]
        iscrowd = [int(o["iscrowd"]) for o in gt]
        io = ious[imgId, catId]
        io = io[:, gtind] if len(io) > 0 else io
        T, G, D = len(iou_thrs), len(gt), len(dt)
        gtm = np.zeros((T, G))
        dtm = np.zeros((T, D))
        gtIg = np.array([g["_ignore"] for g in gt])
        dtIg = np.zeros((T, D))
        if not len(io) == 0:
            for tind, t in enumerate(iou_thrs):
                for dind, d in enumerate(dt):
                    iou = min([t, 1 - 1e-10])
                    m = -1
                    for gind, g in enumerate(gt):
                        if gtm[tind, gind] > 0 and not iscrowd[gind]:
                            continue
                        if m > -1 and gtIg[m] == 0 and gtIg[gind] == 1:
                            break
                        if io[dind, gind] < iou:
                            continue
                        iou = io[dind, gind]
                        m = gind
                    if m == -1:
                        continue
                    dtIg[tind, dind] = gtIg[m]
                    dtm[tind, dind] = gt[m]["id"]
                    gtm[tind, m] = d["id"]
        a = np.array([d["area"] < aRng[0] or d["area"] > aRng[1] for d in dt]).reshape((1, len(dt)))
        dtIg = np.logical_or(dtIg, np.logical_and(dtm == 0, np.repeat(a, T, 0)))
        return {"image_id": imgId, "category_id": catId, "aRng": aRng, "maxDet": maxDet, "dtIds": [d["id"] for d in dt],
                "gtIds": [g["id"] for g in gt], "dtMatches": dtm, "gtMatches": gtm, "dtScores": [d["score"] for d in dt],
                "gtIgnore": gtIg, "dtIgnore": dtIg}

    eval_imgs = {}
    for k, c in enumerate(cat_ids):
        for a, rng in enumerate(area_rng):
            for i, im in enumerate(img_ids):
                eval_imgs[k, a, i] = evaluate_img(im, c, rng)

    T, R, K, A, M = len(iou_thrs), len(rec_thrs), len(cat_ids), len(area_rng), len(max_dets)
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    scores = -np.ones((T, R, K, A, M))
    for k in range(K):
        for a in range(A):
            for m, maxDet_m in enumerate(max_dets):
                E = [eval_imgs[k, a, i] for i in range(len(img_ids))]
                E = [e for e in E if e is not None]
                if len(E) == 0:
                    continue
                dtScores = np.concatenate([e["dtScores"][0:maxDet_m] for e in E])
                inds = np.argsort(-dtScores, kind="mergesort")
                dtScoresSorted = dtScores[inds]
                dtm = np.concatenate([e["dtMatches"][:, 0:maxDet_m] for e in E], axis=1)[:, inds]
                dtIg = np.concatenate([e["dtIgnore"][:, 0:maxDet_m] for e in E], axis=1)[:, inds]
                gtIg = np.concatenate([e["gtIgnore"] for e in E])
                npig = np.count_nonzero(gtIg == 0)
                if npig == 0:
                    continue
                tps = np.logical_and(dtm, np.logical_not(dtIg))
                fps = np.logical_and(np.logical_not(dtm), np.logical_not(dtIg))
                tp_sum = np.cumsum(tps, axis=1).astype(dtype=np.float64)
                fp_sum = np.cumsum(fps, axis=1).astype(dtype=np.float64)
                for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                    tp = np.array(tp)
                    fp = np.array(fp)
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    q = np.zeros((R,))
                    ss = np.zeros((R,))
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    pr = pr.tolist()
                    q = q.tolist()
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    inds_r = np.searchsorted(rc, rec_thrs, side="left")
                    try:
                        for ri, pi in enumerate(inds_r):
                            q[ri] = pr[pi]
                            ss[ri] = dtScoresSorted[pi]
                    except IndexError:
                        pass
                    precision[t, :, k, a, m] = np.array(q)
                    scores[t, :, k, a, m] = np.array(ss)
    return {"precision": precision, "recall": recall, "scores": scores, "eval_imgs": eval_imgs, "img_ids": img_ids, "cat_ids": cat_ids}
