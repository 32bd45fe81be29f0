"""Reference of the detection tracker, association contract "track v1" (include/ore_hip.h): a second restatement, independent of
orehip.track_host.  Plain Python over numpy fp32 scalars: every candidate pair is listed, the list is sorted by the stated key with
Python's sort, scanned once, and the track list is rebuilt from Python lists.  The state is a dict of Python lists and ints.  Also the
case generators the host and the GPU tests share."""
import math

import numpy as np

F = np.float32


def empty_state():
    return {"tracks": [], "next_id": 0, "frames": 0, "dropped": 0}          # a track: (box 4-tuple of np.float32, class, id, ttl)


def iou_ref(t, d):
    """The contract's IoU of two xyxy boxes of np.float32, every operation a single fp32 operation."""
    with np.errstate(all="ignore"):
        area_t = F(F(t[2] - t[0]) * F(t[3] - t[1]))
        area_d = F(F(d[2] - d[0]) * F(d[3] - d[1]))
        iw = F(min(t[2], d[2]) - max(t[0], d[0]))
        ih = F(min(t[3], d[3]) - max(t[1], d[1]))
        inter = F(iw * ih) if (iw > 0 and ih > 0) else F(0)
        if not inter > 0:
            return F(0)
        return F(inter / F(F(area_t + area_d) - inter))


def update_ref(state, boxes, scores, classes=None, n=None, *, capacity=1024, iou_thresh=0.6, ttl=8, class_aware=True, score_thresh=0.0):
    """One update -> (ids [rows] int64, new state).  boxes [rows, 4], scores [rows], classes [rows] or None; n = rows taken (None: all)."""
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    scores = np.asarray(scores, dtype=np.float32).reshape(-1)
    rows = len(scores)
    classes = [0] * rows if classes is None else [int(c) for c in np.asarray(classes).reshape(-1)]
    n = rows if n is None else max(0, min(int(n), rows))
    thr_s, thr_i = F(score_thresh), F(iou_thresh)
    live = []
    for i in range(rows):
        vals = [float(v) for v in boxes[i]] + [float(scores[i])]
        live.append(i < n and all(math.isfinite(v) for v in vals) and bool(scores[i] >= thr_s))
    tracks = state["tracks"]
    pairs = []
    rowf = [tuple(float(v) for v in boxes[d]) for d in range(rows)]         # exact copies, for the quick rejection below
    for slot, (tbox, tcls, _, _) in enumerate(tracks):
        t0, t1, t2, t3 = (float(v) for v in tbox)
        for d in range(rows):
            if not live[d] or (class_aware and tcls != classes[d]):
                continue
            r = rowf[d]
            if not (min(t2, r[2]) > max(t0, r[0]) and min(t3, r[3]) > max(t1, r[1])):
                continue                                                    # iw <= 0 or ih <= 0: IoU 0, never above a threshold >= 0
            v = iou_ref(tbox, boxes[d])
            if v > thr_i:                                                   # strict; a NaN compares false
                pairs.append((-float(v), slot, d))
    pairs.sort()                                                            # iou descending, slot ascending, row ascending
    row_of, track_of = {}, {}
    for _, slot, d in pairs:
        if slot not in row_of and d not in track_of:
            row_of[slot], track_of[d] = d, slot
    ids = np.full(rows, -1, dtype=np.int64)
    next_id = state["next_id"]
    new = []
    for d in range(rows):
        if not live[d]:
            continue
        if d in track_of:
            ids[d] = tracks[track_of[d]][2]
        else:
            ids[d] = next_id
            next_id += 1
        new.append((tuple(F(v) for v in boxes[d]), classes[d], int(ids[d]), int(ttl)))
    for slot, (tbox, tcls, tid, tttl) in enumerate(tracks):
        if slot not in row_of and tttl - 1 > 0:
            new.append((tbox, tcls, tid, tttl - 1))
    cut = max(len(new) - int(capacity), 0)
    return ids, {"tracks": new[:int(capacity)], "next_id": next_id, "frames": state["frames"] + 1, "dropped": state["dropped"] + cut,
                 "n_pairs": len(pairs)}


def state_arrays(state):
    """The reference state in the package's form: {boxes [m, 4] fp32, classes, ids int64, ttl int32, m, next_id, frames, dropped}."""
    tr = state["tracks"]
    return {"boxes": np.array([t[0] for t in tr], dtype=np.float32).reshape(-1, 4), "classes": np.array([t[1] for t in tr], dtype=np.int64),
            "ids": np.array([t[2] for t in tr], dtype=np.int64), "ttl": np.array([t[3] for t in tr], dtype=np.int32), "m": len(tr),
            "next_id": state["next_id"], "frames": state["frames"], "dropped": state["dropped"]}


def same_state(got, want):
    """got: the package's state dict (arrays cut at m); want: a reference state."""
    w = state_arrays(want)
    return all(int(got[k]) == int(w[k]) for k in ("m", "next_id", "frames", "dropped")) and \
        all(np.array_equal(np.asarray(got[k]), w[k]) and np.asarray(got[k]).dtype == w[k].dtype for k in ("boxes", "classes", "ids", "ttl"))


# ---- case generators -------------------------------------------------------------------------------------------------------
def sequence(rows, frames=12, seed=0, n_classes=3, extent=400.0):
    """`frames` frames of `rows` row slots each: objects drift a few pixels per frame; some drop out for 1 .. 9 frames (both sides of
    ttl = 8) and come back where they would be; new objects appear in freed slots; a few rows are low scores, NaN or inf; the count n
    varies below `rows`.  Returns a list of (boxes fp32 [rows, 4], scores fp32 [rows], classes int64 [rows], n)."""
    rng = np.random.default_rng(seed)
    objs = max(rows + rows // 3, 1)
    cx, cy = rng.uniform(0, extent, objs), rng.uniform(0, extent, objs)
    bw, bh = rng.uniform(12, 60, objs), rng.uniform(12, 60, objs)
    vx, vy = rng.uniform(-3, 3, objs), rng.uniform(-3, 3, objs)
    cls = rng.integers(0, n_classes, objs)
    out_until = np.zeros(objs, dtype=np.int64)                   # the object is absent while frame < out_until
    out = []
    for f in range(frames):
        cx, cy = cx + vx, cy + vy
        for o in range(objs):
            if f > 0 and out_until[o] <= f and rng.random() < 0.15:
                out_until[o] = f + int(rng.integers(1, 10))      # 1 .. 9 frames away
        present = [o for o in range(objs) if out_until[o] <= f and (o < rows or f >= 2 + (o % 5))]
        order = rng.permutation(len(present))[:rows]             # the detector's order changes from frame to frame
        b = np.zeros((rows, 4), np.float32)
        s = np.zeros(rows, np.float32)
        c = np.zeros(rows, np.int64)
        for k, j in enumerate(order):
            o = present[j]
            jit = rng.uniform(-1.0, 1.0, 4)
            b[k] = [cx[o] - bw[o] / 2 + jit[0], cy[o] - bh[o] / 2 + jit[1], cx[o] + bw[o] / 2 + jit[2], cy[o] + bh[o] / 2 + jit[3]]
            s[k] = rng.uniform(0.3, 1.0)
            c[k] = cls[o]
        filled = len(order)
        for k in range(filled):
            r = rng.random()
            if r < 0.03:
                s[k] = 0.01                                      # below the tests' score threshold
            elif r < 0.05:
                b[k, int(rng.integers(0, 4))] = [np.nan, np.inf, -np.inf][int(rng.integers(0, 3))]
            elif r < 0.06:
                s[k] = np.nan
        n = filled if f % 3 else max(filled - int(rng.integers(0, 3)), 0)
        out.append((b, s, c, n))
    return out


def ties_case():
    """Three frames whose pairs tie exactly: frame 0 holds duplicate boxes (so the track list holds duplicates), frames 1 and 2 repeat
    them in other orders with further duplicates -- many pairs of IoU exactly 1, and equal IoUs below 1 from boxes shifted by whole pixels."""
    base = np.array([[10, 10, 50, 50], [10, 10, 50, 50], [10, 10, 50, 50], [100, 20, 140, 60], [100, 20, 140, 60], [30, 200, 90, 260]], np.float32)
    f0 = (base, np.full(len(base), 0.9, np.float32), np.zeros(len(base), np.int64), len(base))
    b1 = np.concatenate([base[[3, 0, 5, 1]], base[[0, 3]] + np.float32(2), base[[0, 3]] - np.float32(2), base[[5, 5]], base[[0]] + np.array([2, 0, 2, 0], np.float32)])
    f1 = (b1.astype(np.float32), np.full(len(b1), 0.8, np.float32), np.zeros(len(b1), np.int64), len(b1))
    b2 = np.concatenate([b1[::-1], base]).astype(np.float32)
    f2 = (b2, np.full(len(b2), 0.7, np.float32), np.zeros(len(b2), np.int64), len(b2))
    return [f0, f1, f2]


CHAIN_IOU_THRESH = 0.3


def chain_case(k=40):
    """k tracks and k rows of one size on a line, T0 R0 T1 R1 ..., every box overlapping its neighbours, the gaps between consecutive
    boxes growing along the line (8 px, then eps more each time, to about 28 px of the 64 px width).  The IoU of neighbours therefore
    falls strictly along the path T0-R0-T1-R1-...: the greedy order walks it from the left, accepts (T_i, R_i) and rejects (T_i+1,
    R_i), and in a mutual-best matching only the leftmost remaining pair is mutually best -- one pair per round, k rounds.  With
    iou_thresh = CHAIN_IOU_THRESH every neighbour pair (and the pairs three gaps apart) is a candidate.  Coordinates are multiples of
    1 / 32: exact in fp32.  Returns [frame 0 = the tracks, frame 1 = the rows]."""
    eps = 2.0 ** math.floor(math.log2(20.0 / (2 * k)))            # 40: 0.25, 320: 1 / 32
    gaps = 8.0 + eps * np.arange(2 * k - 1)
    x = np.concatenate([[0.0], np.cumsum(gaps)])
    box = lambda xs: np.stack([xs, np.zeros(len(xs)), xs + 64.0, np.full(len(xs), 32.0)], 1).astype(np.float32)
    ones, zeros = np.full(k, 0.9, np.float32), np.zeros(k, np.int64)
    return [(box(x[0::2]), ones, zeros, k), (box(x[1::2]), ones, zeros, k)]


def mutual_best_rounds(tracks, rows, iou_thresh):
    """How many rounds a mutual-best matching of boxes `tracks` x `rows` (one class) needs -- the rounds that commit at least one pair."""
    T, R = len(tracks), len(rows)
    iou = np.array([[iou_ref(tracks[t], rows[d]) for d in range(R)] for t in range(T)], dtype=np.float32)
    ok = iou > F(iou_thresh)
    free_t, free_r, rounds = set(range(T)), set(range(R)), 0
    while True:
        best_row = {t: min(((-iou[t, d], d) for d in free_r if ok[t, d]), default=None) for t in free_t}
        best_trk = {d: min(((-iou[t, d], t) for t in free_t if ok[t, d]), default=None) for d in free_r}
        commit = [(t, br[1]) for t, br in best_row.items() if br is not None and best_trk[br[1]][1] == t]
        if not commit:
            return rounds
        rounds += 1
        for t, d in commit:
            free_t.discard(t)
            free_r.discard(d)
