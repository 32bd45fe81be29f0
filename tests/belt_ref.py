"""Reference of the belt's shift, contract "belt shift v1" (include/ore_hip.h): a second restatement, independent of
orehip.belt_shift_host.  Plain Python over numpy fp32 scalars: every (track, row) pair is visited in two loops, the histogram is a dict,
the smoothed peak is found by sorting the bins' keys with Python's sort.  The track state is the package's dict (track_host's), the belt
state a dict of ints.  Also the case generators the host and the GPU tests share."""
import math

import numpy as np

import track_ref as TR

F = np.float32
BELT_KEYS = ("dx", "dy", "votes", "travel_x", "travel_y", "frames", "coasted")


def empty_belt():
    return {k: 0 for k in BELT_KEYS}


def empty_tracks():
    return {"boxes": np.zeros((0, 4), np.float32), "classes": np.zeros(0, np.int64), "ids": np.zeros(0, np.int64), "ttl": np.zeros(0, np.int32),
            "m": 0, "next_id": 0, "frames": 0, "dropped": 0}


def geo_ref(box):
    """(w, h, sx, sy) of an xyxy box of np.float32: one fp32 operation each."""
    with np.errstate(all="ignore"):
        return F(box[2] - box[0]), F(box[3] - box[1]), F(box[0] + box[2]), F(box[1] + box[3])


def _q(sd, st, inv):
    """floorf((sd - st) * inv + 0.5f): a difference, a product, a sum, each rounded to fp32, then the floor (NaN if not finite)."""
    v = F(F(F(sd - st) * inv) + F(0.5))
    return F(math.floor(v)) if math.isfinite(v) else F(np.nan)


def bin_ref(tg, dg, tol, inv, K):
    """The bin (qx, qy) the pair of geometries votes for, or None: the size gate and the window, single fp32 operations."""
    with np.errstate(all="ignore"):
        for a, b in ((tg[0], dg[0]), (tg[1], dg[1])):
            if not (F(abs(F(a - b))) <= F(tol * max(a, b))):
                return None
        qx, qy = _q(dg[2], tg[2], inv), _q(dg[3], tg[3], inv)
    if not (abs(qx) <= F(K)) or not (abs(qy) <= F(K)):
        return None
    return int(qx), int(qy)


def shift_ref(state, belt, boxes, scores, classes=None, n=None, *, bin=2, half_bins=64, size_tol=0.125, min_votes=3, frame_h=0, frame_w=0,
              score_thresh=0.0, class_aware=True):
    """One shift -> (the track state moved, the new belt state).  state: the package's track state dict or None, belt: a dict or None."""
    state = empty_tracks() if state is None else state
    belt = empty_belt() if belt is None else belt
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    scores = np.asarray(scores, dtype=np.float32).reshape(-1)
    rows = len(scores)
    classes = [0] * rows if classes is None else [int(c) for c in np.asarray(classes).reshape(-1)]
    n = rows if n is None else max(0, min(int(n), rows))
    K, tol, inv, thr = int(half_bins), F(size_tol), F(1.0 / (2 * bin)), F(score_thresh)
    m = int(state["m"])
    tboxes = np.asarray(state["boxes"], dtype=np.float32).reshape(-1, 4)[:m]
    tcls = [int(c) for c in np.asarray(state["classes"]).reshape(-1)[:m]]
    live = []
    for i in range(rows):
        vals = [float(v) for v in boxes[i]] + [float(scores[i])]
        live.append(i < n and all(math.isfinite(v) for v in vals) and bool(scores[i] >= thr))
    dgeo = [geo_ref(boxes[d]) for d in range(rows)]
    dfl = [tuple(float(v) for v in g) for g in dgeo]            # exact copies, for the quick rejection below
    reach = (K + 2) * 2.0 * bin                                 # |sxd - sxt| beyond this rounds to a q beyond K, whatever the rounding
    hist = {}
    for t in range(m):
        tg = geo_ref(tboxes[t])
        if not (tg[0] > 0 and tg[1] > 0):
            continue
        w, h, sx, sy = (float(v) for v in tg)
        for d in range(rows):
            if not live[d] or (class_aware and tcls[t] != classes[d]):
                continue
            g = dfl[d]
            if not (g[0] > 0 and g[1] > 0):
                continue
            if abs(g[2] - sx) > reach or abs(g[3] - sy) > reach:
                continue
            if abs(w - g[0]) > 1.001 * float(tol) * max(w, g[0]) + 1e-3 or abs(h - g[1]) > 1.001 * float(tol) * max(h, g[1]) + 1e-3:
                continue                                        # far beyond the gate: no rounding brings it back
            q = bin_ref(tg, dgeo[d], tol, inv, K)
            if q is not None:
                hist[q] = hist.get(q, 0) + 1
    keys = []
    for qy in range(-K, K + 1):
        for qx in range(-K, K + 1):
            s = sum(hist.get((qx + u, qy + v), 0) for v in (-1, 0, 1) for u in (-1, 0, 1))
            keys.append((-s, abs(qx * bin - belt["dx"]) + abs(qy * bin - belt["dy"]), qy, qx))
    keys.sort()
    neg_s, _, qy, qx = keys[0]
    new = dict(belt)
    if -neg_s >= min_votes:
        new["dx"], new["dy"], new["votes"] = qx * bin, qy * bin, -neg_s
    else:
        new["votes"] = 0
        new["coasted"] = belt["coasted"] + 1
    new["travel_x"] = belt["travel_x"] + new["dx"]
    new["travel_y"] = belt["travel_y"] + new["dy"]
    new["frames"] = belt["frames"] + 1
    moved = np.zeros((m, 4), np.float32)
    ttl = [int(v) for v in np.asarray(state["ttl"]).reshape(-1)[:m]]
    dx, dy = F(new["dx"]), F(new["dy"])
    with np.errstate(all="ignore"):
        for t in range(m):
            x0, y0, x1, y1 = F(tboxes[t][0] + dx), F(tboxes[t][1] + dy), F(tboxes[t][2] + dx), F(tboxes[t][3] + dy)
            moved[t] = (x0, y0, x1, y1)
            if (frame_h > 0 or frame_w > 0) and (x1 <= 0 or x0 >= F(frame_w) or y1 <= 0 or y0 >= F(frame_h)):
                ttl[t] = 1
    out = dict(state)
    out["boxes"], out["ttl"] = moved, np.array(ttl, dtype=np.int32)
    out["n_votes"] = sum(hist.values())
    return out, new


def same_tracks(got, want):
    """Two track states in the package's form: the four counters, and equality and dtype of every array cut at m."""
    m = int(want["m"])
    return all(int(got[k]) == int(want[k]) for k in ("m", "next_id", "frames", "dropped")) and \
        all(np.array_equal(np.asarray(got[k])[:m].view(np.uint8 if k == "boxes" else np.asarray(got[k]).dtype),
                           np.asarray(want[k])[:m].view(np.uint8 if k == "boxes" else np.asarray(want[k]).dtype)) and
            np.asarray(got[k]).dtype == np.asarray(want[k]).dtype for k in ("boxes", "classes", "ids", "ttl"))


def same_belt(got, want):
    return all(int(got[k]) == int(want[k]) for k in BELT_KEYS)


def tracks_of(boxes, classes=None, ttl=8, first_id=0):
    """A track state holding these boxes as tracks first_id, first_id + 1, ..."""
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    m = len(boxes)
    return {"boxes": boxes.copy(), "classes": np.zeros(m, np.int64) if classes is None else np.asarray(classes, dtype=np.int64),
            "ids": first_id + np.arange(m, dtype=np.int64), "ttl": np.full(m, ttl, np.int32), "m": m, "next_id": first_id + m, "frames": 1,
            "dropped": 0}


def rows_of(boxes, classes=None, score=0.9):
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    return boxes, np.full(len(boxes), score, np.float32), np.zeros(len(boxes), np.int64) if classes is None else np.asarray(classes, dtype=np.int64), len(boxes)


# ---- case generators -------------------------------------------------------------------------------------------------------
def moving_sequence(rows, shift, frames=5, seed=0):
    """track_ref.sequence (drift of a few pixels, drop-outs, new objects, NaN / inf / low-score rows, a varying n) on a belt: frame f is
    moved by f * shift as a whole.  The non-finite coordinates stay what they are."""
    out = []
    for f, (b, s, c, n) in enumerate(TR.sequence(rows, frames=frames, seed=seed)):
        b = b.copy()
        with np.errstate(all="ignore"):
            b[:, 0::2] += F(f * shift[0])
            b[:, 1::2] += F(f * shift[1])
        out.append((b, s, c, n))
    return out


def belt_sequence(objs, shift=(37, 2), frames=8, seed=0, frame=(1080, 1920), miss=0.05):
    """The planted belt: `objs` boxes of 20 .. 70 px on a frame, all moving by `shift` per frame, +-1 px of detection jitter on every
    coordinate, each detection missed with probability `miss`, the rows in a new order in every frame.  Returns a list of
    (boxes, scores, classes, n, objects): objects[k] = the object row k shows."""
    rng = np.random.default_rng(seed)
    h, w = frame
    cx, cy = rng.uniform(0, w, objs), rng.uniform(0, h, objs)
    bw, bh = rng.uniform(20, 70, objs), rng.uniform(20, 70, objs)
    out = []
    for f in range(frames):
        seen = np.nonzero(rng.random(objs) >= miss)[0]
        seen = seen[rng.permutation(len(seen))]
        jit = rng.uniform(-1.0, 1.0, (len(seen), 4))
        x, y = cx[seen] + f * shift[0], cy[seen] + f * shift[1]
        b = np.stack([x - bw[seen] / 2, y - bh[seen] / 2, x + bw[seen] / 2, y + bh[seen] / 2], 1) + jit
        out.append((b.astype(np.float32), rng.uniform(0.3, 1.0, len(seen)).astype(np.float32), np.zeros(len(seen), np.int64), len(seen), seen))
    return out


def kept_ids(frames, ids_per_frame):
    """(objects seen in two consecutive frames that kept their id, how many there were) over a belt_sequence and the ids of its rows."""
    kept = total = 0
    for f in range(1, len(frames)):
        before = {int(o): int(i) for o, i in zip(frames[f - 1][4], ids_per_frame[f - 1])}
        for o, i in zip(frames[f][4], ids_per_frame[f]):
            if int(o) in before:
                total += 1
                kept += int(before[int(o)] == int(i))
    return kept, total


def lattice_case(rows=8192, pitch=300, size=40, shift=(36, -8), cols=128):
    """Boxes of one size on a lattice whose pitch exceeds the window (radius 128 + the shift < pitch): a pair votes iff it is a row and
    its own track.  Frame 0: `rows` boxes; frame 1: the same moved by `shift`, in a fixed permutation.  Returns (frame 0, frame 1, perm)
    with frame 1's row k = object perm[k]."""
    k = np.arange(rows)
    x0, y0 = (k % cols) * float(pitch), (k // cols) * float(pitch)
    b0 = np.stack([x0, y0, x0 + size, y0 + size], 1).astype(np.float32)
    perm = (k * 4099 + 17) % rows                               # 4099 is odd: a permutation of a power of two
    b1 = (b0[perm] + np.array([shift[0], shift[1], shift[0], shift[1]], np.float32)).astype(np.float32)
    ones, zeros = np.full(rows, 0.9, np.float32), np.zeros(rows, np.int64)
    return (b0, ones, zeros, rows), (b1, ones, zeros, rows), perm
