"""Reference of the wide tracker (csrc/ore_track_wide.hip): the association contract "track v1" (include/ore_hip.h) computed by ROUNDS
of mutually best pairs, the way the kernel reaches it, restated in numpy and independent of orehip.track_host's sort: no pair list, no
sort, no scan.  In every round each remaining track takes its best remaining candidate row (IoU descending, row ascending), each
remaining row its best remaining track (IoU descending, slot ascending), and the pairs that name each other are matched.  The state is
the package's dict (arrays cut at m), so a result compares with track_host's field by field.  Also the inputs the host and the GPU tests
of the wide form share."""
import numpy as np

import track_ref as TR

F = np.float32
WIDE_MAX_TRACKS, WIDE_MAX_ROWS = 16384, 8192


def empty_state():
    return {"boxes": np.zeros((0, 4), F), "classes": np.zeros(0, np.int64), "ids": np.zeros(0, np.int64), "ttl": np.zeros(0, np.int32),
            "m": 0, "next_id": 0, "frames": 0, "dropped": 0}


def iou_matrix(tb, b):
    """[m, rows] fp32, the contract's expression, every operation rounded to fp32 on its own."""
    with np.errstate(all="ignore"):
        at = ((tb[:, 2] - tb[:, 0]).astype(F) * (tb[:, 3] - tb[:, 1]).astype(F)).astype(F)
        ad = ((b[:, 2] - b[:, 0]).astype(F) * (b[:, 3] - b[:, 1]).astype(F)).astype(F)
        iw = (np.minimum(tb[:, None, 2], b[None, :, 2]) - np.maximum(tb[:, None, 0], b[None, :, 0])).astype(F)
        ih = (np.minimum(tb[:, None, 3], b[None, :, 3]) - np.maximum(tb[:, None, 1], b[None, :, 1])).astype(F)
        pos = (iw > 0) & (ih > 0)
        inter = np.where(pos, (iw * ih).astype(F), F(0))
        pos = inter > 0
        union = ((at[:, None] + ad[None, :]).astype(F) - inter).astype(F)
        return np.where(pos, (inter / np.where(pos, union, F(1))).astype(F), F(0)).astype(F)


def update_rounds(state, boxes, scores, classes=None, n=None, *, capacity=4096, iou_thresh=0.6, ttl=8, class_aware=True, score_thresh=0.0):
    """One update -> (ids [rows] int64, new state, rounds that matched at least one pair)."""
    st = empty_state() if state is None else state
    m = int(st["m"])
    tb, tc, ti, tt = st["boxes"][:m], st["classes"][:m], st["ids"][:m], st["ttl"][:m]
    b = np.asarray(boxes, dtype=F).reshape(-1, 4)
    s = np.asarray(scores, dtype=F).reshape(-1)
    rows = len(s)
    c = np.zeros(rows, np.int64) if classes is None else np.asarray(classes, dtype=np.int64).reshape(-1)
    n = rows if n is None else max(0, min(int(n), rows))
    with np.errstate(all="ignore"):
        live = (np.arange(rows) < n) & np.isfinite(b).all(1) & np.isfinite(s) & (s >= F(score_thresh))
        iou = iou_matrix(tb, b)
        cand = live[None, :] & (iou > F(iou_thresh))
    if class_aware:
        cand &= tc[:, None] == c[None, :]
    row_of = np.full(m, -1, np.int64)
    track_of = np.full(rows, -1, np.int64)
    rounds = 0
    while True:
        left = cand & (row_of < 0)[:, None] & (track_of < 0)[None, :]
        if not left.any():
            break
        v = np.where(left, iou, F(-1))
        best_row = v.argmax(1)                               # the first maximum: the lowest row of equal IoUs
        best_trk = v.argmax(0)                               # the lowest slot of equal IoUs
        t = np.nonzero(left.any(1))[0]
        t = t[best_trk[best_row[t]] == t]
        assert len(t) > 0, "a round with candidates left matches at least the first remaining pair of the total order"
        row_of[t] = best_row[t]
        track_of[best_row[t]] = t
        rounds += 1
    assert rounds <= min(m, int(live.sum()))
    ids = np.full(rows, -1, np.int64)
    new_rows = live & (track_of < 0)
    ids[live & (track_of >= 0)] = ti[track_of[live & (track_of >= 0)]]
    ids[new_rows] = int(st["next_id"]) + np.arange(int(new_rows.sum()))
    keep = (row_of < 0) & (tt.astype(np.int64) - 1 > 0)
    nb = np.concatenate([b[live], tb[keep]]).astype(F).reshape(-1, 4)
    nc = np.concatenate([c[live], tc[keep]]).astype(np.int64)
    ni = np.concatenate([ids[live], ti[keep]]).astype(np.int64)
    nt = np.concatenate([np.full(int(live.sum()), ttl), tt[keep].astype(np.int64) - 1]).astype(np.int32)
    total = len(ni)
    new = {"boxes": nb[:capacity], "classes": nc[:capacity], "ids": ni[:capacity], "ttl": nt[:capacity], "m": min(total, capacity),
           "next_id": int(st["next_id"]) + int(new_rows.sum()), "frames": int(st["frames"]) + 1, "dropped": int(st["dropped"]) + max(total - capacity, 0)}
    return ids, new, rounds


def same_state(a, b):
    """Two states in the package's form: every field, values and dtypes."""
    return all(int(a[k]) == int(b[k]) for k in ("m", "next_id", "frames", "dropped")) and \
        all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) and np.asarray(a[k]).dtype == np.asarray(b[k]).dtype for k in ("boxes", "classes", "ids", "ttl"))


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def sequence(rows, frames=5, seed=0):
    """track_ref.sequence: drifting boxes, rows that drop out and come back, new rows, dead rows (NaN, inf, low scores), a varying n."""
    return TR.sequence(rows, frames=frames, seed=seed)


def grid_case(rows, frames=4, seed=0, cells=8, n_classes=2):
    """Tie-heavy: corners on an 8-pixel grid of `cells` x `cells` positions, sides 16 or 24, so that many pairs share an IoU exactly
    (1, 1/2, 1/3, 4/9 ...) and the tie order (slot ascending, then row ascending) decides most matches."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(frames):
        x0, y0 = rng.integers(0, cells, rows) * 8.0, rng.integers(0, cells, rows) * 8.0
        w, h = rng.choice([16.0, 24.0], rows), rng.choice([16.0, 24.0], rows)
        b = np.stack([x0, y0, x0 + w, y0 + h], 1).astype(F)
        out.append((b, np.full(rows, 0.9, F), rng.integers(0, n_classes, rows).astype(np.int64), rows))
    return out


CHAIN_IOU_THRESH = TR.CHAIN_IOU_THRESH


def chain_case(k=130, t_off=0, r_off=0):
    """track_ref.chain_case: k tracks and k rows on a line, the IoU of neighbours falling strictly along it, so that only the leftmost
    remaining pair is mutually best in a round: k rounds.  t_off / r_off far-away boxes in front of the tracks / the rows lay the
    chain across the 64-bit words of the candidate masks (slots t_off .. t_off + k - 1, rows r_off .. r_off + k - 1); the fillers of
    the second frame repeat fillers of the first and match them in round 1."""
    (tb, ts, tc, _), (rb, rs, rc, _) = TR.chain_case(k)
    filler = lambda cnt: np.stack([np.arange(cnt) * 100.0, np.full(cnt, 1000.0), np.arange(cnt) * 100.0 + 50.0, np.full(cnt, 1050.0)], 1).astype(F)
    pad = lambda b, cnt: (np.concatenate([filler(cnt), b]).astype(F), np.full(cnt + k, 0.9, F), np.zeros(cnt + k, np.int64), cnt + k)
    return [pad(tb, t_off), pad(rb, r_off)]


def limit_case(rows=WIDE_MAX_ROWS, seed=7):
    """The analytic case at the limits.  Frame 1: `rows` disjoint 24 x 24 boxes at pitch 32.  Frame 2: row r is box perm[r] moved 2
    pixels right: IoU 22 * 24 / (2 * 576 - 528) = 0.846 with its predecessor and 0 with every other box.  Frame 1 issues the ids 0 ..
    rows - 1 in row order, so the ids of frame 2 are perm.  Returns (frame 1, frame 2, perm)."""
    k = np.arange(rows)
    x0, y0 = (k % 128) * 32.0, (k // 128) * 32.0
    b1 = np.stack([x0, y0, x0 + 24.0, y0 + 24.0], 1).astype(F)
    perm = np.random.default_rng(seed).permutation(rows)
    b2 = (b1[perm] + np.array([2, 0, 2, 0], F)).astype(F)
    ones, zeros = np.full(rows, 0.9, F), np.zeros(rows, np.int64)
    return (b1, ones, zeros, rows), (b2, ones, zeros, rows), perm.astype(np.int64)
