"""The tile plan, the gather, the seam rule with its transform and the tiled composition, stated a second time in numpy -- row by row,
with none of orehip's host functions -- for tests/test_tile_host.py (the host statements against it) and tests/test_hip_tiles.py (the
kernels and the wrapper against it)."""
import math

import numpy as np

LEFT, TOP, RIGHT, BOTTOM = 1, 2, 4, 8


def axis_starts(L, t, o):
    """Tile starts along one axis of length L for tile t, overlap o: (extent, starts)."""
    assert 0 <= o < t and L >= 1
    if L <= t:
        return L, [0]
    s = t - o
    n = int(math.ceil((L - t) / s)) + 1
    return t, [min(k * s, L - t) for k in range(n)]


def plan(h, w, tile_hw, overlap_hw):
    th, ys = axis_starts(h, tile_hw[0], overlap_hw[0])
    tw, xs = axis_starts(w, tile_hw[1], overlap_hw[1])
    return dict(th=th, tw=tw, ny=len(ys), nx=len(xs), stride_y=tile_hw[0] - overlap_hw[0], stride_x=tile_hw[1] - overlap_hw[1],
                origins=[(y, x) for y in ys for x in xs])


def gather(frame, p, swap_rb=False):
    """[n, 3, th, tw]: numpy slicing of every tile, planar."""
    out = np.empty((len(p["origins"]), 3, p["th"], p["tw"]), dtype=np.uint8)
    for i, (y0, x0) in enumerate(p["origins"]):
        crop = frame[y0:y0 + p["th"], x0:x0 + p["tw"]]
        for c in range(3):
            out[i, c] = crop[:, :, 2 - c if swap_rb else c]
    return out


def edges_of(p, i, h, w):
    y0, x0 = p["origins"][i]
    e = 0
    if x0 > 0:
        e |= LEFT
    if y0 > 0:
        e |= TOP
    if x0 + p["tw"] < w:
        e |= RIGHT
    if y0 + p["th"] < h:
        e |= BOTTOM
    return e


def collect(boxes, scores, classes, sx, sy, ox, oy, src_hw, edges, margin):
    """Row by row in np.float32 scalars: (kept boxes [k, 4], scores, classes, indices of the kept rows, number rejected)."""
    f = np.float32
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    m, x_hi, y_hi = f(margin), f(f(src_hw[1]) - f(margin)), f(f(src_hw[0]) - f(margin))
    sx, sy, ox, oy = f(sx), f(sy), f(ox), f(oy)
    out, idx = [], []
    with np.errstate(all="ignore"):
        for i, (x0, y0, x1, y1) in enumerate(boxes):
            if (edges & LEFT and x0 < m) or (edges & TOP and y0 < m) or (edges & RIGHT and x1 > x_hi) or (edges & BOTTOM and y1 > y_hi):
                continue
            out.append([f(f(x0 * sx) + ox), f(f(y0 * sy) + oy), f(f(x1 * sx) + ox), f(f(y1 * sy) + oy)])
            idx.append(i)
    idx = np.asarray(idx, dtype=np.int64)
    cls = np.zeros(len(boxes), dtype=np.int64) if classes is None else np.asarray(classes, dtype=np.int64)
    return (np.asarray(out, dtype=np.float32).reshape(-1, 4), np.asarray(scores, dtype=np.float32)[idx], cls[idx], idx, len(boxes) - len(idx))


def sources(frame, p, full_hw, resize, swap_rb=False):
    """The sources of a frame in pass order -- the resized full frame first (when full_hw is given), then the tiles in plan order --
    as dicts(image [3, sh, sw] uint8, sx, sy, ox, oy, src_hw, edges).  resize(hwc, nh, nw) -> hwc is the caller's (Pillow's)."""
    h, w = frame.shape[:2]
    src = []
    if full_hw is not None:
        nh, nw = full_hw
        img = resize(frame, nh, nw)
        img = img[:, :, ::-1] if swap_rb else img
        src.append(dict(image=np.ascontiguousarray(img.transpose(2, 0, 1)), sx=w * 1.0 / nw, sy=h * 1.0 / nh, ox=0.0, oy=0.0,
                        src_hw=(nh, nw), edges=0))
    tiles = gather(frame, p, swap_rb)
    for i, (y0, x0) in enumerate(p["origins"]):
        src.append(dict(image=tiles[i], sx=1.0, sy=1.0, ox=float(x0), oy=float(y0), src_hw=(p["th"], p["tw"]), edges=edges_of(p, i, h, w)))
    return src


def hand_rows(n, src_hw, margin, seed):
    """n detection rows of an [sh, sw] source that sit on the seam rule's edges: coordinates exactly at `margin`, one ulp below and
    above it, exactly at sw - margin / sh - margin and one ulp either side, NaN and +-inf coordinates, and random boxes between.
    Returns (boxes [n, 4] float32, scores [n] float32 -- distinct, positive --, classes [n] int64)."""
    f = np.float32
    sh, sw = src_hw
    rng = np.random.default_rng(seed)
    m = f(margin)
    x_hi, y_hi = f(f(sw) - m), f(f(sh) - m)
    lo = [m, np.nextafter(m, f(-np.inf)), np.nextafter(m, f(np.inf)), f(0), f(-1.5)]
    hi_x = [x_hi, np.nextafter(x_hi, f(-np.inf)), np.nextafter(x_hi, f(np.inf)), f(sw), f(sw + 3)]
    hi_y = [y_hi, np.nextafter(y_hi, f(-np.inf)), np.nextafter(y_hi, f(np.inf)), f(sh), f(sh + 3)]
    special = [f(np.nan), f(np.inf), f(-np.inf)]
    boxes = np.empty((n, 4), dtype=np.float32)
    ctr = rng.uniform(0.05, 0.95, (n, 2)) * [sw, sh]
    half = rng.uniform(2.0, 0.2 * min(sh, sw), (n, 2))
    boxes[:, 0], boxes[:, 1] = ctr[:, 0] - half[:, 0], ctr[:, 1] - half[:, 1]
    boxes[:, 2], boxes[:, 3] = ctr[:, 0] + half[:, 0], ctr[:, 1] + half[:, 1]
    i = 0
    for col, vals in ((0, lo), (1, lo), (2, hi_x), (3, hi_y)):             # one edge value per row, the other coordinates inside
        for v in vals:
            boxes[i, col] = v
            i += 1
    for col in range(4):                                                   # non-finite coordinates: no comparison with NaN is true
        for v in special:
            boxes[i, col] = v
            i += 1
    boxes[i] = [lo[1], lo[1], hi_x[2], hi_y[2]]                            # outside on all four sides
    boxes[i + 1] = [lo[0], lo[0], hi_x[0], hi_y[0]]                        # exactly on all four limits: kept
    assert i + 2 <= n
    scores = rng.permutation(n).astype(np.float32) / f(n) + f(0.001)
    classes = rng.integers(0, 5, n).astype(np.int64)
    return boxes, scores, classes
