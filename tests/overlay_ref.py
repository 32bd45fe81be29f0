"""Reference of the detection overlay, render contract "overlay v1" (include/ore_hip.h): a second numpy restatement, independent of
orehip.overlay_host.  A plain painter's loop: the drawn rows are sorted with Python's sort, and every instance paints whole-frame
boolean masks -- the outline from coordinate grids, the label from a text bitmap assembled glyph by glyph, enlarged with np.kron and
pasted.  Only the glyph atlas is shared with the package (the contract names it: Pillow's embedded bitmap font)."""
import math

import numpy as np

TEXT_MAX = 40
NAME_BYTES = 32


def blend(p, c, a):
    """(p * (255 - a) + c * a + 127) / 255, integer division, on uint8 arrays / values widened to int64."""
    return (p.astype(np.int64) * (255 - a) + np.int64(c) * a + 127) // 255


def label_text(name, score):
    """name + " " + pct + "%" (pct + "%" without a name); pct = clamp((int)rintf(score * 100.0f), 0, 100) with the product in fp32."""
    with np.errstate(over="ignore"):
        prod = np.float32(score) * np.float32(100.0)
    pct = 100 if prod >= 100 else (0 if prod <= 0 else int(np.rint(prod)))       # np.rint: half to even
    text = (name + " " if name else "") + str(pct) + "%"
    return text[:TEXT_MAX]


def class_name(names, cls):
    """names[cls] cut at 32 bytes and at its first NUL, '' when the id is out of range or there is no table."""
    if names is None or not 0 <= cls < len(names):
        return ""
    return str(names[cls]).encode("ascii", "replace")[:NAME_BYTES].split(b"\0")[0].decode("ascii")


def text_bitmap(text, atlas, S):
    """[11 S, len * 6 S] bool: the glyphs side by side, every atlas cell enlarged S x S.  Characters outside 32 .. 126 are blank."""
    cells = [atlas[ord(ch) - 32] if 32 <= ord(ch) <= 126 else np.zeros((11, 6), np.uint8) for ch in text]
    small = np.concatenate(cells, axis=1) if cells else np.zeros((11, 0), np.uint8)
    return np.kron(small, np.ones((S, S), np.uint8)).astype(bool)


def overlay_ref(frame, boxes, scores, classes=None, n=None, *, atlas, score_thresh=0.0, line_width, text_scale, edge_alpha=128,
                label_alpha=204, palette, color_by="instance", names=None):
    """frame [h, w, 3] uint8 -> the drawn frame (a new array).  boxes [m, 4] / scores [m] / classes [m] or None (all 0); n = rows taken
    (None: all).  palette [k, 3] uint8 in the frame's channel order."""
    frame = np.asarray(frame)
    h, w = frame.shape[:2]
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    scores = np.asarray(scores, dtype=np.float32).reshape(-1)
    n = len(scores) if n is None else max(0, min(int(n), len(scores)))
    L, S = int(line_width), int(text_scale)
    palette = np.asarray(palette)
    thresh = np.float32(score_thresh)

    drawn = []
    for i in range(n):
        x0, y0, x1, y1 = (np.float32(v) for v in boxes[i])
        sc = scores[i]
        if not all(math.isfinite(float(v)) for v in (x0, y0, x1, y1, sc)) or not sc >= thresh:
            continue
        # Python integers: floor / ceil of a finite float32 never overflow here
        X0, Y0 = max(math.floor(float(x0)), 0), max(math.floor(float(y0)), 0)
        X1, Y1 = min(math.ceil(float(x1)), w) - 1, min(math.ceil(float(y1)), h) - 1
        if X1 < X0 or Y1 < Y0:
            continue
        with np.errstate(all="ignore"):
            area = np.float32(x1 - x0) * np.float32(y1 - y0)                     # two fp32 subtractions, one fp32 product
        area = 0.0 if math.isnan(float(area)) else float(area)
        drawn.append((-area, i, X0, Y0, X1, Y1))
    drawn.sort(key=lambda t: (t[0], t[1]))                                      # area descending, row ascending

    img = frame.astype(np.int64)
    yy, xx = np.mgrid[0:h, 0:w]
    for _, i, X0, Y0, X1, Y1 in drawn:
        cls = 0 if classes is None else int(np.asarray(classes).reshape(-1)[i])
        colour = palette[(cls if color_by == "class" else i) % len(palette)].astype(np.int64)
        inside = (xx >= X0) & (xx <= X1) & (yy >= Y0) & (yy <= Y1)
        edge = inside & ((xx - X0 < L) | (X1 - xx < L) | (yy - Y0 < L) | (Y1 - yy < L))
        for k in range(3):
            img[..., k] = np.where(edge, blend(img[..., k], colour[k], int(edge_alpha)), img[..., k])
        if S < 1:
            continue
        text = label_text(class_name(names, cls), scores[i])
        width, height = len(text) * 6 * S + 2 * S, 13 * S
        lx = min(max(X0, 0), max(w - width, 0))
        ly = min(max(Y0, 0), max(h - height, 0))
        back = (xx >= lx) & (xx < lx + width) & (yy >= ly) & (yy < ly + height)
        for k in range(3):
            img[..., k] = np.where(back, blend(img[..., k], 0, int(label_alpha)), img[..., k])
        # the text bitmap on a canvas large enough for a label that leaves the frame, cropped to the frame
        canvas = np.zeros((max(h, ly + height), max(w, lx + width)), dtype=bool)
        bitmap = text_bitmap(text, np.asarray(atlas), S)
        canvas[ly + S:ly + S + bitmap.shape[0], lx + S:lx + S + bitmap.shape[1]] = bitmap
        glyph = canvas[:h, :w]
        tcol = colour + ((255 - colour) * 7) // 10
        for k in range(3):
            img[..., k] = np.where(glyph, tcol[k], img[..., k])
    return img.astype(np.uint8)


def cases(h, w, seed=0, rows=24):
    """A mixed set of rows for an h x w frame: overlapping boxes, boxes partly and wholly outside, degenerate and non-finite rows, equal
    areas, scores at x.5 %, class ids outside a 5-name table.  Returns (boxes fp32 [rows, 4], scores fp32, classes int64)."""
    rng = np.random.default_rng(seed)
    b = np.zeros((rows, 4), np.float32)
    cx, cy = rng.uniform(0, w, rows), rng.uniform(0, h, rows)
    bw, bh = rng.uniform(1, max(w * 0.6, 2), rows), rng.uniform(1, max(h * 0.6, 2), rows)
    b[:, 0], b[:, 1], b[:, 2], b[:, 3] = cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2
    s = rng.uniform(0.02, 1.0, rows).astype(np.float32)
    c = rng.integers(0, 5, rows).astype(np.int64)
    special = [
        ([-30.5, -20.25, w * 0.4, h * 0.5], 0.125),             # partly outside, top left; 12.5 % -> 12
        ([w * 0.6, h * 0.55, w + 40.0, h + 25.0], 0.375),       # partly outside, bottom right (label clamped at both edges); 37.5 % -> 38
        ([w + 5.0, 2.0, w + 50.0, 30.0], 0.9),                  # wholly outside
        ([-50.0, -50.0, -1.0, -1.0], 0.9),                      # wholly outside
        ([w * 0.3, h * 0.3, w * 0.3, h * 0.6], 0.8),            # zero width (empty when the column is an integer)
        ([w * 0.5, h * 0.5, w * 0.2, h * 0.1], 0.8),            # reversed
        ([np.nan, 1.0, 20.0, 20.0], 0.7),
        ([1.0, 1.0, np.inf, 20.0], 0.7),
        ([1.0, 1.0, 20.0, 20.0], np.nan),
        ([2.0, 3.0, 2.0 + w * 0.25, 3.0 + h * 0.25], 0.005),    # below a 0.01 threshold; 0.5 % -> 0
        ([4.0, 6.0, 4.0 + w * 0.25, 6.0 + h * 0.25], 0.625),    # equal areas: the tie goes to the lower row
        ([7.0, 9.0, 7.0 + w * 0.25, 9.0 + h * 0.25], 0.995),    # the fp32 product is 99.5: half to even -> 100
        ([w - 10.0, h - 6.0, w - 1.5, h - 0.5], 1.0),           # small, bottom right: the label is pushed back into the frame
        ([-3e38, -3e38, 3e38, 3e38], 0.45),                     # the whole frame; the area overflows to +inf
        ([10.5, 5.0, 10.5, 20.0], 0.55),                        # zero width at a fractional column: one pixel wide, area 0
        ([-3e38, 5.5, 3e38, 5.5], 0.65),                        # inf * 0: the NaN area counts as 0; one pixel high
    ]
    for k, (box, sc) in enumerate(special[:rows]):
        b[k], s[k] = box, sc
    c[3 % rows], c[10 % rows], c[11 % rows] = 17, -2, 5           # ids outside the names table
    return b, s, c
