"""Reference of "overlay v1, track colouring" (include/ore_hip.h): the painter's loop of tests/overlay_ref.py with the colour and the
label prefix taken from track ids.  It restates the whole loop (overlay_ref.py is left as it is) and shares that file's helpers: the
blend, the text "overlay v1" defines, the class name and the text bitmap."""
import math

import numpy as np

from overlay_ref import TEXT_MAX, blend, class_name, label_text, text_bitmap


def track_text(track_id, name, score):
    """"#" + decimal(id) + " " in front of overlay v1's text, cut at 40 characters."""
    return ("#" + str(int(track_id)) + " " + label_text(name, score))[:TEXT_MAX]


def overlay_track_ref(frame, boxes, scores, classes, ids, n=None, *, atlas, score_thresh=0.0, line_width, text_scale, edge_alpha=128,
                      label_alpha=204, palette, names=None):
    """frame [h, w, 3] uint8 -> the drawn frame (a new array), colour and label by ids [m] int64; rows with a negative id are not drawn."""
    frame = np.asarray(frame)
    h, w = frame.shape[:2]
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    scores = np.asarray(scores, dtype=np.float32).reshape(-1)
    ids = [int(v) for v in np.asarray(ids).reshape(-1)]
    n = len(scores) if n is None else max(0, min(int(n), len(scores)))
    L, S = int(line_width), int(text_scale)
    palette = np.asarray(palette)
    thresh = np.float32(score_thresh)

    drawn = []
    for i in range(n):
        x0, y0, x1, y1 = (np.float32(v) for v in boxes[i])
        sc = scores[i]
        if ids[i] < 0:
            continue
        if not all(math.isfinite(float(v)) for v in (x0, y0, x1, y1, sc)) or not sc >= thresh:
            continue
        X0, Y0 = max(math.floor(float(x0)), 0), max(math.floor(float(y0)), 0)
        X1, Y1 = min(math.ceil(float(x1)), w) - 1, min(math.ceil(float(y1)), h) - 1
        if X1 < X0 or Y1 < Y0:
            continue
        with np.errstate(all="ignore"):
            area = np.float32(x1 - x0) * np.float32(y1 - y0)
        area = 0.0 if math.isnan(float(area)) else float(area)
        drawn.append((-area, i, X0, Y0, X1, Y1))
    drawn.sort(key=lambda t: (t[0], t[1]))

    img = frame.astype(np.int64)
    yy, xx = np.mgrid[0:h, 0:w]
    for _, i, X0, Y0, X1, Y1 in drawn:
        cls = 0 if classes is None else int(np.asarray(classes).reshape(-1)[i])
        colour = palette[ids[i] % len(palette)].astype(np.int64)
        inside = (xx >= X0) & (xx <= X1) & (yy >= Y0) & (yy <= Y1)
        edge = inside & ((xx - X0 < L) | (X1 - xx < L) | (yy - Y0 < L) | (Y1 - yy < L))
        for k in range(3):
            img[..., k] = np.where(edge, blend(img[..., k], colour[k], int(edge_alpha)), img[..., k])
        if S < 1:
            continue
        text = track_text(ids[i], class_name(names, cls), scores[i])
        width, height = len(text) * 6 * S + 2 * S, 13 * S
        lx = min(max(X0, 0), max(w - width, 0))
        ly = min(max(Y0, 0), max(h - height, 0))
        back = (xx >= lx) & (xx < lx + width) & (yy >= ly) & (yy < ly + height)
        for k in range(3):
            img[..., k] = np.where(back, blend(img[..., k], 0, int(label_alpha)), img[..., k])
        canvas = np.zeros((max(h, ly + height), max(w, lx + width)), dtype=bool)
        bitmap = text_bitmap(text, np.asarray(atlas), S)
        canvas[ly + S:ly + S + bitmap.shape[0], lx + S:lx + S + bitmap.shape[1]] = bitmap
        glyph = canvas[:h, :w]
        tcol = colour + ((255 - colour) * 7) // 10
        for k in range(3):
            img[..., k] = np.where(glyph, tcol[k], img[..., k])
    return img.astype(np.uint8)


def track_ids_for(rows, seed=0):
    """Ids for the rows of overlay_ref.cases: small ones, some -1, some beyond a 20-colour palette, one of 19 digits (with a 32-byte
    name the text passes 40 characters)."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, 300, rows).astype(np.int64)
    ids[rng.random(rows) < 0.2] = -1
    ids[0], ids[1 % rows], ids[10 % rows], ids[12 % rows] = 7, 9223372036854775807, 1234567890123456789, -1
    ids[13 % rows] = 20                                          # the palette's length: wraps to colour 0
    return ids
