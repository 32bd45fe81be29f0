"""Reference of the support crops ("support crop v1", include/ore_hip.h): the geometry in pure Python integers, the support box in
numpy float32 operations taken one by one, and Pillow's Image.resize(..., BILINEAR) for the pixels.  Shared by tests/test_support_host.py
and tests/test_hip_support.py."""
import math

import numpy as np
from PIL import Image

SIZE, CONTEXT, FILL = 240, 16, (104, 116, 124)


def geometry(h, w, box, S=SIZE, c=CONTEXT):
    """{"D", "origin", "src", "dst"} of one box, or ValueError where the box lies outside the frame."""
    x1, y1, x2, y2 = (float(np.float32(v)) for v in box)
    T = S - 2 * c
    bx0, by0 = max(0, math.floor(x1)), max(0, math.floor(y1))
    bx1, by1 = min(w, math.ceil(x2)), min(h, math.ceil(y2))
    bw, bh = bx1 - bx0, by1 - by0
    if bw < 1 or bh < 1:
        raise ValueError("the box lies outside the frame")
    L = max(bw, bh)
    m = (c * L + T - 1) // T
    D = L + 2 * m
    x0, y0 = bx0 - (D - bw) // 2, by0 - (D - bh) // 2
    rx0, rx1, ry0, ry1 = max(x0, 0), min(x0 + D, w), max(y0, 0), min(y0 + D, h)
    dx0, dx1 = ((rx0 - x0) * S + D // 2) // D, ((rx1 - x0) * S + D // 2) // D
    dy0, dy1 = ((ry0 - y0) * S + D // 2) // D, ((ry1 - y0) * S + D // 2) // D
    return {"D": D, "origin": (x0, y0), "src": (rx0, ry0, rx1, ry1), "dst": (dx0, dy0, dx1, dy1)}


def support_box(box, g, S=SIZE):
    """The box inside the crop: fp32, sx = float(nw) / float(sw); x' = float(dx0) + (x - float(rx0)) * sx; clipped to [0, S]."""
    f = np.float32
    (rx0, ry0, rx1, ry1), (dx0, dy0, dx1, dy1) = g["src"], g["dst"]
    sx, sy = f(dx1 - dx0) / f(rx1 - rx0), f(dy1 - dy0) / f(ry1 - ry0)
    b = [f(v) for v in box]
    out = np.array([f(dx0) + (b[0] - f(rx0)) * sx, f(dy0) + (b[1] - f(ry0)) * sy,
                    f(dx0) + (b[2] - f(rx0)) * sx, f(dy0) + (b[3] - f(ry0)) * sy], dtype=np.float32)
    return np.clip(out, f(0), f(S)).astype(np.float32)


def crop(frame, box, S=SIZE, c=CONTEXT, fill=FILL):
    """(crop [3, S, S] uint8, support box float32 [4]) of one box of frame [h, w, 3] uint8."""
    h, w = frame.shape[:2]
    g = geometry(h, w, box, S, c)
    (rx0, ry0, rx1, ry1), (dx0, dy0, dx1, dy1) = g["src"], g["dst"]
    out = np.empty((S, S, 3), dtype=np.uint8)
    out[:] = np.asarray(fill, dtype=np.uint8)
    out[dy0:dy1, dx0:dx1] = np.asarray(Image.fromarray(np.ascontiguousarray(frame[ry0:ry1, rx0:rx1])).resize((dx1 - dx0, dy1 - dy0), Image.BILINEAR))
    return np.ascontiguousarray(out.transpose(2, 0, 1)), support_box(box, g, S)


def crops(frames, boxes, frame_index=None, S=SIZE, c=CONTEXT, fill=FILL):
    """The per-job reference of a whole call: ([K, 3, S, S] uint8, [K, 4] float32)."""
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    fi = [0] * len(boxes) if frame_index is None else list(frame_index)
    got = [crop(frames[fi[k]], boxes[k], S, c, fill) for k in range(len(boxes))]
    return np.stack([g[0] for g in got]), np.stack([g[1] for g in got])
