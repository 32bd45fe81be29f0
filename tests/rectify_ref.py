"""An independent reference of the contract "rectify v1" (include/ore_hip.h), written from the contract's text and not from
orehip.rectify_host: one output pixel at a time, scalar binary32 arithmetic, Python integers behind it.  Also the case table the host
and the device tests share.

binary32 here is Python's double arithmetic rounded to binary32 after every operation: for +, -, * and / of two binary32 operands the
double result rounded once more to binary32 is the correctly rounded binary32 result (53 >= 2 * 24 + 2 bits), so each step is the one
IEEE binary32 operation the contract names.  A division that meets a zero, an infinity or a NaN goes through numpy's float32."""
import functools
import math
import struct

import numpy as np


def f32(x):
    """x rounded to binary32 (as a Python float)."""
    try:
        return struct.unpack("f", struct.pack("f", x))[0]
    except OverflowError:
        return math.copysign(math.inf, x)


def _div(a, b):
    if b == 0.0 or not (math.isfinite(a) and math.isfinite(b)):
        with np.errstate(all="ignore"):
            return float(np.float32(a) / np.float32(b))
    return f32(a / b)


def _clamp(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


def positions(m, i, j, hs, ws):
    """(inside, U, V) of output pixel (i, j): the contract's fixed-point source position in 1/256 px, or (False, None, None)."""
    xo, yo = f32(float(j) + 0.5), f32(float(i) + 0.5)
    X = f32(f32(f32(m[0] * xo) + f32(m[1] * yo)) + m[2])
    Y = f32(f32(f32(m[3] * xo) + f32(m[4] * yo)) + m[5])
    Z = f32(f32(f32(m[6] * xo) + f32(m[7] * yo)) + m[8])
    u, v = f32(_div(X, Z) - 0.5), f32(_div(Y, Z) - 0.5)
    inside = math.isfinite(X) and math.isfinite(Y) and math.isfinite(Z) and Z > 0 and -0.5 <= u <= f32(float(ws) - 0.5) and \
        -0.5 <= v <= f32(float(hs) - 0.5)
    if not inside:
        return False, None, None
    return True, int(math.floor(f32(f32(u * 256.0) + 0.5))), int(math.floor(f32(f32(v * 256.0) + 0.5)))


def blend(src, U, V):
    """The three bytes the contract's integer blend gives at the fixed-point position (U, V)."""
    hs, ws = src.shape[:2]
    x0, fx, y0, fy = U >> 8, U & 255, V >> 8, V & 255
    xa, xb = _clamp(x0, 0, ws - 1), _clamp(x0 + 1, 0, ws - 1)
    ya, yb = _clamp(y0, 0, hs - 1), _clamp(y0 + 1, 0, hs - 1)
    out = []
    for c in range(3):
        a, b, cc, d = int(src[ya, xa, c]), int(src[ya, xb, c]), int(src[yb, xa, c]), int(src[yb, xb, c])
        top, bot = a * (256 - fx) + b * fx, cc * (256 - fx) + d * fx
        out.append((top * (256 - fy) + bot * fy + 32768) >> 16)
    return out


def rectify_ref(src, M, out_hw, fill=(0, 0, 0)):
    """[ho, wo, 3] uint8: the contract, pixel by pixel."""
    m = [float(v) for v in np.asarray(M, dtype=np.float64).reshape(9).astype(np.float32)]
    hs, ws = src.shape[:2]
    ho, wo = out_hw
    out = np.empty((ho, wo, 3), dtype=np.uint8)
    for i in range(ho):
        for j in range(wo):
            inside, U, V = positions(m, i, j, hs, ws)
            out[i, j] = blend(src, U, V) if inside else fill
    return out


# ------------------------------------------------------------------------------------------------ the cases
def source(hs, ws):
    """Random bytes: a tap that is one off changes almost every byte."""
    return np.random.default_rng(hs * 10007 + ws).integers(0, 256, (hs, ws, 3), dtype=np.uint8)


def matrices(hs, ws, ho, wo):
    """{name: 3 x 3} for one pair of sizes: identity, an integer shift, a half-pixel shift, 2x minification, 3x magnification and a
    true perspective map that keeps most of the output inside the source."""
    sx, sy = ws / wo, hs / ho
    return {
        "identity": [[1, 0, 0], [0, 1, 0], [0, 0, 1]],
        "shift": [[1, 0, 3], [0, 1, -2], [0, 0, 1]],
        "half": [[1, 0, 0.5], [0, 1, 0.5], [0, 0, 1]],
        "min2": [[2, 0, 0], [0, 2, 0], [0, 0, 1]],
        "mag3": [[1 / 3, 0, 0], [0, 1 / 3, 0], [0, 0, 1]],
        "perspective": [[0.9 * sx, 0.11 * ws / ho, 0.2], [-0.07 * hs / wo, 1.1 * sy, 0.3], [0.3 / wo, 0.5 / ho, 1]],
    }


def horizon(ho):
    """Z = 1 - 2 yo / ho changes sign in the middle of the output: the lower half is behind the camera."""
    return [[1, 0, 0], [0, 1, 0], [0, -2.0 / ho, 1]]


OUTSIDE = [[1, 0, 1e5], [0, 1, 1e5], [0, 0, 1]]            # the whole output lies outside the source
SHAPES = [((hs, ws), (ho, wo)) for hs, ws in ((5, 7), (33, 65)) for ho, wo in ((1, 1), (3, 5), (64, 67))] + \
    [((96, 300), (70, 260)), ((1, 1), (3, 5))]


def _cases():
    out = []
    for (hs, ws), (ho, wo) in SHAPES:
        for name, M in matrices(hs, ws, ho, wo).items():
            out.append((f"{hs}x{ws}-{ho}x{wo}-{name}", (hs, ws), (ho, wo), M, (0, 0, 0)))
    out.append(("33x65-64x67-horizon", (33, 65), (64, 67), horizon(64), (9, 8, 7)))
    out.append(("96x300-70x260-horizon", (96, 300), (70, 260), horizon(70), (0, 0, 0)))
    out.append(("33x65-64x67-outside", (33, 65), (64, 67), OUTSIDE, (1, 2, 3)))
    out.append(("33x65-64x67-fill", (33, 65), (64, 67), matrices(33, 65, 64, 67)["shift"], (255, 17, 128)))
    return out


CASES = _cases()                                           # (id, source (hs, ws), (ho, wo), M, fill)
CASE_IDS = [c[0] for c in CASES]


@functools.lru_cache(maxsize=None)
def reference(case_id):
    """The reference's output for a case, computed once per process and shared; callers must not write into it."""
    _, hw, out_hw, M, fill = CASES[CASE_IDS.index(case_id)]
    out = rectify_ref(source(*hw), M, out_hw, fill)
    out.setflags(write=False)
    return out
