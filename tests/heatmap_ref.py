"""Reference of the heat-map render contract "heatmap v1" (include/ore_hip.h): a second, slow and obvious statement, independent of
orehip.heatmap_host / heatmap_levels_host.  Stage A + B walk the locations one by one with numpy fp32 scalars; stage C computes every
tap position with Python integers (exact at any size), one axis at a time -- U depends on x alone and V on y alone --; stage D is
integer arithmetic on int64 arrays.  The jet table comes from exact fractions.  Only the sigmoid is shared with the package, as the
contract names it: ore_sigmoid_host, the host twin of the kernels' ore_sigmoid (tests/test_heatmap_host.py pins it to the oracle)."""
import functools
from fractions import Fraction

import numpy as np


def jet_table():
    """[256, 3] uint8 RGB: t = k / 255, r = clamp(1.5 - |4t - 3|), g = clamp(1.5 - |4t - 2|), b = clamp(1.5 - |4t - 1|), each
    floor(255 c + 0.5), in exact rational arithmetic."""
    tab = np.zeros((256, 3), np.uint8)
    for k in range(256):
        t = Fraction(k, 255)
        for c, centre in enumerate((3, 2, 1)):
            v = min(max(Fraction(3, 2) - abs(4 * t - centre), Fraction(0)), Fraction(1))
            tab[k, c] = (255 * v + Fraction(1, 2)).__floor__()
    return tab


def gray_table():
    return np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)


def table(lut, channel_order="RGB"):
    tab = {"jet": jet_table, "gray": gray_table}[lut]() if isinstance(lut, str) else np.asarray(lut)
    return tab[:, ::-1] if channel_order == "BGR" else tab


def _sigmoid(x):
    import orehip
    return orehip.sigmoid_host(np.float32(x).reshape(1))[0]


def scalar_of(row, channel):
    """Stage A of one location: row = its `ch` values, fp32."""
    if channel != "mean":
        return np.float32(row[channel])
    s = [np.float32(0)] * 4
    for c in range(len(row)):                                  # ascending: partial sum c % 4 takes channel c
        s[c % 4] = np.float32(s[c % 4] + np.float32(row[c]))
    return np.float32(np.float32(np.float32(s[0] + s[1]) + np.float32(s[2] + s[3])) / np.float32(len(row)))


def quantise(v):
    """(int)(fminf(fmaxf(v, 0), 1) * 255.0f); NaN -> 0."""
    v = np.float32(v)
    if not v > 0:                                               # NaN, negatives, zeros
        return 0
    return int(np.float32(min(v, np.float32(1)) * np.float32(255)))


def levels_ref(values, channel="mean", transform=None, norm="max"):
    """Stages A + B: values = per level an [h, w, ch] fp32 array -> per level an [h, w] uint8 map."""
    with np.errstate(all="ignore"):
        scal = []
        for v in values:
            v = np.asarray(v, dtype=np.float32)
            s = np.zeros(v.shape[:2], np.float32)
            for i in range(v.shape[0]):
                for j in range(v.shape[1]):
                    x = scalar_of(v[i, j], channel)
                    s[i, j] = _sigmoid(x) if transform == "sigmoid" else x
            scal.append(s)
        if norm == "max":
            m = np.float32(0)
            for s in scal:
                for x in s.reshape(-1):
                    if x > m:                                   # NaN never is
                        m = x
        out = []
        for s in scal:
            q = np.zeros(s.shape, np.uint8)
            for i in range(s.shape[0]):
                for j in range(s.shape[1]):
                    if norm == "unit":
                        q[i, j] = quantise(s[i, j])
                    elif m > 0:
                        q[i, j] = quantise(np.float32(s[i, j] / m))
            out.append(q)
    return out


def taps(n_out, n_in, stride, length):
    """Per output coordinate t: (i0, i1, f) of U = floor(((2t + 1) * n_in * 256) / (2 * n_out * stride)) - 128 in [0, (length - 1) * 256]."""
    i0, i1, f = [], [], []
    for t in range(n_out):
        u = ((2 * t + 1) * n_in * 256) // (2 * n_out * stride) - 128
        u = min(max(u, 0), (length - 1) * 256)
        i0.append(u >> 8)
        i1.append(min((u >> 8) + 1, length - 1))
        f.append(u & 255)
    return np.array(i0), np.array(i1), np.array(f, dtype=np.int64)


def merged_ref(h, w, maps, strides, in_hw):
    """Stage C: the [h, w] int64 array of v = max over the levels of val_l."""
    v = np.zeros((h, w), np.int64)
    for q, s in zip(maps, strides):
        q = np.asarray(q).astype(np.int64)
        y0, y1, fy = taps(h, in_hw[0], s, q.shape[0])
        x0, x1, fx = taps(w, in_hw[1], s, q.shape[1])
        fx, fy = fx[None, :], fy[:, None]
        top = q[np.ix_(y0, x0)] * (256 - fx) + q[np.ix_(y0, x1)] * fx
        bot = q[np.ix_(y1, x0)] * (256 - fx) + q[np.ix_(y1, x1)] * fx
        v = np.maximum(v, (top * (256 - fy) + bot * fy + 32768) >> 16)
    return v


def heatmap_ref(frame, maps, strides, in_hw, *, lut="jet", alpha=128, alpha_mode="constant", channel_order="RGB"):
    """frame [h, w, 3] uint8 -> the drawn frame (a new array).  maps: per level [h_l, w_l] uint8; lut: "jet", "gray" or a [256, 3]
    uint8 RGB table."""
    frame = np.asarray(frame)
    h, w = frame.shape[:2]
    v = merged_ref(h, w, maps, strides, in_hw)
    col = table(lut, channel_order).astype(np.int64)[v]
    A = np.full((h, w), int(alpha), np.int64) if alpha_mode == "constant" else (int(alpha) * v + 127) // 255
    A = A[..., None]
    return ((frame.astype(np.int64) * (255 - A) + col * A + 127) // 255).astype(np.uint8)


# ---------------------------------------------------------------------------------------------- the cases both test files share
IN_HW = (40, 56)
STRIDES = (8, 16, 32)
LEVEL_HW = ((5, 7), (3, 4), (2, 2))
FRAMES = [(37, 53), (6, 9), (75, 100), (1, 1), (40, 3), (3, 1030), (480, 640)]


def frame(h, w, seed=0):
    return np.random.default_rng(seed * 7919 + h * 131 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def level_maps(seed=0):
    """Three uint8 maps (5x7, 3x4, 2x2) with both extremes present."""
    rng = np.random.default_rng(seed)
    maps = [rng.integers(0, 256, hw, dtype=np.uint8) for hw in LEVEL_HW]
    maps[0][0, 0], maps[0][4, 6], maps[1][1, 1], maps[2][1, 0] = 255, 0, 255, 0
    for m in maps:
        m.setflags(write=False)
    return tuple(maps)


RANDOM_LUT = np.random.default_rng(99).integers(0, 256, (256, 3), dtype=np.uint8)
RANDOM_LUT.setflags(write=False)
STYLES = [dict(lut="jet", alpha=128, alpha_mode="constant"), dict(lut="gray", alpha=178, alpha_mode="constant"),
          dict(lut="jet", alpha=255, alpha_mode="value"), dict(lut=RANDOM_LUT, alpha=128, alpha_mode="value"),
          dict(lut="gray", alpha=0, alpha_mode="constant"), dict(lut=RANDOM_LUT, alpha=255, alpha_mode="constant"),
          dict(lut="jet", alpha=0, alpha_mode="value")]


def _key(style):
    return tuple((k, v if isinstance(v, (str, int)) else "random") for k, v in sorted(style.items()))


_RENDER = {}


def render_case(hw, style_index=0, n_levels=3, in_hw=IN_HW):
    """(frame, maps, strides, in_hw, style, reference picture) -- computed once, shared by the host and the device tests."""
    key = (hw, style_index, n_levels, in_hw)
    if key not in _RENDER:
        img = frame(*hw, seed=style_index)
        img.setflags(write=False)
        maps, strides, style = level_maps()[:n_levels], STRIDES[:n_levels], STYLES[style_index]
        want = heatmap_ref(img, maps, strides, in_hw, **style)
        want.setflags(write=False)
        _RENDER[key] = (img, maps, strides, in_hw, style, want)
    return _RENDER[key]


def quantise_values(seed, hw, ch, special=True):
    """[h, w, ch] fp32 values around 0 .. 1 with 0, 1, > 1, negatives, NaN and both infinities sprinkled in."""
    rng = np.random.default_rng(seed)
    v = rng.normal(0.4, 0.5, hw + (ch,)).astype(np.float32)
    if special:
        flat = v.reshape(-1)
        for k, x in enumerate((0.0, 1.0, 1.5, -0.25, np.nan, np.inf, -np.inf, -0.0, 0.999999, 1e-30)):
            flat[(k * 37 + 5) % flat.size] = x
    return v


def bf16_round(v):
    """fp32 -> the nearest bf16 (ties to even), as fp32."""
    b = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32).astype(np.uint64)
    nan = np.isnan(v)
    b = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    out = b.astype(np.uint32).view(np.float32).copy()
    out[nan] = np.nan
    return out


def straddle_logits():
    """For k = 1 .. 255 the fp32 logit of k / 255 and its +-1, +-2 ulp neighbours: where the sigmoid crosses a quantisation step."""
    out = []
    for k in range(1, 255):
        p = k / 255.0
        bits = int(np.float32(np.log(p / (1.0 - p))).view(np.uint32))
        out += [np.uint32(bits + d).view(np.float32) for d in (-2, -1, 0, 1, 2)]
    # k = 255: the logit of 1 is +inf (its upper neighbours are NaNs: those are test_quantise's); below it the largest floats, and
    # the neighbourhood where the fp32 sigmoid first rounds to 1.0
    inf_bits = int(np.float32(np.inf).view(np.uint32))
    out += [np.uint32(inf_bits + d).view(np.float32) for d in (-2, -1, 0)]
    for x in (16.0, 16.5, 17.0, 17.5):
        bits = int(np.float32(x).view(np.uint32))
        out += [np.uint32(bits + d).view(np.float32) for d in (-2, -1, 0, 1, 2)]
    return np.array(out, dtype=np.float32)
