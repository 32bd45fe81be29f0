"""Heat maps of a detection pass: kernel wrappers and their numpy twins."""

from __future__ import annotations

import re
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from ._capi import OreError, _chk, _i32s, _ptr, _stream, lib
from .overlay import OVERLAY_MAX_SIDE, _overlay_table_dev


# ---------------------------------------------------------------------------------------------------
# Heat maps of a detection pass (render contract "heatmap v1", include/ore_hip.h)
HEATMAP_MEAN = -1                                          # ORE_HEATMAP_MEAN
HEATMAP_MAX_LEVELS, HEATMAP_MAX_MAP_SIDE, HEATMAP_MAX_INPUT_SIDE, HEATMAP_MAX_STRIDE = 3, 4096, 8192, 128
HEATMAP_LUTS = ("jet", "gray")
_HEATMAP_TRANSFORMS = {None: 0, "none": 0, "sigmoid": 1}
_HEATMAP_NORMS = {"unit": 0, "max": 1}
_HEATMAP_ALPHA_MODES = {"constant": 0, "value": 1}
# the level buffers every pass -- an N-way pass included -- leaves as a batch of `B` images per level (the laterals are not among
# them: an N-way pass computes them for its one image only)
_HEATMAP_LEVEL_BUFFERS = ("p", "attn", "pos", "tower", "head")
_HEATMAP_WS: Dict[tuple, torch.Tensor] = {}
_HEATMAP_WS_MAX = 16


def heatmap_lut(name_or_table="jet", channel_order: str = "RGB") -> np.ndarray:
    """The colour table of a heat map: [256, 3] uint8 in `channel_order`.  "gray": (k, k, k).  "jet": with t = k / 255 the classic
    r = clamp(1.5 - |4t - 3|), g = clamp(1.5 - |4t - 2|), b = clamp(1.5 - |4t - 1|), each floor(255 c + 0.5) -- the package's own
    table (255 c + 0.5 = 383 - |4k - 765| is an integer, so the table is integer arithmetic), not matplotlib's bytes.  Any [256, 3]
    uint8 table, taken as RGB, is accepted.  channel_order "BGR" reverses the channels."""
    if channel_order not in ("RGB", "BGR"):
        raise OreError(f'heatmap_lut: channel_order is "RGB" or "BGR", not {channel_order!r}')
    if isinstance(name_or_table, str):
        k = np.arange(256, dtype=np.int64)
        if name_or_table == "gray":
            tab = np.stack([k, k, k], 1)
        elif name_or_table == "jet":
            tab = np.stack([np.clip(383 - np.abs(4 * k - c), 0, 255) for c in (765, 510, 255)], 1)
        else:
            raise OreError(f"heatmap_lut: the built-in tables are {', '.join(HEATMAP_LUTS)}; not {name_or_table!r}")
        tab = tab.astype(np.uint8)
    else:
        tab = name_or_table.detach().cpu().numpy() if torch.is_tensor(name_or_table) else np.asarray(name_or_table)
        if tab.dtype != np.uint8 or tab.shape != (256, 3):
            raise OreError(f"heatmap_lut: a table is [256, 3] uint8, got {tab.shape} {tab.dtype}")
    return np.ascontiguousarray(tab[:, ::-1] if channel_order == "BGR" else tab)


def _heatmap_style(alpha, alpha_mode) -> Tuple[int, int]:
    if isinstance(alpha, bool) or not isinstance(alpha, (int, np.integer)) or not 0 <= int(alpha) <= 255:
        raise OreError(f"heatmap: alpha is an integer 0 .. 255, not {alpha!r}")
    if alpha_mode not in _HEATMAP_ALPHA_MODES:
        raise OreError(f'heatmap: alpha_mode is "constant" or "value", not {alpha_mode!r}')
    return int(alpha), _HEATMAP_ALPHA_MODES[alpha_mode]


def _heatmap_geometry(levels_hw, strides, in_hw) -> None:
    if not 1 <= len(levels_hw) <= HEATMAP_MAX_LEVELS or len(strides) != len(levels_hw):
        raise OreError(f"heatmap: 1 .. {HEATMAP_MAX_LEVELS} levels, one stride each; got {len(levels_hw)} levels, {len(strides)} strides")
    for (h, w), s in zip(levels_hw, strides):
        if not (1 <= h <= HEATMAP_MAX_MAP_SIDE and 1 <= w <= HEATMAP_MAX_MAP_SIDE and 1 <= s <= HEATMAP_MAX_STRIDE):
            raise OreError(f"heatmap: level {h}x{w} at stride {s}: map sides 1 .. {HEATMAP_MAX_MAP_SIDE}, strides 1 .. {HEATMAP_MAX_STRIDE}")
    if in_hw is not None and not (1 <= in_hw[0] <= HEATMAP_MAX_INPUT_SIDE and 1 <= in_hw[1] <= HEATMAP_MAX_INPUT_SIDE):
        raise OreError(f"heatmap: model input {in_hw[0]}x{in_hw[1]}: sides 1 .. {HEATMAP_MAX_INPUT_SIDE}")


def heat_kind(kind: str) -> dict:
    """A heat-map kind as its parts: {"buffers": names, "channel": int or "mean", "transform", "norm"}.  "objectness": head3 .. head5
    channel 4 through the sigmoid, norm "unit"; "attention": attn3 .. attn5, channel mean, norm "max"; "<buffer>" or
    "<buffer>:<channel>": one level buffer (p, attn, pos, tower, head + 3 .. 5), its mean or that channel, norm "max"."""
    if kind == "objectness":
        return {"buffers": ("head3", "head4", "head5"), "channel": 4, "transform": "sigmoid", "norm": "unit"}
    if kind == "attention":
        return {"buffers": ("attn3", "attn4", "attn5"), "channel": "mean", "transform": None, "norm": "max"}
    m = re.fullmatch(r"(%s)([345])(?::(\d+))?" % "|".join(_HEATMAP_LEVEL_BUFFERS), kind) if isinstance(kind, str) else None
    if m is None:
        raise OreError(f'heat map kind {kind!r}: "objectness", "attention", or a level buffer "<name><3 .. 5>[:<channel>]" with a name of '
                       f"{', '.join(_HEATMAP_LEVEL_BUFFERS)}")
    if m[1] == "head" and m[3] is None:
        raise OreError(f'heat map kind {kind!r}: the head rows are [l, t, r, b, hm]; name a channel ("{kind}:4")')
    return {"buffers": (m[1] + m[2],), "channel": "mean" if m[3] is None else int(m[3]), "transform": None, "norm": "max"}


class HeatSource:
    """Where a heat map's scalars live: 1 .. 3 level buffers on one device, and what to take from them.

    buffers: per level a contiguous 2-D device tensor [batch * h * w, ld], fp32 or bf16 (all alike); levels: per level (h, w, stride);
    the `ch` channels of a row start at element coff (an int, or one per level).  channel: an index below ch, or "mean" (ch, ld and coff
    multiples of 4); transform None or "sigmoid"; norm "unit" or "max"; in_hw: the model-input size the maps were computed at; slot:
    the image of the batch.  Engine.heat_source builds one over the engine's own buffers: it then also holds the engine and the serial
    of the pass it views, and check() raises once the engine has begun a newer pass."""

    def __init__(self, buffers, levels, *, ch: int, coff=0, channel="mean", transform=None, norm: str = "max", in_hw, batch: int = 1,
                 slot: int = 0, kind: Optional[str] = None):
        levels = [(int(h), int(w), int(s)) for h, w, s in levels]
        self.hw, self.strides = [(h, w) for h, w, _ in levels], [s for _, _, s in levels]
        self.in_hw = (int(in_hw[0]), int(in_hw[1]))
        _heatmap_geometry(self.hw, self.strides, self.in_hw)
        buffers = list(buffers)
        if len(buffers) != len(levels):
            raise OreError(f"HeatSource: {len(buffers)} buffers for {len(levels)} levels")
        self.batch, self.slot, self.ch, self.kind = int(batch), int(slot), int(ch), kind
        if self.batch < 1 or not 0 <= self.slot < self.batch:
            raise OreError(f"HeatSource: batch slot {slot} of {batch}")
        self.coff = [int(c) for c in coff] if isinstance(coff, (list, tuple)) else [int(coff)] * len(levels)
        first = buffers[0]
        for t, (h, w) in zip(buffers, self.hw):
            if not (torch.is_tensor(t) and t.is_cuda and t.dim() == 2 and t.is_contiguous() and t.dtype in (torch.float32, torch.bfloat16)
                    and t.dtype == first.dtype and t.device == first.device and t.shape[0] == self.batch * h * w):
                raise OreError("HeatSource: a level buffer is a contiguous [batch * h * w, ld] fp32 or bf16 device tensor, all of one type and device")
        self.device, self.is_bf16 = first.device, first.dtype == torch.bfloat16
        self.ptrs, self.ld, self._keep = [t.data_ptr() for t in buffers], [int(t.shape[1]) for t in buffers], buffers
        self.engine, self.serial = None, None
        self._set_what(channel, transform, norm)

    def _set_what(self, channel, transform, norm) -> None:
        if transform not in _HEATMAP_TRANSFORMS or norm not in _HEATMAP_NORMS:
            raise OreError(f'HeatSource: transform None or "sigmoid", norm "unit" or "max"; not {transform!r}, {norm!r}')
        self.transform, self.norm = transform, norm
        if channel == "mean":
            if self.ch % 4 or any(v % 4 for v in self.ld + self.coff):
                raise OreError(f"HeatSource: the channel mean takes ch, ld and coff that are multiples of 4 (ch {self.ch}, ld {self.ld}, coff {self.coff})")
            self.channel = HEATMAP_MEAN
        elif isinstance(channel, (int, np.integer)) and not isinstance(channel, bool) and 0 <= int(channel) < self.ch:
            self.channel = int(channel)
        else:
            raise OreError(f'HeatSource: channel {channel!r}: "mean" or an index below {self.ch}')
        if any(c < 0 or c + self.ch > ld for c, ld in zip(self.coff, self.ld)):
            raise OreError(f"HeatSource: {self.ch} channels at {self.coff} do not fit ld {self.ld}")

    def check(self) -> None:
        """Raises when the engine behind this source has begun a newer pass: its buffers no longer hold what the source was taken of."""
        if self.engine is not None and self.engine.last_geometry()["serial"] != self.serial:
            raise OreError(f"heat source {self.kind!r} is stale: the engine has begun a newer pass (take heat_source() again after it)")


class HeatLevels:
    """The quantised level maps of a HeatSource (heatmap_levels): .maps = per level an [h, w] uint8 device tensor, .strides, .in_hw.
    The maps are views of a workspace the current stream owns: the next heatmap_levels on that stream overwrites them (stream order
    protects a draw that was enqueued before); .clone() what must outlive it."""

    def __init__(self, maps, strides, in_hw, source=None):
        self.maps, self.strides, self.in_hw, self.source = list(maps), [int(s) for s in strides], (int(in_hw[0]), int(in_hw[1])), source

    def __len__(self):
        return len(self.maps)

    def __getitem__(self, i):
        return self.maps[i]

    def __iter__(self):
        return iter(self.maps)


def heatmap_levels(source: HeatSource) -> HeatLevels:
    """Stages A + B of the render contract on the device (ore_heatmap_levels_fwd): the scalar of every location of every level of the
    source, quantised to uint8 -- the reference's predhm_l windows.  One launch (norm "unit") or two ("max") on the current stream, no
    host sync; the workspace is cached per stream."""
    if not isinstance(source, HeatSource):
        raise OreError("heatmap_levels takes a HeatSource (Engine.heat_source, or one built over your own level buffers)")
    source.check()
    n, dev = len(source.hw), source.device
    hw = _i32s(v for pair in source.hw for v in pair)
    with torch.cuda.device(dev):
        need = int(lib().ore_heatmap_workspace_bytes(n, hw))
        if need == 0:
            raise OreError(f"heatmap_levels: level sizes {source.hw} are out of range")
        key = (str(dev), _stream())                                  # per stream: two streams' maps must not share a workspace
        ws = _HEATMAP_WS.get(key)
        if ws is None or ws.numel() < need:
            if torch.cuda.is_current_stream_capturing():
                raise OreError("heatmap_levels: no workspace for this stream yet; run once outside the stream capture first")
            while ws is None and len(_HEATMAP_WS) >= _HEATMAP_WS_MAX:
                _HEATMAP_WS.pop(next(iter(_HEATMAP_WS)))
            ws = _HEATMAP_WS[key] = torch.empty(max(need, 1 << 18), dtype=torch.uint8, device=dev)
        p = source.ptrs + [None] * (3 - n)
        _chk(lib().ore_heatmap_levels_fwd(n, p[0], p[1], p[2], hw, _i32s(source.ld), _i32s(source.coff), source.ch, int(source.is_bf16),
                                          source.batch, source.slot, source.channel, _HEATMAP_TRANSFORMS[source.transform],
                                          _HEATMAP_NORMS[source.norm], _ptr(ws), ws.numel(), _stream()), "ore_heatmap_levels_fwd")
        maps = []
        for l, (h, w) in enumerate(source.hw):
            off = int(lib().ore_heatmap_level_offset(n, hw, l))
            maps.append(ws[off:off + h * w].view(h, w))
    return HeatLevels(maps, source.strides, source.in_hw, source)


def _heatmap_levels_arg(levels, in_hw):
    """heatmap_draw's / heatmap_host's `levels` as (maps, strides, in_hw): a HeatLevels, or a sequence of (map, stride)."""
    if isinstance(levels, HeatLevels):
        maps, strides, in_hw = levels.maps, levels.strides, levels.in_hw if in_hw is None else in_hw
    else:
        try:
            pairs = [(m, int(s)) for m, s in levels]
        except (TypeError, ValueError):
            raise OreError("heatmap: levels is a HeatSource, a HeatLevels or a sequence of (uint8 map [h, w], stride)") from None
        maps, strides = [m for m, _ in pairs], [s for _, s in pairs]
    if in_hw is None:
        raise OreError("heatmap: in_hw, the model-input size the maps were computed at, is needed with bare maps")
    if not all(getattr(m, "ndim", 0) == 2 for m in maps):
        raise OreError("heatmap: a level map is [h, w] uint8")
    in_hw = (int(in_hw[0]), int(in_hw[1]))
    _heatmap_geometry([(int(m.shape[0]), int(m.shape[1])) for m in maps], strides, in_hw)
    return maps, strides, in_hw


def heatmap_draw(frame_hwc_u8: torch.Tensor, levels, in_hw=None, *, out: Optional[torch.Tensor] = None, lut="jet", alpha: int = 128,
                 alpha_mode: str = "constant", channel_order: str = "RGB") -> torch.Tensor:
    """A heat map blended over a contiguous [h, w, 3] uint8 device frame (ore_heatmap_draw_fwd; stages C + D of "heatmap v1"), enqueued
    on the current stream, no host sync.  levels: a HeatSource (its maps are computed first: heatmap_levels), a HeatLevels, or a
    sequence of (uint8 device map [h_l, w_l], stride) with in_hw = the model-input size they belong to.  lut: "jet", "gray" or a
    [256, 3] uint8 RGB table; channel_order: the frame's.  alpha_mode "constant" blends every pixel with alpha, "value" with
    (alpha * v + 127) / 255.  out=None returns a fresh frame, out=frame draws in place.  A source whose engine has begun a newer
    pass raises."""
    f = frame_hwc_u8
    if not (torch.is_tensor(f) and f.is_cuda and f.dtype == torch.uint8 and f.dim() == 3 and f.shape[2] == 3 and f.is_contiguous()):
        raise OreError("heatmap_draw takes a contiguous [h, w, 3] uint8 device tensor")
    h, w = int(f.shape[0]), int(f.shape[1])
    if not (1 <= h <= OVERLAY_MAX_SIDE and 1 <= w <= OVERLAY_MAX_SIDE):
        raise OreError(f"heatmap_draw: frame {h}x{w}: sides 1 .. {OVERLAY_MAX_SIDE}")
    a, mode = _heatmap_style(alpha, alpha_mode)
    table = heatmap_lut(lut, channel_order)
    if isinstance(levels, HeatSource):
        levels = heatmap_levels(levels)
    elif isinstance(levels, HeatLevels) and levels.source is not None:
        levels.source.check()
    maps, strides, in_hw = _heatmap_levels_arg(levels, in_hw)
    dev = f.device
    for m in maps:
        if not (torch.is_tensor(m) and m.dtype == torch.uint8 and m.device == dev and m.is_contiguous()):
            raise OreError("heatmap_draw: a level map is a contiguous [h, w] uint8 tensor on the frame's device")
    if out is None:
        out = torch.empty_like(f)
    if not (out.is_cuda and out.dtype == torch.uint8 and out.shape == f.shape and out.is_contiguous() and out.device == dev):
        raise OreError("heatmap_draw: out is a contiguous uint8 device tensor of the frame's shape")
    with torch.cuda.device(dev):
        lut_d = _overlay_table_dev(dev, ("heatmap_lut", table.tobytes()), lambda: table)
        p = [_ptr(m) for m in maps] + [None] * (3 - len(maps))
        _chk(lib().ore_heatmap_draw_fwd(_ptr(f), _ptr(out), h, w, len(maps), p[0], p[1], p[2],
                                        _i32s(int(v) for m in maps for v in m.shape), _i32s(strides), in_hw[0], in_hw[1], _ptr(lut_d), a, mode,
                                        _stream()), "ore_heatmap_draw_fwd")
    return out


def sigmoid_host(x) -> np.ndarray:
    """ore_sigmoid of the kernels on the host, operation by operation (ore_sigmoid_host): fp32 in, fp32 out, the input's shape."""
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float32))
    y = np.empty_like(x)
    _chk(lib().ore_sigmoid_host(x.ctypes.data, y.ctypes.data, x.size), "ore_sigmoid_host")
    return y


def heatmap_levels_host(values, *, channel="mean", transform=None, norm: str = "max") -> List[np.ndarray]:
    """heatmap_levels on the host: values = per level an [h, w, ch] fp32 array (bf16 widened by the caller) -> per level [h, w] uint8.
    The channel mean keeps the kernel's order: four partial sums over c % 4 == j, ascending, (s0 + s1) + (s2 + s3), / ch."""
    if transform not in _HEATMAP_TRANSFORMS or norm not in _HEATMAP_NORMS:
        raise OreError(f'heatmap_levels_host: transform None or "sigmoid", norm "unit" or "max"; not {transform!r}, {norm!r}')
    scal = []
    with np.errstate(all="ignore"):
        for v in values:
            v = np.asarray(v, dtype=np.float32)
            if v.ndim != 3:
                raise OreError("heatmap_levels_host: a level is [h, w, ch] fp32")
            ch = v.shape[2]
            if channel == "mean":
                if ch % 4:
                    raise OreError(f"heatmap_levels_host: the channel mean takes a channel count that is a multiple of 4, not {ch}")
                s = np.zeros(v.shape[:2] + (4,), dtype=np.float32)
                for c in range(0, ch, 4):
                    s = s + v[:, :, c:c + 4]
                x = ((s[..., 0] + s[..., 1]) + (s[..., 2] + s[..., 3])) / np.float32(ch)
            elif isinstance(channel, (int, np.integer)) and not isinstance(channel, bool) and 0 <= int(channel) < ch:
                x = v[:, :, int(channel)]
            else:
                raise OreError(f'heatmap_levels_host: channel {channel!r}: "mean" or an index below {ch}')
            scal.append(sigmoid_host(x) if _HEATMAP_TRANSFORMS[transform] else np.ascontiguousarray(x))
        quant = lambda x: (np.fmin(np.fmax(x, np.float32(0)), np.float32(1)) * np.float32(255)).astype(np.int32).astype(np.uint8)
        if norm == "unit":
            return [quant(x) for x in scal]
        m = np.float32(max([np.float32(0)] + [np.fmax(x, np.float32(0)).max() for x in scal if x.size]))
        if not m > 0:
            return [np.zeros(x.shape, dtype=np.uint8) for x in scal]
        return [quant(x / m) for x in scal]


def _heatmap_taps(n_out: int, n_in: int, stride: int, length: int):
    """One axis of stage C, every output coordinate at once: (i0, i1, frac)."""
    t = np.arange(n_out, dtype=np.int64)
    u = np.clip(((2 * t + 1) * n_in * 256) // (2 * n_out * stride) - 128, 0, (length - 1) * 256)
    i0 = u >> 8
    return i0, np.minimum(i0 + 1, length - 1), u & 255


def heatmap_host(frame_hwc_u8, levels, in_hw=None, *, out=None, lut="jet", alpha: int = 128, alpha_mode: str = "constant",
                 channel_order: str = "RGB") -> np.ndarray:
    """heatmap_draw on the host: the vectorised numpy statement of stages C + D of "heatmap v1" (include/ore_hip.h), byte for byte
    what the kernel draws.  levels: a sequence of (uint8 map [h_l, w_l], stride) -- numpy arrays or CPU tensors -- with in_hw, or a
    HeatLevels (its maps are copied to the host).  Returns an [h, w, 3] uint8 array: a fresh one, or `out` (the frame itself: in place)."""
    as_np = lambda t: t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    frame = as_np(frame_hwc_u8)
    if frame.dtype != np.uint8 or frame.ndim != 3 or frame.shape[2] != 3:
        raise OreError(f"heatmap_host takes an [h, w, 3] uint8 frame, got {frame.shape} {frame.dtype}")
    h, w = frame.shape[:2]
    if not (1 <= h <= OVERLAY_MAX_SIDE and 1 <= w <= OVERLAY_MAX_SIDE):
        raise OreError(f"heatmap_host: frame {h}x{w}: sides 1 .. {OVERLAY_MAX_SIDE}")
    a, mode = _heatmap_style(alpha, alpha_mode)
    table = heatmap_lut(lut, channel_order).astype(np.int64)
    maps, strides, in_hw = _heatmap_levels_arg(levels, in_hw)
    maps = [as_np(m) for m in maps]
    if any(m.dtype != np.uint8 for m in maps):
        raise OreError("heatmap_host: a level map is [h, w] uint8")
    v = np.zeros((h, w), dtype=np.int64)
    for m, s in zip(maps, strides):
        q = m.astype(np.int64)
        y0, y1, fy = _heatmap_taps(h, in_hw[0], s, m.shape[0])
        x0, x1, fx = _heatmap_taps(w, in_hw[1], s, m.shape[1])
        top = q[y0][:, x0] * (256 - fx) + q[y0][:, x1] * fx
        bot = q[y1][:, x0] * (256 - fx) + q[y1][:, x1] * fx
        v = np.maximum(v, (top * (256 - fy)[:, None] + bot * fy[:, None] + 32768) >> 16)
    A = ((a * v + 127) // 255 if mode else np.full_like(v, a))[..., None]
    res = ((frame.astype(np.int64) * (255 - A) + table[v] * A + 127) // 255).astype(np.uint8)
    if out is None:
        return res
    img = out if out is frame_hwc_u8 or out is frame else as_np(out)
    img[...] = res
    return img
