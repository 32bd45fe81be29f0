"""Test-time augmentation and tiled inference."""

from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np
import torch

from ._capi import OreError, _chk, _ptr, _stream, lib


# ---------------------------------------------------------------------------------------------------
# test-time augmentation tail (csrc/ore_tta.hip): flipped variants, per-variant collection, the merge
# ---------------------------------------------------------------------------------------------------
TTA_MAX_CANDIDATES = 8192                                # rows one ore_tta_merge_fwd takes (include/ore_hip.h)


def tta_hflip_u8(img_chw_u8: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[3, nh, nw] uint8 planar device image with its columns reversed (img[:, :, ::-1]) -- the flipped TTA variant, a copy of the
    resized variant's bytes (ore_tta_hflip_u8_fwd).  Enqueued on the current stream."""
    assert img_chw_u8.is_cuda and img_chw_u8.dtype == torch.uint8 and img_chw_u8.dim() == 3 and img_chw_u8.is_contiguous(), \
        "tta_hflip_u8 takes a contiguous [c, h, w] uint8 device tensor"
    if out is None:
        out = torch.empty_like(img_chw_u8)
    assert out.is_cuda and out.dtype == torch.uint8 and out.shape == img_chw_u8.shape and out.is_contiguous()
    c, nh, nw = (int(v) for v in img_chw_u8.shape)
    with torch.cuda.device(img_chw_u8.device):
        _chk(lib().ore_tta_hflip_u8_fwd(_ptr(img_chw_u8), _ptr(out), c * nh, nw, _stream()), "ore_tta_hflip_u8_fwd")
    return out


class TTAPool:
    """Device buffers of one TTA merge: the candidate pool of `variants` x `rows` rows (boxes, scores, class ids), its running row
    count, the per-variant counts and the merge workspace."""

    def __init__(self, variants: int, rows: int, device):
        self.variants, self.rows, self.cap = int(variants), int(rows), int(variants) * int(rows)
        if not 1 <= self.cap <= TTA_MAX_CANDIDATES:
            raise OreError(f"TTAPool: {variants} variants x {rows} rows = {self.cap} candidates, one merge takes 1 .. {TTA_MAX_CANDIDATES}")
        dev = torch.device(device)
        self.boxes = torch.zeros(self.cap, 4, dtype=torch.float32, device=dev)
        self.scores = torch.zeros(self.cap, dtype=torch.float32, device=dev)
        self.classes = torch.zeros(self.cap, dtype=torch.int64, device=dev)
        self.n = torch.zeros(1, dtype=torch.int32, device=dev)
        self.var_counts = torch.zeros(self.variants, dtype=torch.int32, device=dev)
        self.ws_bytes = int(lib().ore_tta_merge_workspace_bytes(self.cap))
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=dev)


def tta_collect(pool: TTAPool, variant: int, boxes, scores, classes, n, max_rows: int, *, flip: bool, variant_w: int,
                sx: float, sy: float, pre: Optional[Tuple[float, float]] = None) -> None:
    """Append one variant's detection rows, inverse-transformed, to the pool (ore_tta_collect_fwd; no host sync).  boxes [.., 4] /
    scores / classes (int64, or None: all 0): device tensors whose rows are contiguous; n: an int32 device tensor holding the row count
    (read by the kernel) or a host int; at most max_rows rows are taken.  sx, sy (and pre = (px, py)) are the inverse resize ratios,
    computed in double by the caller and rounded to fp32 here."""
    n_dev, n_host = (_ptr(n), 0) if torch.is_tensor(n) else (None, int(n))
    px, py = pre if pre is not None else (1.0, 1.0)
    with torch.cuda.device(pool.boxes.device):
        _chk(lib().ore_tta_collect_fwd(_ptr(boxes), _ptr(scores), _ptr(classes), n_dev, n_host, int(max_rows), int(bool(flip)), int(variant_w),
                                       float(np.float32(sx)), float(np.float32(sy)), int(pre is not None), float(np.float32(px)),
                                       float(np.float32(py)), _ptr(pool.boxes), _ptr(pool.scores), _ptr(pool.classes), _ptr(pool.n), pool.cap,
                                       _ptr(pool.var_counts), int(variant), _stream()), "ore_tta_collect_fwd")


def tta_merge(pool: TTAPool, out_h: int, out_w: int, score_thresh: float, nms_thresh: float, topk: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """fast_rcnn_inference_single_image over the pool (ore_tta_merge_fwd; no host sync): returns (record, count) -- a fresh fp32 tensor
    laid out [R][4] boxes | [R] scores | [R] int64 classes with R = topk rounded up to even, and the int32 device count of its valid rows.
    `record_views(record, R, count)` cuts it."""
    R = int(topk) + (int(topk) & 1)
    dev = pool.boxes.device
    rec = torch.empty(R * 7, dtype=torch.float32, device=dev)
    cnt = torch.empty(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _chk(lib().ore_tta_merge_fwd(_ptr(pool.boxes), _ptr(pool.scores), _ptr(pool.classes), _ptr(pool.n), pool.cap, int(out_h), int(out_w),
                                     float(score_thresh), float(nms_thresh), int(topk), _ptr(rec), R, _ptr(cnt), _ptr(pool.ws), pool.ws_bytes,
                                     _stream()), "ore_tta_merge_fwd")
    return rec, cnt


def record_views(rec: torch.Tensor, R: int, k: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(boxes [k, 4], scores [k], classes [k] int64) of a result record of R rows (the layout of Engine.detect_end)."""
    return rec.as_strided((k, 4), (4, 1)), rec.as_strided((k,), (1,), R * 4), rec.view(torch.int64).as_strided((k,), (1,), R * 5 // 2)


# ---------------------------------------------------------------------------------------------------
# tiled inference (csrc/ore_tile.hip): the tile plan, the gather of every tile in one launch, the per-source collection with the seam
# rule.  tile_gather_u8 / tile_collect are the kernels, tile_gather_host / tile_collect_host the numpy statements of the same contracts.
# ---------------------------------------------------------------------------------------------------
TILE_MAX_SIDE, TILE_MAX_TILES = 8192, 128                # limits of ore_tile_gather_u8_fwd (include/ore_hip.h)
TILE_EDGE_LEFT, TILE_EDGE_TOP, TILE_EDGE_RIGHT, TILE_EDGE_BOTTOM = 1, 2, 4, 8


def _tile_axis(L: int, t: int, o: int) -> Tuple[int, int, int, List[int]]:
    """One axis of tile_plan: (extent, stride, count, starts)."""
    L, t, o = int(L), int(t), int(o)
    if L < 1 or t < 1 or not 0 <= o < t:
        raise ValueError(f"tile_plan: length {L} (>= 1), tile {t} (>= 1), overlap {o} (0 .. tile - 1)")
    e, s = min(t, L), t - o
    n = 1 if L <= t else -((t - L) // s) + 1             # ceil((L - t) / s) + 1
    return e, s, n, [min(k * s, L - e) for k in range(n)]


def tile_plan(h: int, w: int, tile_hw: Tuple[int, int], overlap_hw: Tuple[int, int]) -> dict:
    """The tiles of an [h, w] frame, pure integer: dict(th, tw, ny, nx, stride_y, stride_x, origins).  Per axis with length L, tile t
    and overlap o (0 <= o < t): the extent is min(t, L); L <= t gives one tile at 0; otherwise the stride is t - o, there are
    ceil((L - t) / stride) + 1 tiles and tile k starts at min(k * stride, L - extent) -- the last tile is flush with the far edge and
    nothing is ever padded.  All tiles have the same extent (th, tw); origins lists (y0, x0) row-major (iy * nx + ix)."""
    th, sy, ny, ys = _tile_axis(h, tile_hw[0], overlap_hw[0])
    tw, sx, nx, xs = _tile_axis(w, tile_hw[1], overlap_hw[1])
    return dict(th=th, tw=tw, ny=ny, nx=nx, stride_y=sy, stride_x=sx, origins=[(y, x) for y in ys for x in xs])


def tile_edges(plan: dict, index: int, h: int, w: int) -> int:
    """The `edges` bits of tile `index` of a plan over an [h, w] frame: a bit is set where the frame continues beyond the tile."""
    y0, x0 = plan["origins"][index]
    return (TILE_EDGE_LEFT if x0 > 0 else 0) | (TILE_EDGE_TOP if y0 > 0 else 0) | \
        (TILE_EDGE_RIGHT if x0 + plan["tw"] < w else 0) | (TILE_EDGE_BOTTOM if y0 + plan["th"] < h else 0)


def tile_gather_host(frame_hwc_u8, plan: dict, swap_rb: bool = False) -> np.ndarray:
    """The gather contract on the host: [ny * nx, 3, th, tw] uint8, tile i = frame[y0 : y0 + th, x0 : x0 + tw] of plan["origins"][i]
    transposed to planar, channels 0 and 2 exchanged with swap_rb."""
    frame = np.asarray(frame_hwc_u8)
    assert frame.dtype == np.uint8 and frame.ndim == 3 and frame.shape[2] == 3, "tile_gather_host takes an [h, w, 3] uint8 frame"
    th, tw = plan["th"], plan["tw"]
    out = np.stack([frame[y:y + th, x:x + tw].transpose(2, 0, 1) for y, x in plan["origins"]])
    return np.ascontiguousarray(out[:, ::-1] if swap_rb else out)


def tile_collect_host(boxes, scores, classes=None, *, sx: float, sy: float, ox: float, oy: float, src_hw: Tuple[int, int], edges: int,
                      margin: float):
    """The collect contract on the host, fp32 throughout: the seam rule on the source-local rows (a comparison with NaN is false, so
    such a row is kept), then x' = fl(fl(x * sx) + ox), y' = fl(fl(y * sy) + oy) on the kept rows, in row order.  Returns (boxes
    [k, 4] float32, scores [k] float32, classes [k] int64, kept: bool mask over the input rows)."""
    b = np.ascontiguousarray(boxes, dtype=np.float32).reshape(-1, 4)
    s = np.asarray(scores, dtype=np.float32).reshape(-1)
    c = np.zeros(len(s), dtype=np.int64) if classes is None else np.asarray(classes, dtype=np.int64).reshape(-1)
    m, edges = np.float32(margin), int(edges)
    x_hi, y_hi = np.float32(src_hw[1]) - m, np.float32(src_hw[0]) - m
    cut = np.zeros(len(s), dtype=bool)
    with np.errstate(all="ignore"):
        if edges & TILE_EDGE_LEFT:
            cut |= b[:, 0] < m
        if edges & TILE_EDGE_TOP:
            cut |= b[:, 1] < m
        if edges & TILE_EDGE_RIGHT:
            cut |= b[:, 2] > x_hi
        if edges & TILE_EDGE_BOTTOM:
            cut |= b[:, 3] > y_hi
        k = b[~cut]
        out = np.empty_like(k)
        out[:, 0::2] = k[:, 0::2] * np.float32(sx) + np.float32(ox)
        out[:, 1::2] = k[:, 1::2] * np.float32(sy) + np.float32(oy)
    return out, s[~cut], c[~cut], ~cut


class TilePool(TTAPool):
    """The merge pool of one tiled frame: a TTAPool of `sources` x `rows` candidates (ore_tta_merge_fwd reads it unchanged) with, per
    source, the rows appended (src_counts, the TTAPool's var_counts) and the rows the seam rule rejected (src_dropped)."""

    def __init__(self, sources: int, rows: int, device):
        super().__init__(sources, rows, device)
        self.sources, self.src_counts = self.variants, self.var_counts
        self.src_dropped = torch.zeros(self.sources, dtype=torch.int32, device=self.boxes.device)


def tile_gather_u8(frame_hwc_u8: torch.Tensor, plan: dict, swap_rb: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[h, w, 3] uint8 device frame (interleaved) -> [ny * nx, 3, th, tw] uint8 planar tiles of tile_plan(h, w, ...), byte for byte
    tile_gather_host, in one launch (ore_tile_gather_u8_fwd) on the current stream.  tiles[i] and tiles[i : i + B] are the images
    Engine.eval_forward / eval_forward_batch take."""
    assert frame_hwc_u8.is_cuda and frame_hwc_u8.dtype == torch.uint8 and frame_hwc_u8.dim() == 3 and frame_hwc_u8.shape[2] == 3 and \
        frame_hwc_u8.is_contiguous(), "tile_gather_u8 takes a contiguous [h, w, 3] uint8 device tensor"
    h, w = int(frame_hwc_u8.shape[0]), int(frame_hwc_u8.shape[1])
    n, th, tw = int(plan["ny"]) * int(plan["nx"]), int(plan["th"]), int(plan["tw"])
    dev = frame_hwc_u8.device
    if out is None:
        out = torch.empty(n, 3, th, tw, dtype=torch.uint8, device=dev)
    assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (n, 3, th, tw) and out.is_contiguous()
    with torch.cuda.device(dev):
        _chk(lib().ore_tile_gather_u8_fwd(_ptr(frame_hwc_u8), h, w, th, tw, int(plan["stride_y"]), int(plan["stride_x"]), int(plan["ny"]),
                                          int(plan["nx"]), int(bool(swap_rb)), _ptr(out), _stream()), "ore_tile_gather_u8_fwd")
    return out


def tile_collect(pool: TilePool, source: int, boxes, scores, classes, n, max_rows: int, *, sx: float, sy: float, ox: float, oy: float,
                 src_hw: Tuple[int, int], edges: int, margin: float) -> None:
    """Append one source's detection rows -- a tile's, or the full-frame pass's -- to the pool behind the seam rule and the transform
    of tile_collect_host (ore_tile_collect_fwd; no host sync).  boxes [.., 4] / scores / classes (int64, or None: all 0): device tensors
    whose rows are contiguous; n: an int32 device tensor holding the row count (read by the kernel) or a host int; at most max_rows
    rows are taken.  sx, sy, ox, oy and margin are rounded to fp32 here; source 0 restarts the pool."""
    n_dev, n_host = (_ptr(n), 0) if torch.is_tensor(n) else (None, int(n))
    with torch.cuda.device(pool.boxes.device):
        _chk(lib().ore_tile_collect_fwd(_ptr(boxes), _ptr(scores), _ptr(classes), n_dev, n_host, int(max_rows), float(np.float32(sx)),
                                        float(np.float32(sy)), float(np.float32(ox)), float(np.float32(oy)), int(src_hw[0]), int(src_hw[1]),
                                        int(edges), float(np.float32(margin)), _ptr(pool.boxes), _ptr(pool.scores), _ptr(pool.classes),
                                        _ptr(pool.n), pool.cap, _ptr(pool.src_counts), _ptr(pool.src_dropped), int(source), _stream()),
             "ore_tile_collect_fwd")
