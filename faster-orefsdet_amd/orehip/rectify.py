"""Rectification of oblique camera frames into the belt plane: the host statement of the contract "rectify v1", the launch, the
homography of an installation from four points, and Rectifier, which carries both and moves points and boxes between the two views."""

from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np
import torch

from ._capi import OreError, _chk, _ptr, _stream, lib


# ---------------------------------------------------------------------------------------------------
# Rectification (csrc/ore_rectify.hip; contract "rectify v1", include/ore_hip.h).  A camera that looks at the belt obliquely sees it in
# perspective: "belt shift v1" votes one translation for the whole frame and box sizes are read in pixels, and both hold only in a
# fronto-parallel view.  The camera is fixed, so one homography per installation warps every frame into the belt plane before anything
# else looks at it.  rectify_u8 is one launch, rectify_host the numpy statement of the same contract: both give the same bytes.
RECTIFY_MAX_SIDE = 16384                                   # ORE_RECTIFY_MAX_SIDE


def _rectify_m9(who: str, M) -> np.ndarray:
    """The nine coefficients as the fp32 the kernel takes, row-major; refused unless they are 9 finite numbers."""
    try:
        m = np.asarray(M.detach().cpu().numpy() if torch.is_tensor(M) else M, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        m = np.empty(0)
    if m.size != 9:
        raise ValueError(f"{who}: M is 9 numbers (3 x 3, row-major: output pixel -> source), got {M!r}")
    with np.errstate(over="ignore"):
        m32 = m.astype(np.float32)
    if not np.isfinite(m32).all():
        raise ValueError(f"{who}: M has a coefficient that is not finite as fp32: {m.tolist()}")
    return np.ascontiguousarray(m32)


def _rectify_hw(who: str, what: str, hw) -> Tuple[int, int]:
    try:
        h, w = hw
        ok = all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in (h, w))
    except (TypeError, ValueError):
        ok = False
    if not ok or not (1 <= h <= RECTIFY_MAX_SIDE and 1 <= w <= RECTIFY_MAX_SIDE):
        raise ValueError(f"{who}: {what} {hw!r} is (height, width), both 1 .. {RECTIFY_MAX_SIDE}")
    return int(h), int(w)


def _rectify_fill(who: str, fill) -> Tuple[int, int, int]:
    try:
        f = tuple(fill)
        ok = len(f) == 3 and all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) and 0 <= v <= 255 for v in f)
    except TypeError:
        ok = False
    if not ok:
        raise ValueError(f"{who}: fill {fill!r} is three bytes (0 .. 255) in the frame's channel order")
    return int(f[0]), int(f[1]), int(f[2])


def rectify_host(frame, M, out_hw, fill=(0, 0, 0)) -> np.ndarray:
    """The contract "rectify v1" (include/ore_hip.h) on the host, numpy fp32 one operation at a time and integers behind them: what
    ore_rectify_u8_fwd computes, bit for bit.  frame [hs, ws, 3] uint8 (array or host tensor), M the 3 x 3 map from output pixels to
    source coordinates, out_hw (ho, wo).  Returns [ho, wo, 3] uint8."""
    src = np.asarray(frame.detach().cpu().numpy() if torch.is_tensor(frame) else frame)
    if src.dtype != np.uint8 or src.ndim != 3 or src.shape[2] != 3:
        raise ValueError(f"rectify_host: the frame is [h, w, 3] uint8, got {src.dtype} {src.shape}")
    hs, ws = _rectify_hw("rectify_host", "the frame's size", (src.shape[0], src.shape[1]))
    ho, wo = _rectify_hw("rectify_host", "out_hw", out_hw)
    m = _rectify_m9("rectify_host", M)
    fill = _rectify_fill("rectify_host", fill)
    f32, half = np.float32, np.float32(0.5)
    out = np.empty((ho, wo, 3), dtype=np.uint8)
    out[:] = np.array(fill, dtype=np.uint8)
    xo = np.arange(wo, dtype=np.float32) + half
    s = src.astype(np.int32)
    for r0 in range(0, ho, 256):                                # 256 rows at a time: a 4K frame's temporaries stay small
        r1 = min(r0 + 256, ho)
        yo = (np.arange(r0, r1, dtype=np.float32) + half)[:, None]
        with np.errstate(all="ignore"):
            X = (m[0] * xo[None, :] + m[1] * yo) + m[2]
            Y = (m[3] * xo[None, :] + m[4] * yo) + m[5]
            Z = (m[6] * xo[None, :] + m[7] * yo) + m[8]
            u = X / Z - half
            v = Y / Z - half
            inside = np.isfinite(X) & np.isfinite(Y) & np.isfinite(Z) & (Z > 0) & (u >= -half) & (u <= f32(ws) - half) & (v >= -half) & \
                (v <= f32(hs) - half)
            U = np.floor(np.where(inside, u, f32(0)) * f32(256.0) + half).astype(np.int32)
            V = np.floor(np.where(inside, v, f32(0)) * f32(256.0) + half).astype(np.int32)
        x0, fx, y0, fy = U >> 8, (U & 255)[..., None], V >> 8, (V & 255)[..., None]
        xa, xb = np.clip(x0, 0, ws - 1), np.clip(x0 + 1, 0, ws - 1)
        ya, yb = np.clip(y0, 0, hs - 1), np.clip(y0 + 1, 0, hs - 1)
        top = s[ya, xa] * (256 - fx) + s[ya, xb] * fx
        bot = s[yb, xa] * (256 - fx) + s[yb, xb] * fx
        val = ((top * (256 - fy) + bot * fy + 32768) >> 16).astype(np.uint8)
        blk = out[r0:r1]
        blk[inside] = val[inside]
    return out


def rectify_u8(frame: torch.Tensor, M, out_hw, fill=(0, 0, 0), out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[hs, ws, 3] uint8 contiguous device tensor -> its rectified [ho, wo, 3] uint8 tensor, byte for byte rectify_host's: one launch on
    the current stream, no host synchronisation.  out: a (ho, wo, 3) uint8 contiguous tensor of the same device that does not alias
    the frame.  Everything is checked before anything is enqueued (ValueError; OreError from the library)."""
    if not torch.is_tensor(frame) or not frame.is_cuda:
        raise ValueError("rectify_u8: the frame is a device tensor (rectify_host takes host frames)")
    if frame.dtype != torch.uint8 or frame.dim() != 3 or frame.shape[2] != 3 or not frame.is_contiguous():
        raise ValueError(f"rectify_u8: the frame is a contiguous [h, w, 3] uint8 tensor, got {frame.dtype} {tuple(frame.shape)}")
    hs, ws = _rectify_hw("rectify_u8", "the frame's size", (int(frame.shape[0]), int(frame.shape[1])))
    ho, wo = _rectify_hw("rectify_u8", "out_hw", out_hw)
    m = _rectify_m9("rectify_u8", M)
    f = _rectify_fill("rectify_u8", fill)
    dev = frame.device
    if out is not None:
        if not torch.is_tensor(out) or out.device != dev or out.dtype != torch.uint8 or tuple(out.shape) != (ho, wo, 3) or not out.is_contiguous():
            raise ValueError(f"rectify_u8: out is a contiguous ({ho}, {wo}, 3) uint8 tensor on {dev}")
        a0, b0 = frame.data_ptr(), out.data_ptr()
        if a0 < b0 + out.numel() and b0 < a0 + frame.numel():
            raise ValueError("rectify_u8: out overlaps the frame")
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty(ho, wo, 3, dtype=torch.uint8, device=dev)
        m9 = (C.c_float * 9)(*m.tolist())
        _chk(lib().ore_rectify_u8_fwd(_ptr(frame), hs, ws, m9, _ptr(out), ho, wo, f[0] | f[1] << 8 | f[2] << 16, _stream()),
             "ore_rectify_u8_fwd")
    return out


def homography_from_quad(quad, out_hw) -> np.ndarray:
    """The 3 x 3 float64 matrix, m22 = 1, that maps the output rectangle's corners (0, 0), (wo, 0), (wo, ho), (0, ho) to the four source
    points quad [4][2] (x, y), in that order: the M of rectify_u8 for a belt whose corners were marked in a camera frame.  Refused
    (ValueError): a singular system (three points on a line, repeated points), or a quad that puts an output corner behind the camera
    (Z <= 0: a quad that is not convex, or whose points do not run round it)."""
    ho, wo = _rectify_hw("homography_from_quad", "out_hw", out_hw)
    try:
        q = np.asarray(quad, dtype=np.float64)
    except (TypeError, ValueError):
        q = np.empty(0)
    if q.shape != (4, 2) or not np.isfinite(q).all():
        raise ValueError(f"homography_from_quad: quad is four finite points (x, y), got {quad!r}")
    corners = np.array([[0, 0], [wo, 0], [wo, ho], [0, ho]], dtype=np.float64)
    A, b = np.zeros((8, 8)), np.zeros(8)
    for k, ((x, y), (u, v)) in enumerate(zip(corners, q)):
        A[2 * k] = (x, y, 1, 0, 0, 0, -u * x, -u * y)
        A[2 * k + 1] = (0, 0, 0, x, y, 1, -v * x, -v * y)
        b[2 * k], b[2 * k + 1] = u, v
    # scale the columns to unit size before judging the system: the corners are in pixels, the third column in ones
    scale = np.abs(A).max(0)
    scale[scale == 0] = 1.0
    try:
        if np.linalg.cond(A / scale) > 1e10:
            raise np.linalg.LinAlgError
        h = np.linalg.solve(A, b)
    except np.linalg.LinAlgError:
        raise ValueError(f"homography_from_quad: the quad {q.tolist()} is degenerate (the system is singular)") from None
    M = np.append(h, 1.0).reshape(3, 3)
    Z = corners @ M[2, :2] + 1.0
    if not np.isfinite(M).all() or not (Z > 0).all():
        raise ValueError(f"homography_from_quad: the quad {q.tolist()} puts an output corner behind the camera (Z = {Z.tolist()})")
    return M


def _apply_h(H: np.ndarray, points) -> np.ndarray:
    p = np.asarray(points.detach().cpu().numpy() if torch.is_tensor(points) else points, dtype=np.float64).reshape(-1, 2)
    with np.errstate(all="ignore"):
        x = p[:, 0] * H[0, 0] + p[:, 1] * H[0, 1] + H[0, 2]
        y = p[:, 0] * H[1, 0] + p[:, 1] * H[1, 1] + H[1, 2]
        z = p[:, 0] * H[2, 0] + p[:, 1] * H[2, 1] + H[2, 2]
        return np.stack([x / z, y / z], 1)


def _boxes_through(H: np.ndarray, boxes) -> np.ndarray:
    b = np.asarray(boxes.detach().cpu().numpy() if torch.is_tensor(boxes) else boxes, dtype=np.float64).reshape(-1, 4)
    corners = np.stack([b[:, [0, 1]], b[:, [2, 1]], b[:, [2, 3]], b[:, [0, 3]]], 1)        # [n, 4, 2]
    q = _apply_h(H, corners.reshape(-1, 2)).reshape(-1, 4, 2)
    return np.concatenate([q.min(1), q.max(1)], 1)


class Rectifier:
    """One installation's rectification: the homography and the output size, fixed with the camera.

        R = Rectifier(quad=[(560, 300), (1360, 300), (1900, 1000), (20, 1000)], out_hw=(720, 1280))   # or Rectifier(M, out_hw=...)
        flat = R(frame)                          # a device frame: rectify_u8, one launch; a host frame: rectify_host
        R.boxes_to_rectified(camera_boxes)       # annotations made in the camera view, moved into the belt plane

    quad: where the output rectangle's corners (0, 0), (wo, 0), (wo, ho), (0, ho) lie in the camera frame (homography_from_quad).  M maps
    output pixels to source coordinates; .M is its fp32 rounding, which is what the kernel takes and what the point maps use.  The warp
    has no anti-aliasing: keep out_hw near the belt region's resolution in the camera frame."""

    def __init__(self, M=None, *, quad=None, out_hw, fill=(0, 0, 0)):
        if (M is None) == (quad is None):
            raise ValueError("Rectifier: exactly one of M and quad")
        self.out_hw = _rectify_hw("Rectifier", "out_hw", out_hw)
        self.fill = _rectify_fill("Rectifier", fill)
        self.M = _rectify_m9("Rectifier", homography_from_quad(quad, self.out_hw) if M is None else M).reshape(3, 3)
        self._fwd = self.M.astype(np.float64)
        if abs(np.linalg.det(self._fwd)) < 1e-300 or not np.isfinite(np.linalg.cond(self._fwd)):
            raise ValueError(f"Rectifier: M is singular: {self._fwd.tolist()}")
        self._inv = np.linalg.inv(self._fwd)

    def __call__(self, frame, out: Optional[torch.Tensor] = None):
        if torch.is_tensor(frame) and frame.is_cuda:
            return rectify_u8(frame, self.M, self.out_hw, self.fill, out=out)
        res = rectify_host(frame, self.M, self.out_hw, self.fill)
        return torch.from_numpy(res) if torch.is_tensor(frame) else res

    def to_source(self, points) -> np.ndarray:
        """Points (x, y) of the rectified frame -> the camera frame: [n, 2] float64, continuous coordinates (a pixel's centre is at
        index + 0.5)."""
        return _apply_h(self._fwd, points)

    def to_rectified(self, points) -> np.ndarray:
        """Points (x, y) of the camera frame -> the rectified frame: [n, 2] float64."""
        return _apply_h(self._inv, points)

    def boxes_to_source(self, boxes) -> np.ndarray:
        """Boxes [n, 4] xyxy of the rectified frame -> the axis-aligned bounds of their four corners in the camera frame, float64."""
        return _boxes_through(self._fwd, boxes)

    def boxes_to_rectified(self, boxes) -> np.ndarray:
        """Boxes [n, 4] xyxy of the camera frame -> the axis-aligned bounds of their four corners in the rectified frame, float64."""
        return _boxes_through(self._inv, boxes)
