"""The belt's shift in front of the trackers: the host statement of the contract "belt shift v1" and both belt trackers."""

from __future__ import annotations

import math

import numpy as np
import torch

from ._capi import OreError, _chk, _ptr, lib
from .track import TRACK_WIDE_MAX_ROWS, BoxTracker, WideBoxTracker, track_state_empty


# ---------------------------------------------------------------------------------------------------
# The belt's shift (csrc/ore_belt.hip; contract "belt shift v1", include/ore_hip.h).  "track v1" matches a row to a track's last observed
# box, which holds while the scene moves less than a quarter of a box per frame; a belt moves rigidly and faster.  The one translation the
# frame shares is voted from the boxes and every track box is moved by it before the update.  BeltTracker / WideBeltTracker hold the
# belt state and run the kernels, belt_shift_host is the numpy statement of the same contract: both give the same two states.
BELT_MAX_HALF_BINS = 64                                    # ORE_BELT_MAX_HALF_BINS
BELT_BINS = (1, 2, 4, 8, 16)
BELT_DEFAULTS = {"bin": 2, "radius": 128, "size_tol": 0.125, "min_votes": 3, "frame": None}
_BELT_STATE_BYTES = 64                                     # int32 dx, dy, votes, reserved; int64 travel_x, travel_y, frames, coasted; zeros
_BELT_KEYS = ("dx", "dy", "votes", "travel_x", "travel_y", "frames", "coasted")


def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _belt_contract(who: str, bin, half_bins, size_tol, min_votes, frame_h, frame_w) -> dict:
    """The contract's parameters, checked against the limits of ore_belt_shift_fwd; size_tol as the fp32 the kernel takes."""
    if not _is_int(bin) or int(bin) not in BELT_BINS:
        raise OreError(f"{who}: bin {bin!r} (one of {BELT_BINS})")
    if not _is_int(half_bins) or not 1 <= half_bins <= BELT_MAX_HALF_BINS:
        raise OreError(f"{who}: half_bins {half_bins!r} (1 .. {BELT_MAX_HALF_BINS})")
    with np.errstate(over="ignore"):
        tol = np.float32(size_tol)
    if not (np.isfinite(tol) and 0 <= tol < 1):
        raise OreError(f"{who}: size_tol {size_tol!r} is finite, >= 0 and < 1")
    if not _is_int(min_votes) or not 1 <= min_votes <= 1 << 30:
        raise OreError(f"{who}: min_votes {min_votes!r} (1 .. {1 << 30})")
    if not (_is_int(frame_h) and _is_int(frame_w)) or frame_h < 0 or frame_w < 0 or (frame_h > 0) != (frame_w > 0) or max(frame_h, frame_w) >= 1 << 31:
        raise OreError(f"{who}: frame {frame_h!r} x {frame_w!r} (both 0: no frame test, or both > 0)")
    return {"bin": int(bin), "half_bins": int(half_bins), "size_tol": tol, "min_votes": int(min_votes), "frame_h": int(frame_h),
            "frame_w": int(frame_w)}


def _belt_params(who: str, bin, radius, size_tol, min_votes, frame) -> dict:
    """The keywords of a belt tracker as the contract's parameters: half_bins = ceil(radius / bin), frame None or (h, w)."""
    if not _is_int(bin) or int(bin) not in BELT_BINS:
        raise OreError(f"{who}: bin {bin!r} (one of {BELT_BINS})")
    if isinstance(radius, bool) or not isinstance(radius, (int, float, np.integer, np.floating)) or not radius > 0 or not math.isfinite(radius):
        raise OreError(f"{who}: radius {radius!r} is a positive number of pixels")
    half_bins = int(math.ceil(radius / int(bin)))
    if half_bins > BELT_MAX_HALF_BINS:
        raise OreError(f"{who}: radius {radius!r} at bin {bin} needs {half_bins} bins a side (at most {BELT_MAX_HALF_BINS}): use a larger bin")
    fh = fw = 0
    if frame is not None:
        try:
            fh, fw = frame
        except (TypeError, ValueError):
            fh = None
        if not (_is_int(fh) and _is_int(fw)) or fh < 1 or fw < 1:
            raise OreError(f"{who}: frame {frame!r} is None or (height, width), both at least 1")
    return _belt_contract(who, bin, half_bins, size_tol, min_votes, int(fh), int(fw))


def belt_state_empty() -> dict:
    """The state of a belt that has seen no frame: the shift (dx, dy) and its votes, the travel, the frames and those coasted."""
    return {k: 0 for k in _BELT_KEYS}


def belt_shift_host(state, belt, boxes, scores, classes=None, n=None, *, bin: int = 2, half_bins: int = 64, size_tol: float = 0.125,
                    min_votes: int = 3, frame_h: int = 0, frame_w: int = 0, score_thresh: float = 0.0, class_aware: bool = True):
    """One shift of the contract "belt shift v1" (include/ore_hip.h) on the host, numpy fp32 one operation at a time: what
    ore_belt_shift_fwd computes, bit for bit, in either form.  state: a track_host state (None: the empty one), belt: a belt_state_empty
    dict (None: the empty one); the rows as track_host takes them.  Returns (the track state with its boxes moved and the ttl of the
    tracks outside the frame set to 1, the new belt state); both arguments are left as they were."""
    as_np = lambda t: t.detach().cpu().numpy() if torch.is_tensor(t) else (None if t is None else np.asarray(t))
    p = _belt_contract("belt_shift_host", bin, half_bins, size_tol, min_votes, frame_h, frame_w)
    with np.errstate(over="ignore"):
        thr = np.float32(score_thresh)
    if np.isnan(thr):
        raise OreError("belt_shift_host: score_thresh is NaN")
    st = track_state_empty() if state is None else state
    old = belt_state_empty() if belt is None else belt
    m = int(st["m"])
    tb = np.array(np.asarray(as_np(st["boxes"]), dtype=np.float32).reshape(-1, 4)[:m])
    tc = np.asarray(as_np(st["classes"])).reshape(-1)[:m].astype(np.int64)
    tt = np.array(np.asarray(as_np(st["ttl"])).reshape(-1)[:m], dtype=np.int32)
    b = np.ascontiguousarray(np.asarray(as_np(boxes), dtype=np.float32)).reshape(-1, 4)
    s = np.asarray(as_np(scores), dtype=np.float32).reshape(-1)
    rows = len(s)
    if rows > TRACK_WIDE_MAX_ROWS or len(b) != rows:
        raise OreError(f"belt_shift_host: {len(b)} boxes, {rows} scores (at most {TRACK_WIDE_MAX_ROWS} rows)")
    c = np.zeros(rows, dtype=np.int64) if classes is None else np.asarray(as_np(classes), dtype=np.int64).reshape(-1)
    n = rows if n is None else min(max(int(n), 0), rows)
    K, bn, tol = p["half_bins"], p["bin"], p["size_tol"]
    W = 2 * K + 1
    inv, half, fk = np.float32(1.0 / (2 * bn)), np.float32(0.5), np.float32(K)
    H = np.zeros(W * W, dtype=np.int64)
    with np.errstate(all="ignore"):
        live = (np.arange(rows) < n) & np.isfinite(b).all(1) & np.isfinite(s) & (s >= thr)
        wd, hd, sxd, syd = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1], b[:, 0] + b[:, 2], b[:, 1] + b[:, 3]
        wt, ht, sxt, syt = tb[:, 2] - tb[:, 0], tb[:, 3] - tb[:, 1], tb[:, 0] + tb[:, 2], tb[:, 1] + tb[:, 3]
        row_ok = live & (wd > 0) & (hd > 0)
        for t0 in range(0, m, 1024):                            # [1024, rows] at a time: the limits would not fit as one array
            t1 = min(t0 + 1024, m)
            T = slice(t0, t1)
            ok = row_ok[None, :] & ((wt[T] > 0) & (ht[T] > 0))[:, None]
            if class_aware:
                ok &= tc[T, None] == c[None, :]
            ok &= np.abs(wt[T, None] - wd[None, :]) <= tol * np.maximum(wt[T, None], wd[None, :])
            ok &= np.abs(ht[T, None] - hd[None, :]) <= tol * np.maximum(ht[T, None], hd[None, :])
            qx = np.floor((sxd[None, :] - sxt[T, None]) * inv + half)
            qy = np.floor((syd[None, :] - syt[T, None]) * inv + half)
            ok &= (np.abs(qx) <= fk) & (np.abs(qy) <= fk)
            idx = (qy[ok].astype(np.int64) + K) * W + (qx[ok].astype(np.int64) + K)
            H += np.bincount(idx, minlength=W * W)
    H = H.reshape(W, W)
    pad = np.zeros((W + 2, W + 2), dtype=np.int64)
    pad[1:-1, 1:-1] = H
    S = sum(pad[1 + v:1 + v + W, 1 + u:1 + u + W] for v in (-1, 0, 1) for u in (-1, 0, 1))
    q = np.arange(-K, K + 1, dtype=np.int64) * bn
    dist = np.abs(q[None, :] - int(old["dx"])) + np.abs(q[:, None] - int(old["dy"]))
    best = int(S.max())
    cand = np.nonzero((S == best).reshape(-1))[0]               # ascending: qy, then qx
    peak = int(cand[np.argmin(dist.reshape(-1)[cand])])         # the first of the smallest distances
    new = {k: int(old[k]) for k in _BELT_KEYS}
    if best >= p["min_votes"]:
        new["dx"], new["dy"], new["votes"] = int(q[peak % W]), int(q[peak // W]), best
    else:
        new["votes"] = 0
        new["coasted"] += 1
    new["travel_x"] += new["dx"]
    new["travel_y"] += new["dy"]
    new["frames"] += 1
    with np.errstate(all="ignore"):
        dx, dy = np.float32(new["dx"]), np.float32(new["dy"])
        tb[:, 0] += dx
        tb[:, 2] += dx
        tb[:, 1] += dy
        tb[:, 3] += dy
        if p["frame_h"] > 0:
            gone = (tb[:, 2] <= 0) | (tb[:, 0] >= np.float32(p["frame_w"])) | (tb[:, 3] <= 0) | (tb[:, 1] >= np.float32(p["frame_h"]))
            tt[gone] = 1
    moved = dict(st)
    moved["boxes"], moved["ttl"] = tb, tt
    return moved, new


class _BeltShift:
    """What BeltTracker and WideBeltTracker add to their trackers: the belt state, the shift in front of every update, the extra
    statistics.  The base class calls _before_update / _before_host once every check of the rows has passed."""

    def __init__(self, device, *, bin: int = 2, radius=128, size_tol: float = 0.125, min_votes: int = 3, frame=None, **tracker_kw):
        self.belt_params = _belt_params(type(self).__name__, bin, radius, size_tol, min_votes, frame)
        self._belt, self._belt_ws, self._belt_ws_bytes, self._belt_host, self._belt_form = None, None, 0, None, 0
        super().__init__(device, **tracker_kw)                  # ends with reset(): both buffers
        if self._host is None:
            L, K = lib(), self.belt_params["half_bins"]
            self._belt_form = int(L.ore_belt_shift_form(self.capacity, self._row_limit(), K))
            if self._belt_form < 1:
                raise OreError(f"{type(self).__name__}: ore_belt_shift_form failed ({self._belt_form}): {L.ore_last_error().decode()}")
            if self._belt_form != 1:
                self._belt_ws_bytes = int(L.ore_belt_workspace_bytes(self.capacity, self._row_limit(), K))
                with torch.cuda.device(self.device):
                    self._belt_ws = torch.empty(max(self._belt_ws_bytes, 256), dtype=torch.uint8, device=self.device)

    def set_frame(self, frame) -> None:
        """The frame (height, width) beyond which a moved track is given up, or None: no frame test.  Takes effect with the next update."""
        p = self.belt_params
        fresh = _belt_params(type(self).__name__, p["bin"], p["half_bins"] * p["bin"], p["size_tol"], p["min_votes"], frame)
        p["frame_h"], p["frame_w"] = fresh["frame_h"], fresh["frame_w"]

    def _ordered(self) -> int:
        cur = super()._ordered()
        if self._belt is not None and self._event_stream is not None and self._event_stream != cur:
            here = torch.cuda.current_stream(self.device)
            self._belt.record_stream(here)
            if self._belt_ws is not None:
                self._belt_ws.record_stream(here)
        return cur

    def reset(self) -> None:
        """The empty track state and the empty belt state, enqueued on the current stream (device) like an update."""
        super().reset()
        if self._host is not None:
            self._belt_host = belt_state_empty()
            return
        with torch.cuda.device(self.device):
            if self._belt is None:
                self._belt = torch.empty(_BELT_STATE_BYTES, dtype=torch.uint8, device=self.device)
            cur = self._ordered()
            _chk(lib().ore_belt_reset(_ptr(self._belt), cur), "ore_belt_reset")
            self._updated(cur)

    def _contract_kw(self) -> dict:
        return dict(self.belt_params, score_thresh=self.params["score_thresh"], class_aware=self.params["class_aware"])

    def _before_host(self, boxes, scores, classes, n) -> None:
        limit = TRACK_WIDE_MAX_ROWS if self._host_kw.get("wide") else int(lib().ore_det_record_rows())
        if len(scores) > limit or len(boxes) != len(scores):    # what track_host refuses: before the tracks are moved
            raise OreError(f"{type(self).__name__}.update: {len(boxes)} boxes, {len(scores)} scores (at most {limit} rows)")
        self._host, self._belt_host = belt_shift_host(self._host, self._belt_host, boxes, scores, classes, n, **self._contract_kw())

    def _before_update(self, boxes, scores, classes, n_dev, n_host: int, rows: int, cur: int) -> None:
        p, t = self.belt_params, self.params
        _chk(lib().ore_belt_shift_fwd(_ptr(self._belt), _ptr(self._buf), self.capacity, _ptr(boxes) if rows else None,
                                      _ptr(scores) if rows else None, _ptr(classes) if rows else None, _ptr(n_dev), n_host, rows,
                                      float(t["score_thresh"]), int(t["class_aware"]), p["bin"], p["half_bins"], float(p["size_tol"]),
                                      p["min_votes"], p["frame_h"], p["frame_w"], 0, _ptr(self._belt_ws), self._belt_ws_bytes, cur),
             "ore_belt_shift_fwd")

    def belt_host(self) -> dict:
        """The belt state as belt_shift_host's dict; one explicit sync on a device."""
        if self._host is not None:
            return dict(self._belt_host)
        self._event.synchronize()
        raw = self._belt.cpu().numpy()
        dx, dy, votes = (int(v) for v in raw[:12].view(np.int32))
        tx, ty, frames, coasted = (int(v) for v in raw[16:48].view(np.int64))
        return {"dx": dx, "dy": dy, "votes": votes, "travel_x": tx, "travel_y": ty, "frames": frames, "coasted": coasted}

    def state_host(self) -> dict:
        """The tracker's state_host() and "belt": the belt state as belt_shift_host's dict."""
        out = super().state_host()
        out["belt"] = self.belt_host()
        return out

    def stats(self) -> dict:
        """The tracker's stats() and "shift": (dx, dy) of the last frame, "travel": (x, y) the belt's travel in pixels, "votes": the
        votes of the last accepted peak (0: the frame coasted), "coasted": the frames without an accepted peak."""
        out = super().stats()
        b = self.belt_host()
        out.update(shift=(b["dx"], b["dy"]), travel=(b["travel_x"], b["travel_y"]), votes=b["votes"], coasted=b["coasted"])
        return out


class BeltTracker(_BeltShift, BoxTracker):
    """BoxTracker for a scene that moves as one, a conveyor belt: before every update the frame's shift is voted from the boxes (contract
    "belt shift v1", include/ore_hip.h) and the tracks are moved by it, so ids persist at belt speeds where "track v1" alone starts every
    id afresh in every frame.

        tracker = BeltTracker(device, frame=(1080, 1920))  # bin=2, radius=128, size_tol=0.125, min_votes=3, and BoxTracker's keywords
        ids = tracker.update(boxes, scores, classes, n_dev)   # one more launch in front of the update, on the same stream; no sync
        tracker.stats()                                    # ... and "shift", "travel", "votes", "coasted"

    bin: pixels per histogram bin; radius: the largest shift per axis and frame in pixels (half_bins = ceil(radius / bin), at most 64);
    size_tol: how far two boxes' widths and heights may differ, relative to the larger, to vote; min_votes: the smoothed peak a shift
    needs, below it the belt coasts at its last shift; frame (height, width): a track moved wholly outside is dropped by the update unless
    a row continues it.  Everything else is BoxTracker's.  device "cpu" runs belt_shift_host and track_host."""


class WideBeltTracker(_BeltShift, WideBoxTracker):
    """WideBoxTracker with the belt's shift in front of every update: up to 16384 tracks and 8192 rows (the vote runs on the whole chip:
    three operations on the stream in front of the update's two).  The keywords are BeltTracker's and WideBoxTracker's."""
