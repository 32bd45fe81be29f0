"""Detection tracking: the host statement of the contract and both trackers."""

from __future__ import annotations

import numpy as np
import torch

from ._capi import OreError, _chk, _ptr, _stream, lib


# ---------------------------------------------------------------------------------------------------
# Detection tracking (csrc/ore_track.hip; association contract "track v1", include/ore_hip.h).  BoxTracker holds the state and runs the
# kernel, track_host is the numpy statement of the same contract: both give the same ids and the same state.
TRACK_MAX_TRACKS = 1024                                    # ORE_TRACK_MAX_TRACKS
TRACK_WIDE_MAX_TRACKS, TRACK_WIDE_MAX_ROWS = 16384, 8192   # ORE_TRACK_WIDE_MAX_TRACKS, ORE_TRACK_WIDE_MAX_ROWS (csrc/ore_track_wide.hip)
TRACK_WIDE_DEFAULTS = {"capacity": 4096, "max_rows": 2048, "iou_thresh": 0.6, "ttl": 8, "class_aware": True, "score_thresh": 0.0}
TRACK_DEFAULTS = {"capacity": 1024, "iou_thresh": 0.6, "ttl": 8, "class_aware": True, "score_thresh": 0.0}
_TRACK_HEADER = 32                                         # bytes: int32 m, capacity; int64 next_id, frames, dropped


def _track_params(who: str, capacity, iou_thresh, ttl, class_aware, score_thresh, max_tracks: int = TRACK_MAX_TRACKS) -> dict:
    """The parameters of a tracker, checked against the limits of ore_track_update_fwd (max_tracks = TRACK_WIDE_MAX_TRACKS: of
    ore_track_wide_update_fwd); the thresholds as the fp32 the kernel takes."""
    with np.errstate(over="ignore"):
        iou, sc = np.float32(iou_thresh), np.float32(score_thresh)
    if isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer)) or not 1 <= capacity <= max_tracks:
        raise OreError(f"{who}: capacity {capacity!r} (1 .. {max_tracks})")
    if isinstance(ttl, bool) or not isinstance(ttl, (int, np.integer)) or not 1 <= ttl <= 1 << 20:
        raise OreError(f"{who}: ttl {ttl!r} (1 .. {1 << 20})")
    if not (np.isfinite(iou) and iou >= 0):
        raise OreError(f"{who}: iou_thresh {iou_thresh!r} is finite and >= 0")
    if np.isnan(sc):
        raise OreError(f"{who}: score_thresh is NaN")
    return {"capacity": int(capacity), "iou_thresh": iou, "ttl": int(ttl), "class_aware": bool(class_aware), "score_thresh": sc}


def track_state_empty(capacity: int = 1024) -> dict:
    """The state of a tracker that has seen no frame, as track_host takes and returns it: the arrays cut at m = 0."""
    return {"boxes": np.zeros((0, 4), np.float32), "classes": np.zeros(0, np.int64), "ids": np.zeros(0, np.int64), "ttl": np.zeros(0, np.int32),
            "m": 0, "next_id": 0, "frames": 0, "dropped": 0}


def track_host(state, boxes, scores, classes=None, n=None, *, capacity: int = 1024, iou_thresh: float = 0.6, ttl: int = 8,
               class_aware: bool = True, score_thresh: float = 0.0, wide: bool = False):
    """One update of the association contract "track v1" (include/ore_hip.h) on the host, numpy fp32 one operation at a time: what
    ore_track_update_fwd computes, bit for bit.  wide=True: the same code with the limits of ore_track_wide_update_fwd (capacity up to
    16384, up to 8192 rows) -- what that computes, bit for bit.  state: a dict {boxes [m, 4] fp32, classes, ids [m] int64, ttl [m] int32, m, next_id,
    frames, dropped} (None: the empty state); boxes [rows, 4], scores [rows], classes [rows] or None (all 0), n = rows taken (None: all).
    Returns (ids [rows] int64 with -1 for rows that are not live, the new state); `state` is left as it was."""
    as_np = lambda t: t.detach().cpu().numpy() if torch.is_tensor(t) else (None if t is None else np.asarray(t))
    p = _track_params("track_host", capacity, iou_thresh, ttl, class_aware, score_thresh, TRACK_WIDE_MAX_TRACKS if wide else TRACK_MAX_TRACKS)
    max_rows = TRACK_WIDE_MAX_ROWS if wide else int(lib().ore_det_record_rows())
    st = track_state_empty() if state is None else state
    m = int(st["m"])
    tb = np.asarray(as_np(st["boxes"]), dtype=np.float32).reshape(-1, 4)[:m]
    tc, ti, tt = (np.asarray(as_np(st[k])).reshape(-1)[:m] for k in ("classes", "ids", "ttl"))
    b = np.ascontiguousarray(np.asarray(as_np(boxes), dtype=np.float32)).reshape(-1, 4)
    s = np.asarray(as_np(scores), dtype=np.float32).reshape(-1)
    rows = len(s)
    if rows > max_rows or len(b) != rows:
        raise OreError(f"track_host: {len(b)} boxes, {rows} scores (at most {max_rows} rows)")
    c = np.zeros(rows, dtype=np.int64) if classes is None else np.asarray(as_np(classes), dtype=np.int64).reshape(-1)
    n = rows if n is None else min(max(int(n), 0), rows)
    with np.errstate(all="ignore"):
        live = (np.arange(rows) < n) & np.isfinite(b).all(1) & np.isfinite(s) & (s >= p["score_thresh"])
        # IoU [m, rows], the contract's expression: a subtraction, a product, a sum, a difference and a quotient, each rounded to fp32
        area_t = (tb[:, 2] - tb[:, 0]) * (tb[:, 3] - tb[:, 1])
        area_d = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
        iw = np.minimum(tb[:, None, 2], b[None, :, 2]) - np.maximum(tb[:, None, 0], b[None, :, 0])
        ih = np.minimum(tb[:, None, 3], b[None, :, 3]) - np.maximum(tb[:, None, 1], b[None, :, 1])
        inter = np.where((iw > 0) & (ih > 0), iw * ih, np.float32(0))
        union = (area_t[:, None] + area_d[None, :]) - inter
        iou = np.where(inter > 0, inter / np.where(inter > 0, union, np.float32(1)), np.float32(0)).astype(np.float32)
        cand = live[None, :] & (iou > p["iou_thresh"])
    if p["class_aware"]:
        cand &= tc[:, None] == c[None, :]
    # greedy over (iou descending, slot ascending, row ascending): np.nonzero lists the pairs by (slot, row), a stable sort keeps that
    ts, ds = np.nonzero(cand)
    order = np.argsort(-iou[ts, ds].astype(np.float64), kind="stable")
    row_track = np.full(rows, -1, dtype=np.int64)
    track_row = np.full(m, -1, dtype=np.int64)
    for k in order:
        t, d = int(ts[k]), int(ds[k])
        if track_row[t] < 0 and row_track[d] < 0:
            track_row[t], row_track[d] = d, t
    ids = np.full(rows, -1, dtype=np.int64)
    next_id = int(st["next_id"])
    for d in np.nonzero(live)[0]:
        if row_track[d] >= 0:
            ids[d] = ti[row_track[d]]
        else:
            ids[d] = next_id
            next_id += 1
    keep = (track_row < 0) & (tt.astype(np.int64) - 1 > 0)
    nb = np.concatenate([b[live], tb[keep]]).astype(np.float32).reshape(-1, 4)
    nc = np.concatenate([c[live], tc[keep]]).astype(np.int64)
    ni = np.concatenate([ids[live], ti[keep]]).astype(np.int64)
    nt = np.concatenate([np.full(int(live.sum()), p["ttl"]), tt[keep].astype(np.int64) - 1]).astype(np.int32)
    total, cap = len(ni), p["capacity"]
    new = {"boxes": nb[:cap], "classes": nc[:cap], "ids": ni[:cap], "ttl": nt[:cap], "m": min(total, cap), "next_id": next_id,
           "frames": int(st["frames"]) + 1, "dropped": int(st["dropped"]) + max(total - cap, 0)}
    return ids, new


class BoxTracker:
    """Ids that persist from frame to frame (association contract "track v1", include/ore_hip.h):

        tracker = BoxTracker(device)                       # capacity=1024, iou_thresh=0.6, ttl=8, class_aware=True, score_thresh=0.0
        ids = tracker.update(boxes, scores, classes, n_dev)   # int64 [rows] on the device, -1 for rows that are not live; no sync
        tracker.update(instances)                          # a device Instances: also sets instances.track_ids
        tracker.stats()                                    # one sync: {"tracks", "started", "frames", "dropped"}

    On a device the state is one buffer and an update is one launch of ore_track_update_fwd on the current stream.  The tracker keeps
    the event behind its last update, and an update on another stream waits for it on the device: several streams may share one
    tracker, and the frames are associated in the order of the calls.  device "cpu" (or host tensors' tracker) runs track_host instead:
    the same ids."""

    # what WideBoxTracker replaces: the limits, the three entry points, the workspace
    MAX_TRACKS = TRACK_MAX_TRACKS
    _STATE_BYTES, _RESET, _UPDATE = "ore_track_state_bytes", "ore_track_reset", "ore_track_update_fwd"
    _host_kw: dict = {}

    def _row_limit(self) -> int:
        return int(lib().ore_det_record_rows())

    def _workspace(self):
        """(address or None, bytes) of the update's workspace."""
        return None, 0

    def __init__(self, device, *, capacity: int = 1024, iou_thresh: float = 0.6, ttl: int = 8, class_aware: bool = True,
                 score_thresh: float = 0.0):
        self.params = _track_params(type(self).__name__, capacity, iou_thresh, ttl, class_aware, score_thresh, self.MAX_TRACKS)
        self.capacity = self.params["capacity"]
        self.device = torch.device(device)
        self._host = None if self.device.type == "cuda" else track_state_empty()
        self._event, self._event_stream = None, None
        if self._host is None:
            if self.device.index is None:
                self.device = torch.device("cuda", torch.cuda.current_device())
            nbytes = int(getattr(lib(), self._STATE_BYTES)(self.capacity))
            with torch.cuda.device(self.device):
                self._buf = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
                self._event = torch.cuda.Event()
            cap, o = self.capacity, _TRACK_HEADER
            self._hdr32, self._hdr64 = self._buf[:8].view(torch.int32), self._buf[8:32].view(torch.int64)
            self._boxes = self._buf[o:o + 16 * cap].view(torch.float32).view(cap, 4)
            self._classes = self._buf[o + 16 * cap:o + 24 * cap].view(torch.int64)
            self._ids = self._buf[o + 24 * cap:o + 32 * cap].view(torch.int64)
            self._ttl = self._buf[o + 32 * cap:o + 36 * cap].view(torch.int32)
        self.reset()

    def _ordered(self) -> int:
        """The current stream, made to follow the tracker's last update wherever that ran."""
        cur = _stream()
        if self._event_stream is not None and self._event_stream != cur:
            here = torch.cuda.current_stream(self.device)
            here.wait_event(self._event)
            self._buf.record_stream(here)
        return cur

    def _updated(self, cur: int) -> None:
        self._event.record(torch.cuda.current_stream(self.device))
        self._event_stream = cur

    def _before_update(self, boxes, scores, classes, n_dev, n_host: int, rows: int, cur: int) -> None:
        """What a subclass enqueues on the update's stream `cur` in front of the update, once every check of the rows has passed and
        the stream follows the last update (orehip/belt.py moves the tracks here).  Nothing, in this class."""

    def _before_host(self, boxes, scores, classes, n) -> None:
        """The same in front of track_host, for a tracker on the host."""

    def reset(self) -> None:
        """The empty state: no tracks, next_id 0, the counters 0.  Enqueued on the current stream (device) like an update."""
        if self._host is not None:
            self._host = track_state_empty()
            return
        with torch.cuda.device(self.device):
            cur = self._ordered()
            _chk(getattr(lib(), self._RESET)(_ptr(self._buf), self.capacity, cur), self._RESET)
            self._updated(cur)

    def update(self, boxes, scores=None, classes=None, n_dev=None, *, out=None):
        """The ids of one frame's rows, and the state moved on by that frame.  boxes [rows, 4] fp32, scores [rows] fp32, classes [rows]
        int64 or None; n_dev: an int32 device tensor holding the row count (read by the kernel), an int, or None: every row.  Or one
        Instances (pred_boxes, scores, optional pred_classes), whose track_ids is set as well.  out: an int64 [rows] tensor for the ids."""
        if scores is None and hasattr(boxes, "has") and hasattr(boxes, "pred_boxes"):
            inst = boxes
            if not inst.has("pred_boxes") or not inst.has("scores"):
                raise OreError("BoxTracker.update: the Instances needs pred_boxes and scores")
            b = inst.pred_boxes
            b = b.tensor if hasattr(b, "tensor") else torch.as_tensor(b)
            c = inst.pred_classes.long().contiguous() if inst.has("pred_classes") else None
            ids = self.update(b.float().contiguous().reshape(-1, 4), inst.scores.float().contiguous(), c, out=out)
            inst.track_ids = ids
            return ids
        if scores is None:
            raise OreError("BoxTracker.update takes boxes and scores, or one Instances")
        if self._host is not None:
            n = int(n_dev.reshape(-1)[0]) if torch.is_tensor(n_dev) else n_dev
            self._before_host(boxes, scores, classes, n)
            ids, self._host = track_host(self._host, boxes, scores, classes, n, **self.params, **self._host_kw)
            ids = torch.from_numpy(ids)
            if out is not None:
                out.copy_(ids)
                ids = out
            return ids
        dev = self.device
        rows = int(boxes.shape[0])
        if not all(torch.is_tensor(t) and t.device == dev for t in (boxes, scores) + (() if classes is None else (classes,))):
            raise OreError(f"BoxTracker.update: the rows are tensors on the tracker's device {dev}")
        if not (boxes.dtype == torch.float32 and scores.dtype == torch.float32 and (classes is None or classes.dtype == torch.int64) and
                boxes.dim() == 2 and boxes.shape[1] == 4 and scores.dim() == 1 and int(scores.shape[0]) == rows and
                (classes is None or (classes.dim() == 1 and int(classes.shape[0]) == rows)) and
                (rows == 0 or (boxes.stride(1) == 1 and boxes.stride(0) == 4)) and
                (rows <= 1 or (scores.stride(0) == 1 and (classes is None or classes.stride(0) == 1)))):
            raise OreError("BoxTracker.update: boxes [n, 4] fp32, scores [n] fp32, classes [n] int64, rows contiguous")
        if rows > self._row_limit():
            raise OreError(f"{type(self).__name__}.update: {rows} rows (at most {self._row_limit()})")
        n_host = rows
        if n_dev is not None and not torch.is_tensor(n_dev):
            n_host, n_dev = min(max(int(n_dev), 0), rows), None
        if n_dev is not None and not (n_dev.dtype == torch.int32 and n_dev.device == dev and n_dev.numel() >= 1):
            raise OreError("BoxTracker.update: n_dev is an int32 tensor on the tracker's device (the kernel reads its first element)")
        with torch.cuda.device(dev):
            if out is None:
                out = torch.empty(rows, dtype=torch.int64, device=dev)
            elif not (torch.is_tensor(out) and out.dtype == torch.int64 and out.device == dev and out.dim() == 1 and
                      int(out.shape[0]) == rows and (rows <= 1 or out.stride(0) == 1)):
                raise OreError("BoxTracker.update: out is a contiguous int64 tensor [n] on the tracker's device")
            p = self.params
            cur = self._ordered()
            ws, ws_bytes = self._workspace()
            self._before_update(boxes, scores, classes, n_dev, n_host, rows, cur)
            _chk(getattr(lib(), self._UPDATE)(_ptr(self._buf), self.capacity, _ptr(boxes) if rows else None, _ptr(scores) if rows else None,
                                              _ptr(classes) if rows else None, _ptr(n_dev), n_host, rows, float(p["score_thresh"]),
                                              float(p["iou_thresh"]), p["ttl"], int(p["class_aware"]), _ptr(out) if rows else None, ws,
                                              ws_bytes, cur), self._UPDATE)
            self._updated(cur)
        return out

    def state(self) -> dict:
        """Views of the state: boxes [capacity, 4], classes, ids, ttl [capacity] (the first m are the list, the rest zeros) and m,
        next_id, frames, dropped as one-element tensors.  Device tensors: synchronise with the updates' stream before reading them."""
        if self._host is not None:
            return {k: (torch.from_numpy(np.array(v)) if isinstance(v, np.ndarray) else torch.tensor([v])) for k, v in self._host.items()}
        return {"boxes": self._boxes, "classes": self._classes, "ids": self._ids, "ttl": self._ttl, "m": self._hdr32[0:1],
                "next_id": self._hdr64[0:1], "frames": self._hdr64[1:2], "dropped": self._hdr64[2:3]}

    def state_host(self) -> dict:
        """The state as track_host's dict (numpy, the arrays cut at m); one explicit sync on a device."""
        if self._host is not None:
            return dict(self._host)
        self._event.synchronize()
        raw = self._buf.cpu().numpy()
        cap, o = self.capacity, _TRACK_HEADER
        m = int(raw[:4].view(np.int32)[0])
        nxt, frames, dropped = (int(v) for v in raw[8:32].view(np.int64))
        return {"boxes": raw[o:o + 16 * cap].view(np.float32).reshape(cap, 4)[:m].copy(), "classes": raw[o + 16 * cap:o + 24 * cap].view(np.int64)[:m].copy(),
                "ids": raw[o + 24 * cap:o + 32 * cap].view(np.int64)[:m].copy(), "ttl": raw[o + 32 * cap:o + 36 * cap].view(np.int32)[:m].copy(),
                "m": m, "next_id": nxt, "frames": frames, "dropped": dropped}

    def stats(self) -> dict:
        """{"tracks": the list's length, "started": ids issued so far (the particle count), "frames", "dropped"} as Python ints, after
        one explicit sync with the last update."""
        if self._host is not None:
            h = self._host
            return {"tracks": int(h["m"]), "started": int(h["next_id"]), "frames": int(h["frames"]), "dropped": int(h["dropped"])}
        self._event.synchronize()
        raw = self._buf[:_TRACK_HEADER].cpu().numpy()
        nxt, frames, dropped = (int(v) for v in raw[8:32].view(np.int64))
        return {"tracks": int(raw[:4].view(np.int32)[0]), "started": nxt, "frames": frames, "dropped": dropped}


class WideBoxTracker(BoxTracker):
    """BoxTracker for the rows of a tiled or TTA merge: up to 16384 tracks and 8192 rows per update (csrc/ore_track_wide.hip), the same
    contract "track v1", the same ids and the same state as BoxTracker wherever both take the input.

        tracker = WideBoxTracker(device)                   # capacity=4096, max_rows=2048, iou_thresh=0.6, ttl=8, ...
        ids = tracker.update(boxes, scores, classes, n_dev)   # two launches on the current stream, no sync

    max_rows is the most rows one update takes; it sizes the workspace (candidate bits of every track x row tile, the copy of the old
    list).  Everything else -- update, reset, state, state_host, stats, the Instances form, out=, n_dev, the ordering across streams
    -- is BoxTracker's.  device "cpu" runs track_host(wide=True)."""

    MAX_TRACKS = TRACK_WIDE_MAX_TRACKS
    _STATE_BYTES, _RESET, _UPDATE = "ore_track_wide_state_bytes", "ore_track_wide_reset", "ore_track_wide_update_fwd"
    _host_kw = {"wide": True}

    def __init__(self, device, *, capacity: int = 4096, max_rows: int = 2048, iou_thresh: float = 0.6, ttl: int = 8,
                 class_aware: bool = True, score_thresh: float = 0.0):
        if isinstance(max_rows, bool) or not isinstance(max_rows, (int, np.integer)) or not 0 <= max_rows <= TRACK_WIDE_MAX_ROWS:
            raise OreError(f"WideBoxTracker: max_rows {max_rows!r} (0 .. {TRACK_WIDE_MAX_ROWS})")
        self.max_rows = int(max_rows)
        self._ws = None
        super().__init__(device, capacity=capacity, iou_thresh=iou_thresh, ttl=ttl, class_aware=class_aware, score_thresh=score_thresh)
        if self._host is None:
            self._ws_bytes = int(lib().ore_track_wide_workspace_bytes(self.capacity, self.max_rows))
            with torch.cuda.device(self.device):
                self._ws = torch.empty(max(self._ws_bytes, 256), dtype=torch.uint8, device=self.device)

    def _row_limit(self) -> int:
        return self.max_rows

    def _workspace(self):
        return _ptr(self._ws), self._ws_bytes

    def _ordered(self) -> int:
        cur = super()._ordered()
        if self._ws is not None and self._event_stream is not None and self._event_stream != cur:
            self._ws.record_stream(torch.cuda.current_stream(self.device))
        return cur
