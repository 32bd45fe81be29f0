"""The detection overlay: kernel wrapper and its numpy twin."""

from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch

from ._capi import OreError, _chk, _ptr, _stream, lib
from .image import _cached_table


# ---------------------------------------------------------------------------------------------------
# detection overlay (csrc/ore_overlay.hip): boxes, scores and class names drawn onto a frame; render contract "overlay v1" of
# include/ore_hip.h.  overlay_draw is the kernel, overlay_host the numpy statement of the same contract: both give the same bytes.
# ---------------------------------------------------------------------------------------------------
OVERLAY_MAX_SIDE, OVERLAY_TEXT, OVERLAY_NAME = 8192, 40, 32          # ORE_OVERLAY_MAX_SIDE; characters of a label; bytes of a name
# the default palette, RGB (a BGR frame takes it reversed along the last axis): the one place it is defined
OVERLAY_PALETTE = np.array([[230, 25, 75], [60, 180, 75], [255, 225, 25], [0, 130, 200], [245, 130, 48], [145, 30, 180], [70, 240, 240],
                            [240, 50, 230], [210, 245, 60], [250, 190, 212], [0, 128, 128], [220, 190, 255], [170, 110, 40],
                            [255, 250, 200], [128, 0, 0], [170, 255, 195], [128, 128, 0], [255, 215, 180], [0, 0, 128], [128, 128, 128]],
                           dtype=np.uint8)
_OVERLAY_ATLAS: Optional[np.ndarray] = None
_OVERLAY_TABLES: Dict[tuple, torch.Tensor] = {}
_OVERLAY_TABLES_MAX = 32
_OVERLAY_WS: Dict[tuple, torch.Tensor] = {}
_OVERLAY_WS_MAX = 16


def overlay_atlas() -> np.ndarray:
    """[95, 11, 6] uint8 (0 / 1): the glyphs of ASCII 32 .. 126 of Pillow's embedded bitmap font, every one a 6 x 11 cell of coverage
    0 or 255.  Built once; the kernel, overlay_host and the tests read this one table."""
    global _OVERLAY_ATLAS
    if _OVERLAY_ATLAS is None:
        from PIL import ImageFont
        font = ImageFont.load_default_imagefont()
        atlas = np.zeros((95, 11, 6), dtype=np.uint8)
        for ch in range(32, 127):
            m = font.getmask(chr(ch))
            if m.size != (6, 11):
                raise OreError(f"overlay_atlas: glyph {ch} of Pillow's bitmap font is {m.size}, not 6 x 11")
            cov = np.asarray(m, dtype=np.uint8).reshape(11, 6)
            if not np.isin(cov, (0, 255)).all():
                raise OreError(f"overlay_atlas: glyph {ch} of Pillow's bitmap font is not 0 / 255")
            atlas[ch - 32] = cov != 0
        atlas.setflags(write=False)
        _OVERLAY_ATLAS = atlas
    return _OVERLAY_ATLAS


def overlay_names_table(names) -> np.ndarray:
    """Class names as the kernel's table: [n, 32] uint8, ASCII, NUL-padded (longer names are cut at 32 bytes)."""
    names = [] if names is None else list(names)
    tab = np.zeros((len(names), OVERLAY_NAME), dtype=np.uint8)
    for i, nm in enumerate(names):
        raw = str(nm).encode("ascii", "replace")[:OVERLAY_NAME]
        tab[i, :len(raw)] = np.frombuffer(raw, dtype=np.uint8)
    return tab


def _overlay_palette(palette) -> np.ndarray:
    pal = OVERLAY_PALETTE if palette is None else np.ascontiguousarray(np.asarray(palette))
    if pal.dtype != np.uint8 or pal.ndim != 2 or pal.shape[1] != 3 or not 1 <= pal.shape[0] <= 256:
        raise OreError(f"overlay: the palette is [1 .. 256, 3] uint8, got {pal.shape} {pal.dtype}")
    return pal


def _overlay_color_by(color_by: str, ids=None, has_ids: bool = True) -> int:
    """0 instance, 1 class, 2 track ("overlay v1, track colouring": needs ids)."""
    if color_by not in ("instance", "class", "track"):
        raise OreError(f'overlay: color_by is "instance", "class" or "track", not {color_by!r}')
    if color_by == "track" and ids is None and has_ids:
        raise OreError('overlay: color_by "track" needs ids (the ids of a BoxTracker update)')
    return ("instance", "class", "track").index(color_by)


def _overlay_table_dev(dev, key: tuple, make) -> torch.Tensor:
    """A constant table (atlas, palette, names) on the device, uploaded once and cached under `key` (make() builds the numpy table on a
    miss); never built inside a stream capture.  Stream order, the upload's event for a use on another stream, and record_stream
    protect a table as they do the resize tables (_resize_tables, _table_on_stream)."""
    def fill() -> torch.Tensor:
        arr = np.array(make(), dtype=np.uint8).reshape(-1)        # a writable copy: the atlas is read-only
        host = torch.empty(max(arr.size, 1), dtype=torch.uint8, pin_memory=True)
        host[:arr.size].copy_(torch.from_numpy(arr))
        return host

    return _cached_table(_OVERLAY_TABLES, _OVERLAY_TABLES_MAX, dev, key, fill,
                         "overlay_draw: a table is not on the device yet; draw once outside the stream capture first")


def overlay_draw(frame_hwc_u8: torch.Tensor, boxes: torch.Tensor, scores: torch.Tensor, classes: Optional[torch.Tensor] = None,
                 n_dev: Optional[torch.Tensor] = None, *, out: Optional[torch.Tensor] = None, score_thresh: float = 0.0, line_width: int,
                 text_scale: int, edge_alpha: int = 128, label_alpha: int = 204, palette=None, color_by: str = "instance",
                 names=None, ids: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Detection rows drawn onto a contiguous [h, w, 3] uint8 device frame (ore_overlay_draw_fwd; the render contract "overlay v1" of
    include/ore_hip.h), enqueued on the current stream, no host sync.  boxes [n, 4] fp32 xyxy at the frame's size, scores [n] fp32,
    classes [n] int64 or None (all 0): device tensors whose rows are contiguous.  n_dev: an int32 device tensor holding the row count
    (read by the kernel; at most boxes.shape[0] rows are taken), or None: every row.  out=None returns a fresh frame, out=frame draws
    in place.  palette: [k, 3] uint8 in the frame's channel order (None: OVERLAY_PALETTE, RGB); color_by "instance" or "class";
    names: class names (None: no names, the labels are the percentages); text_scale 0 draws no labels.  ids [n] int64 (a BoxTracker
    update's) with color_by "track": "overlay v1, track colouring" -- rows with a negative id are not drawn, the colour follows the id
    and "#<id> " leads the label; with another color_by the ids are ignored."""
    f = frame_hwc_u8
    assert f.is_cuda and f.dtype == torch.uint8 and f.dim() == 3 and f.shape[2] == 3 and f.is_contiguous(), \
        "overlay_draw takes a contiguous [h, w, 3] uint8 device tensor"
    h, w = int(f.shape[0]), int(f.shape[1])
    dev = f.device
    rows = int(boxes.shape[0])
    assert boxes.dtype == torch.float32 and scores.dtype == torch.float32 and (classes is None or classes.dtype == torch.int64)
    assert (rows == 0 or boxes.stride(-1) == 1 and boxes.stride(0) == 4) and int(scores.shape[0]) == rows and \
        (classes is None or int(classes.shape[0]) == rows), "overlay_draw: boxes [n, 4], scores [n], classes [n], rows contiguous"
    assert rows <= 1 or (scores.stride(0) == 1 and (classes is None or classes.stride(0) == 1))
    assert all(t is None or t.device == dev for t in (boxes, scores, classes)), "overlay_draw: the rows live on the frame's device"
    if n_dev is not None and not (torch.is_tensor(n_dev) and n_dev.dtype == torch.int32 and n_dev.device == dev and n_dev.numel() >= 1):
        raise OreError("overlay_draw: n_dev is an int32 tensor on the frame's device (the kernel reads its first element)")
    if out is None:
        out = torch.empty_like(f)
    assert out.is_cuda and out.dtype == torch.uint8 and out.shape == f.shape and out.is_contiguous() and out.device == dev
    pal = _overlay_palette(palette)
    by = _overlay_color_by(color_by, ids)
    if ids is not None and not (torch.is_tensor(ids) and ids.dtype == torch.int64 and ids.device == dev and ids.dim() == 1 and
                                int(ids.shape[0]) == rows and (rows <= 1 or ids.stride(0) == 1)):
        raise OreError("overlay_draw: ids is a contiguous int64 tensor [n] on the frame's device")
    names = () if names is None else tuple(str(nm) for nm in names)
    with torch.cuda.device(dev):
        pal_d = _overlay_table_dev(dev, ("palette", None if palette is None else pal.tobytes()), lambda: pal)
        atlas_d = _overlay_table_dev(dev, ("atlas",), overlay_atlas) if int(text_scale) >= 1 else None
        names_d = _overlay_table_dev(dev, ("names", names), lambda: overlay_names_table(names)) if names else None
        ws_bytes = int(lib().ore_overlay_workspace_bytes(rows))
        ws_key = (str(dev), _stream())                              # per stream: two streams' draws must not share an instance table
        ws = _OVERLAY_WS.get(ws_key)
        if ws is None or ws.numel() < ws_bytes:
            while ws is None and len(_OVERLAY_WS) >= _OVERLAY_WS_MAX:    # streams come and go: the oldest stream's workspace leaves
                _OVERLAY_WS.pop(next(iter(_OVERLAY_WS)))                  # (its block returns to the stream it was allocated on)
            ws = _OVERLAY_WS[ws_key] = torch.empty(max(ws_bytes, int(lib().ore_overlay_workspace_bytes(int(lib().ore_det_record_rows())))),
                                                   dtype=torch.uint8, device=dev)
        if ids is None:
            _chk(lib().ore_overlay_draw_fwd(_ptr(f), _ptr(out), h, w, _ptr(boxes) if rows else None, _ptr(scores) if rows else None,
                                            _ptr(classes) if rows else None, _ptr(n_dev), rows, rows, float(np.float32(score_thresh)),
                                            int(line_width), int(text_scale), int(edge_alpha), int(label_alpha), _ptr(pal_d), len(pal), by,
                                            _ptr(names_d), len(names), _ptr(atlas_d), _ptr(ws), ws.numel(), _stream()), "ore_overlay_draw_fwd")
        else:
            _chk(lib().ore_overlay_draw_ids_fwd(_ptr(f), _ptr(out), h, w, _ptr(boxes) if rows else None, _ptr(scores) if rows else None,
                                                _ptr(classes) if rows else None, _ptr(ids) if rows else None, _ptr(n_dev), rows, rows,
                                                float(np.float32(score_thresh)), int(line_width), int(text_scale), int(edge_alpha),
                                                int(label_alpha), _ptr(pal_d), len(pal), by, _ptr(names_d), len(names), _ptr(atlas_d),
                                                _ptr(ws), ws.numel(), _stream()), "ore_overlay_draw_ids_fwd")
    return out


def _blend8(p: np.ndarray, c, a: int) -> np.ndarray:
    return ((p.astype(np.int32) * (255 - a) + np.asarray(c, dtype=np.int32) * a + 127) // 255).astype(np.uint8)


def overlay_instance_table(boxes, scores, classes, n, h: int, w: int, score_thresh: float, text_scale: int, palette: np.ndarray, color_by: int,
                           names_tab: np.ndarray, ids=None) -> List[dict]:
    """The instance table of the render contract, in draw order, as the prepare step of the kernel builds it: per drawn row the
    integer rectangle, colour, text colour, label text and label rectangle.  Host arithmetic in numpy fp32, one operation at a time.
    color_by 2 ("overlay v1, track colouring") reads ids [n] int64: negative ids are not drawn, the id picks the colour and leads the text."""
    by_track = color_by == 2
    if by_track:
        if ids is None:
            raise OreError('overlay: color_by "track" needs ids')
        tid = np.asarray(ids, dtype=np.int64).reshape(-1)
    b = np.ascontiguousarray(np.asarray(boxes, dtype=np.float32)).reshape(-1, 4)
    s = np.asarray(scores, dtype=np.float32).reshape(-1)
    c = np.zeros(len(s), dtype=np.int64) if classes is None else np.asarray(classes, dtype=np.int64).reshape(-1)
    n = len(s) if n is None else min(max(int(n), 0), len(s))
    b, s, c = b[:n], s[:n], c[:n]
    S = int(text_scale)
    with np.errstate(all="ignore"):
        ok = np.isfinite(b).all(1) & np.isfinite(s) & (s >= np.float32(score_thresh))
        if by_track:
            if len(tid) < n:
                raise OreError(f"overlay: {len(tid)} ids for {n} rows")
            tid = tid[:n]
            ok &= tid >= 0
        X0 = np.clip(np.floor(b[:, 0]), 0, w)
        Y0 = np.clip(np.floor(b[:, 1]), 0, h)
        X1 = np.clip(np.ceil(b[:, 2]), 0, w) - 1
        Y1 = np.clip(np.ceil(b[:, 3]), 0, h) - 1
        ok &= (X1 >= X0) & (Y1 >= Y0)
        area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
        pct = np.clip(np.rint(s * np.float32(100.0)), 0, 100)
    area = np.where(np.isnan(area), np.float32(0), area)
    idx = np.arange(n)
    table: List[Optional[dict]] = [None] * int(ok.sum())
    for i in idx[ok]:
        rank = int((ok & ((area > area[i]) | ((area == area[i]) & (idx < i)))).sum())
        col = palette[int((tid[i] if by_track else c[i] if color_by else i) % len(palette))].astype(np.int32)
        q = {"row": int(i), "rect": (int(X0[i]), int(Y0[i]), int(X1[i]), int(Y1[i])), "col": col, "tcol": col + ((255 - col) * 7) // 10, "text": b""}
        if S >= 1:
            name = b""
            if 0 <= c[i] < len(names_tab):
                name = bytes(names_tab[c[i]]).split(b"\0")[0]
            text = (b"#%d " % int(tid[i]) if by_track else b"") + ((name + b" ") if name else b"") + b"%d%%" % int(pct[i])
            q["text"] = text = text[:OVERLAY_TEXT]
            lw, lh = len(text) * 6 * S + 2 * S, 13 * S
            q["label"] = (min(max(int(X0[i]), 0), max(w - lw, 0)), min(max(int(Y0[i]), 0), max(h - lh, 0)), lw, lh)
        table[rank] = q
    return table


def overlay_host(frame_hwc_u8, boxes, scores, classes=None, n=None, *, out=None, score_thresh: float = 0.0, line_width: int, text_scale: int,
                 edge_alpha: int = 128, label_alpha: int = 204, palette=None, color_by: str = "instance", names=None, ids=None) -> np.ndarray:
    """overlay_draw on the host: the numpy statement of the render contract "overlay v1" (include/ore_hip.h), byte for byte what the
    kernel draws.  Takes numpy arrays or CPU tensors; n = the row count (None: every row).  Returns an [h, w, 3] uint8 array: a fresh
    one, or `out` (the frame itself: in place)."""
    as_np = lambda t: t.detach().cpu().numpy() if torch.is_tensor(t) else (None if t is None else np.asarray(t))
    frame = as_np(frame_hwc_u8)
    if frame.dtype != np.uint8 or frame.ndim != 3 or frame.shape[2] != 3:
        raise OreError(f"overlay_host takes an [h, w, 3] uint8 frame, got {frame.shape} {frame.dtype}")
    h, w = frame.shape[:2]
    L, S = int(line_width), int(text_scale)
    rows = len(as_np(scores))
    if not (1 <= h <= OVERLAY_MAX_SIDE and 1 <= w <= OVERLAY_MAX_SIDE and 1 <= L <= 16 and 0 <= S <= 8 and 0 <= int(edge_alpha) <= 255 and
            0 <= int(label_alpha) <= 255 and rows <= int(lib().ore_det_record_rows())):
        raise OreError(f"overlay_host: frame {h}x{w} (sides 1 .. {OVERLAY_MAX_SIDE}), {rows} rows, line_width {L} (1 .. 16), text_scale {S} (0 .. 8), "
                       f"alphas {edge_alpha} / {label_alpha} (0 .. 255)")
    pal = _overlay_palette(palette)
    table = overlay_instance_table(as_np(boxes), as_np(scores), as_np(classes), n, h, w, score_thresh, S, pal, _overlay_color_by(color_by, ids),
                                   overlay_names_table(names), ids=as_np(ids))
    if out is None:
        img = frame.copy()
    else:
        img = out if out is frame_hwc_u8 or out is frame else as_np(out)
        if img is not frame:
            img[...] = frame
    atlas = overlay_atlas()
    for q in table:
        X0, Y0, X1, Y1 = q["rect"]
        xs, ys = np.arange(X0, X1 + 1), np.arange(Y0, Y1 + 1)
        edge = ((xs - X0 < L) | (X1 - xs < L))[None, :] | ((ys - Y0 < L) | (Y1 - ys < L))[:, None]
        reg = img[Y0:Y1 + 1, X0:X1 + 1]
        reg[edge] = _blend8(reg[edge], q["col"], int(edge_alpha))
        if S >= 1:
            lx, ly, lw, lh = q["label"]
            xs, ys = np.arange(lx, min(lx + lw, w)), np.arange(ly, min(ly + lh, h))
            reg = img[ly:ly + len(ys), lx:lx + len(xs)]
            reg[...] = _blend8(reg, 0, int(label_alpha))
            gx, gy = xs - lx - S, ys - ly - S
            chars = np.frombuffer(q["text"], dtype=np.uint8).astype(np.int64) - 32
            okx, oky = (gx >= 0) & (gx < len(chars) * 6 * S), (gy >= 0) & (gy < 11 * S)
            cell = np.clip(gx // (6 * S), 0, len(chars) - 1)
            ch = chars[cell]
            u, v = np.clip((gx - cell * 6 * S) // S, 0, 5), np.clip(gy // S, 0, 10)
            okx &= (ch >= 0) & (ch < 95)
            on = atlas[np.clip(ch, 0, 94)[None, :], v[:, None], u[None, :]].astype(bool) & okx[None, :] & oky[:, None]
            reg[on] = q["tcol"].astype(np.uint8)
    return img
