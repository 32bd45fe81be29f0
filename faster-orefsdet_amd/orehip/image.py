"""Host-to-device copies, the Pillow-exact resize, support crops and the batch canvases of a training step."""

from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch

from ._capi import OreError, _chk, _f32, _ptr, _stream, lib


def to_device(t: torch.Tensor, dev) -> torch.Tensor:
    """Host tensor -> device without a blocking pageable copy (a pageable hipMemcpy drains the stream first: one hidden host sync per
    small upload): staged through torch's cached pinned allocator and issued asynchronously.  Device tensors pass through."""
    dev = torch.device(dev)
    if t.is_cuda:
        return t if t.device == dev or dev.index is None else t.to(dev)
    if dev.type != "cuda":
        return t.to(dev)
    return t.pin_memory().to(dev, non_blocking=True)


# ---------------------------------------------------------------------------------------------------
# image resize: Pillow's Image.resize(size, BILINEAR) on the device (csrc/ore_resize.hip, csrc/ore_resize_plan.cpp)
# ---------------------------------------------------------------------------------------------------
RESIZE_FORM_LDS, RESIZE_FORM_WORKSPACE = 1, 2            # ORE_RESIZE_FORM_* (include/ore_hip.h)


def resize_shortest_edge_shape(h: int, w: int, size: int, max_size: int) -> Tuple[int, int]:
    """(nh, nw) of detectron2 v0.5's ResizeShortestEdge.get_transform (d2z:data/transforms/augmentation_impl.py): the short side
    scaled to `size`, everything rescaled when the long side then exceeds `max_size`, int(x + 0.5) at the end -- the arithmetic of
    DatasetMapperWithSupport._resize_flip."""
    scale = size * 1.0 / min(h, w)
    nh, nw = (size, scale * w) if h < w else (scale * h, size)
    if max(nh, nw) > max_size:
        s2 = max_size * 1.0 / max(nh, nw)
        nh, nw = nh * s2, nw * s2
    return int(nh + 0.5), int(nw + 0.5)


def resize_plan(n_in: int, n_out: int) -> Tuple[np.ndarray, np.ndarray]:
    """One axis of the resample (ore_resize_plan, host only): bounds [n_out, 2] int32 = (first source index, count) and coeffs
    [n_out, ksize] int32, Pillow's 22-bit fixed-point weights.  A pixel is clip8((2^21 + sum(src * coeff)) >> 22)."""
    ks = int(lib().ore_resize_ksize(int(n_in), int(n_out)))
    if ks <= 0:
        raise OreError(f"resize_plan: sizes {n_in} -> {n_out} outside [1, 8192]")
    bounds, coeffs = np.empty((n_out, 2), dtype=np.int32), np.empty((n_out, ks), dtype=np.int32)
    _chk(lib().ore_resize_plan(int(n_in), int(n_out), bounds.ctypes.data, coeffs.ctypes.data, None), "ore_resize_plan")
    return bounds, coeffs


def resize_form(h: int, w: int, nh: int, nw: int) -> int:
    """The form resize_bilinear_u8 takes for this size pair: RESIZE_FORM_LDS (one launch) or RESIZE_FORM_WORKSPACE (two)."""
    return int(lib().ore_resize_form(int(h), int(w), int(nh), int(nw)))


_RESIZE_TABLES: Dict[tuple, torch.Tensor] = {}
_RESIZE_TABLES_MAX = 32
_RESIZE_WS: Dict[tuple, torch.Tensor] = {}


def _table_uploaded(tab: torch.Tensor, cur: int) -> None:
    """Mark a cached device table as uploaded just now, asynchronously, on the current stream `cur`: the event behind the copy is
    what a use on another stream has to wait for."""
    tab._ore_stream, tab._ore_event, tab._ore_arrived = cur, torch.cuda.Event(), False
    tab._ore_event.record(torch.cuda.current_stream(tab.device))


def _table_on_stream(tab: torch.Tensor, cur: int) -> None:
    """Make a cached table safe to read from work enqueued next on the current stream `cur`.  On the stream that uploaded it, stream
    order is enough.  Another stream is made to wait for the upload's event until that event is seen complete (the wait is enqueued
    on the device; the host does not block), and the table is marked as used there so that an eviction does not free it early."""
    if tab._ore_stream == cur:
        return
    stream = torch.cuda.current_stream(tab.device)
    if not tab._ore_arrived:
        tab._ore_arrived = tab._ore_event.query()
        if not tab._ore_arrived:
            stream.wait_event(tab._ore_event)
    tab.record_stream(stream)


def _cached_table(cache: Dict[tuple, torch.Tensor], cap: int, dev, key: tuple, fill, in_capture: Optional[str]) -> torch.Tensor:
    """The device table cached under `key`, safe to read from the launch enqueued next on the current stream.  On a miss fill() gives
    the table in pinned host memory, the oldest entry leaves while the cache holds `cap`, and the copy goes behind the current stream's
    work (_table_uploaded); a hit goes through _table_on_stream.  in_capture: the refusal of a miss during a stream capture, or None."""
    key = (str(dev),) + key
    tab = cache.get(key)
    cur = _stream()
    if tab is None:
        if in_capture is not None and torch.cuda.is_current_stream_capturing():
            raise OreError(in_capture)
        host = fill()
        while len(cache) >= cap:
            cache.pop(next(iter(cache)))
        tab = cache[key] = host.to(dev, non_blocking=True)
        _table_uploaded(tab, cur)
    else:
        _table_on_stream(tab, cur)
    return tab


def _resize_tables(dev, h: int, w: int, nh: int, nw: int) -> torch.Tensor:
    """The device tables of one size pair, cached.  A new table is planned on the host into pinned memory and copied behind the
    current stream's work, so the launch that follows on that stream reads it complete.  The cache is bounded: the oldest table
    leaves when a new one would be the 33rd.  Nothing here is captured in a graph, so a launch that still reads an evicted table is
    protected by stream order alone: torch's allocator hands the block to later work of the stream it was allocated on, and a table
    used on another stream is marked for that stream (record_stream) at that use.  A use on another stream than the uploading one
    first waits, on the device, for the event behind the upload (_table_on_stream)."""
    def fill() -> torch.Tensor:
        n = int(lib().ore_resize_table_ints(h, w, nh, nw))
        if n <= 0:
            raise OreError(f"resize_bilinear_u8: {h}x{w} -> {nh}x{nw}: sides must be in [1, 8192]")
        host = torch.empty(n, dtype=torch.int32, pin_memory=True)
        _chk(lib().ore_resize_tables_host(h, w, nh, nw, host.data_ptr()), "ore_resize_tables_host")
        return host

    return _cached_table(_RESIZE_TABLES, _RESIZE_TABLES_MAX, dev, (h, w, nh, nw), fill, None)


def resize_bilinear_u8(img_hwc_u8: torch.Tensor, nh: int, nw: int, swap_rb: bool = False, out: Optional[torch.Tensor] = None,
                       stream: Optional["torch.cuda.Stream"] = None, form: int = 0) -> torch.Tensor:
    """[h, w, 3] uint8 device tensor (interleaved, what an image reader gives) -> [3, nh, nw] uint8 planar, byte for byte
    np.asarray(Image.fromarray(img).resize((nw, nh), Image.BILINEAR)).transpose(2, 0, 1); swap_rb exchanges channels 0 and 2.
    form: 0 = the library's choice (resize_form), or RESIZE_FORM_LDS / RESIZE_FORM_WORKSPACE to force one."""
    if stream is not None:
        with torch.cuda.stream(stream):
            return resize_bilinear_u8(img_hwc_u8, nh, nw, swap_rb, out, None, form)
    assert img_hwc_u8.is_cuda and img_hwc_u8.dtype == torch.uint8 and img_hwc_u8.dim() == 3 and img_hwc_u8.shape[2] == 3 and \
        img_hwc_u8.is_contiguous(), "resize_bilinear_u8 takes a contiguous [h, w, 3] uint8 device tensor"
    h, w = int(img_hwc_u8.shape[0]), int(img_hwc_u8.shape[1])
    nh, nw = int(nh), int(nw)
    dev = img_hwc_u8.device
    with torch.cuda.device(dev):
        tab = _resize_tables(dev, h, w, nh, nw)
        if out is None:
            out = torch.empty(3, nh, nw, dtype=torch.uint8, device=dev)
        assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (3, nh, nw) and out.is_contiguous()
        ws, ws_bytes = None, 0
        if form == RESIZE_FORM_WORKSPACE or (form == 0 and resize_form(h, w, nh, nw) == RESIZE_FORM_WORKSPACE):
            ws_bytes = int(lib().ore_resize_workspace_bytes(h, w, nh, nw))
            ws_key = (str(dev), _stream())                          # per stream: two streams' passes must not share an intermediate
            ws = _RESIZE_WS.get(ws_key)
            if ws is None or ws.numel() < ws_bytes:
                ws = _RESIZE_WS[ws_key] = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        _chk(lib().ore_resize_bilinear_u8_fwd(_ptr(img_hwc_u8), h, w, _ptr(out), nh, nw, int(bool(swap_rb)), _ptr(tab), int(form), _ptr(ws),
                                              ws_bytes, _stream()), "ore_resize_bilinear_u8_fwd")
    return out


# ---------------------------------------------------------------------------------------------------
# support crops: annotated frames -> the S x S crops and support boxes of a support set (csrc/ore_support.hip, csrc/ore_support_plan.cpp)
# ---------------------------------------------------------------------------------------------------
SUPPORT_JOB_INTS = 32                                    # ORE_SUPPORT_JOB_INTS; the record's words are ORE_SJ_* (include/ore_hip.h)
SUPPORT_FILL = (104, 116, 124)                           # round(cfg.MODEL.PIXEL_MEAN): padding normalises to about 0
_SJ_H, _SJ_RECT, _SJ_DST, _SJ_XB, _SJ_YB, _SJ_KX, _SJ_KY, _SJ_KSX, _SJ_KSY, _SJ_FORM, _SJ_D, _SJ_X0, _SJ_BOX = 2, 4, 8, 12, 13, 14, 15, 16, 17, 18, 24, 25, 27
_SUPPORT_BUF: Dict[tuple, dict] = {}                     # (device, stream) -> pinned job buffers with their uploads' events, the device copy, the workspace


def _support_box(box) -> np.ndarray:
    b = np.ascontiguousarray(np.asarray(box, dtype=np.float32).reshape(4))
    return b


def _support_refused(h, w, box, size, context, index=None) -> ValueError:
    which = "box" if index is None else f"box {index}"
    return ValueError(f"support crop: {which} {[float(v) for v in box]} lies outside its {h}x{w} frame, or a size is out of range "
                      f"(frame sides 1 .. 8192, 2 * context {context} < size {size} <= 8192)")


def support_crop_form(h: int, w: int, box, size: int = 240, context: int = 16) -> int:
    """The form the crop of this box takes (ore_support_crop_form): RESIZE_FORM_LDS (served by the one launch that covers every such
    job of a call) or RESIZE_FORM_WORKSPACE (a horizontal and a vertical launch through a workspace slice)."""
    b = _support_box(box)
    form = int(lib().ore_support_crop_form(int(h), int(w), b.ctypes.data, int(size), int(context)))
    if form == 0:
        raise _support_refused(h, w, b, size, context)
    return form


def support_crop_plan(h: int, w: int, box, size: int = 240, context: int = 16) -> dict:
    """The plan of one support crop (ore_support_crop_plan, host only; the contract is "support crop v1" of include/ore_hip.h):
    {"D", "origin" (x0, y0), "src" (rx0, ry0, rx1, ry1), "dst" (dx0, dy0, dx1, dy1), "box" float32 [4] inside the crop, "form",
    "workspace_bytes", and the job's resample tables "x_bounds" [nw, 2], "x_coeffs" [nw, ksx], "y_bounds" [nh, 2], "y_coeffs" [nh, ksy]}."""
    L = lib()
    h, w, size, context = int(h), int(w), int(size), int(context)
    b = _support_box(box)
    n = int(L.ore_support_crop_job_ints(h, w, b.ctypes.data, size, context))
    if n == 0:
        raise _support_refused(h, w, b, size, context)
    buf = np.zeros(SUPPORT_JOB_INTS + n, dtype=np.int32)
    _chk(L.ore_support_crop_plan(h, w, b.ctypes.data, size, context, None, SUPPORT_JOB_INTS, 0, buf.ctypes.data, buf.ctypes.data),
         "ore_support_crop_plan")
    r = buf[:SUPPORT_JOB_INTS]
    src, dst = tuple(int(v) for v in r[_SJ_RECT:_SJ_RECT + 4]), tuple(int(v) for v in r[_SJ_DST:_SJ_DST + 4])
    nw, nh, ksx, ksy = dst[2] - dst[0], dst[3] - dst[1], int(r[_SJ_KSX]), int(r[_SJ_KSY])
    return {"D": int(r[_SJ_D]), "origin": (int(r[_SJ_X0]), int(r[_SJ_X0 + 1])), "src": src, "dst": dst,
            "box": r[_SJ_BOX:_SJ_BOX + 4].view(np.float32).copy(), "form": int(r[_SJ_FORM]),
            "workspace_bytes": int(L.ore_support_crop_workspace_bytes(h, w, b.ctypes.data, size, context)),
            "x_bounds": buf[r[_SJ_XB]:r[_SJ_XB] + nw * 2].reshape(nw, 2).copy(), "x_coeffs": buf[r[_SJ_KX]:r[_SJ_KX] + nw * ksx].reshape(nw, ksx).copy(),
            "y_bounds": buf[r[_SJ_YB]:r[_SJ_YB] + nh * 2].reshape(nh, 2).copy(), "y_coeffs": buf[r[_SJ_KY]:r[_SJ_KY] + nh * ksy].reshape(nh, ksy).copy()}


def support_crops(frames, boxes, frame_index=None, size: int = 240, context: int = 16, fill=SUPPORT_FILL,
                  out: Optional[torch.Tensor] = None, device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Support crops of K boxes ("support crop v1", include/ore_hip.h).  frames: one [h, w, 3] uint8 tensor / array or a list of them
    (sizes may differ; a host frame is uploaded once through pinned memory), boxes [K, 4] XYXY absolute, frame_index [K] (default: all
    0).  Returns (crops [K, 3, size, size] uint8 on the device, planar, the frames' channel order; support boxes [K, 4] float32 on the
    host).  All K jobs are planned on the host into one pinned buffer, uploaded with one copy, and run by at most three launches on
    the current stream; the host does not wait for the device: a pinned buffer is written again only once the upload that read it
    is seen complete (an event query), and while none is free another one is added.  The buffers are cached per (device, stream)
    and do not touch the resize tables' cache.  A box outside its frame: ValueError naming its index."""
    L = lib()
    size, context = int(size), int(context)
    if torch.is_tensor(frames) or isinstance(frames, np.ndarray):
        frames = [frames]
    frames = [torch.from_numpy(np.ascontiguousarray(f)) if isinstance(f, np.ndarray) else f for f in frames]
    if device is None:
        device = next((f.device for f in frames if f.is_cuda), None) or torch.device("cuda", torch.cuda.current_device())
    dev = torch.device(device)
    bx = np.ascontiguousarray(torch.as_tensor(boxes).detach().cpu().numpy() if torch.is_tensor(boxes) else np.asarray(boxes), dtype=np.float32).reshape(-1, 4)
    K = len(bx)
    fi = np.zeros(K, dtype=np.int64) if frame_index is None else np.asarray(torch.as_tensor(frame_index).cpu().numpy(), dtype=np.int64).reshape(-1)
    if K < 1 or len(fi) != K or (fi < 0).any() or (fi >= len(frames)).any():
        raise ValueError(f"support_crops: {K} boxes, {len(fi)} frame indices into {len(frames)} frames")
    fill = tuple(int(v) for v in fill)
    if len(fill) != 3 or min(fill) < 0 or max(fill) > 255:
        raise ValueError(f"support_crops: fill must be three bytes, not {fill}")
    for f in frames:
        if f.dtype != torch.uint8 or f.dim() != 3 or f.shape[2] != 3:
            raise ValueError(f"support_crops takes [h, w, 3] uint8 frames, not {tuple(f.shape)} {f.dtype}")
    with torch.cuda.device(dev):
        used = sorted(set(int(i) for i in fi))
        on_dev = {i: (frames[i] if frames[i].is_cuda else frames[i].contiguous().pin_memory().to(dev, non_blocking=True)).contiguous() for i in used}
        # sizes first: table words and workspace slice of every job
        n_tab, n_ws = [], []
        for k in range(K):
            h, w = int(frames[fi[k]].shape[0]), int(frames[fi[k]].shape[1])
            n = int(L.ore_support_crop_job_ints(h, w, bx[k].ctypes.data, size, context))
            if n == 0:
                raise _support_refused(h, w, bx[k], size, context, k)
            n_tab.append(n)
            n_ws.append(int(L.ore_support_crop_workspace_bytes(h, w, bx[k].ctypes.data, size, context)))
        total, ws_bytes = K * SUPPORT_JOB_INTS + sum(n_tab), sum(n_ws)
        cur = _stream()
        st = _SUPPORT_BUF.setdefault((str(dev), cur), {"pinned": [], "dev": None, "ws": None})
        # a pinned buffer whose last upload has completed (queried, not waited for); a backlog on the stream adds a buffer instead
        slot = next((p for p in st["pinned"] if p["host"].numel() >= total and (p["event"] is None or p["event"].query())), None)
        if slot is None:
            st["pinned"] = [p for p in st["pinned"] if p["host"].numel() >= total or not (p["event"] is None or p["event"].query())]     # outgrown and idle: dropped
            slot = {"host": torch.empty(total, dtype=torch.int32, pin_memory=True), "event": None}
            st["pinned"].append(slot)
        if st["dev"] is None or st["dev"].numel() < total:
            st["dev"] = torch.empty(total, dtype=torch.int32, device=dev)
        if ws_bytes and (st["ws"] is None or st["ws"].numel() < ws_bytes):
            st["ws"] = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        st["last"] = slot                                                      # the latest call's plan (tools/bench_support.py replays it)
        host, base = slot["host"], slot["host"].data_ptr()
        t_off, w_off = K * SUPPORT_JOB_INTS, 0
        for k in range(K):
            f = on_dev[int(fi[k])]
            _chk(L.ore_support_crop_plan(int(f.shape[0]), int(f.shape[1]), bx[k].ctypes.data, size, context, f.data_ptr(), t_off, w_off,
                                         base + 4 * k * SUPPORT_JOB_INTS, base), "ore_support_crop_plan")
            t_off += n_tab[k]
            w_off += n_ws[k]
        st["dev"][:total].copy_(host[:total], non_blocking=True)               # the call's one upload
        slot["event"] = torch.cuda.Event()
        slot["event"].record(torch.cuda.current_stream(dev))
        if out is None:
            out = torch.empty(K, 3, size, size, dtype=torch.uint8, device=dev)
        assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (K, 3, size, size) and out.is_contiguous()
        _chk(L.ore_support_crop_u8_fwd(_ptr(st["dev"]), base, total, K, size, fill[0] | fill[1] << 8 | fill[2] << 16, _ptr(out),
                                       _ptr(st["ws"]) if ws_bytes else None, ws_bytes, cur), "ore_support_crop_u8_fwd")
        rec = host[:K * SUPPORT_JOB_INTS].view(K, SUPPORT_JOB_INTS)
        sboxes = rec[:, _SJ_BOX:_SJ_BOX + 4].contiguous().view(torch.float32).clone()
    return out, sboxes


# ---------------------------------------------------------------------------------------------------
# batch canvases of a training step ("batch canvas v1", include/ore_hip.h; csrc/ore_batch_canvas.hip)
# ---------------------------------------------------------------------------------------------------
BATCH_CANVAS_JOB_INTS = 8                                # ORE_BATCH_CANVAS_JOB_INTS
_BCJ_SRC, _BCJ_H, _BCJ_W, _BCJ_DST, _BCJ_HC, _BCJ_WC = 0, 2, 3, 4, 6, 7


class BatchCanvasGeom(tuple):
    """What of a batch-canvas plan is a launch argument -- and therefore fixed in a captured launch: (n_query, (Hq, Wq), query_u8,
    n_support, (Hs, Ws), support_u8, table_bytes, slab_bytes).  Two plans with equal geometry are served by the same launch."""
    __slots__ = ()
    n_query = property(lambda s: s[0])
    q_canvas = property(lambda s: s[1])
    q_u8 = property(lambda s: s[2])
    n_support = property(lambda s: s[3])
    s_canvas = property(lambda s: s[4])
    s_u8 = property(lambda s: s[5])
    table_bytes = property(lambda s: s[6])
    slab_bytes = property(lambda s: s[7])

    @property
    def out_floats(self) -> int:
        return self.n_query * 3 * self.q_canvas[0] * self.q_canvas[1] + self.n_support * 3 * self.s_canvas[0] * self.s_canvas[1]


class BatchCanvasPlan:
    """One step's raw images packed for ore_batch_canvas_fwd: `host` = ONE pinned uint8 buffer [table | slab] (the table: one row of
    BATCH_CANVAS_JOB_INTS int32 words per job, query rows first; the slab: every image planar at its own size, each at a 16-byte
    boundary), `used` = the bytes of it that a step has to upload, `table` = the rows as an int32 [jobs, 8] view of the buffer,
    `geom` = the launch's fixed arguments."""

    def __init__(self, host, used, table, geom):
        self.host, self.used, self.table, self.geom = host, int(used), table, geom


def _canvas_group(images, what: str):
    """A group's images as a flat list of [3, h, w] host tensors of one dtype (a [N, 3, h, w] tensor counts as N images), and the
    tensors as given, each with the index of its first image: [(first, [n, 3, h, w])]."""
    flat, blocks = [], []
    for t in images:
        t = torch.as_tensor(t)
        if t.is_cuda:
            raise ValueError(f"batch_canvas_plan packs host images; a {what} image lives on {t.device}")
        blocks.append((len(flat), t if t.dim() == 4 else t[None]))
        if t.dim() == 4:
            flat.extend(t[i] for i in range(t.shape[0]))
        else:
            flat.append(t)
    for t in flat:
        if t.dim() != 3 or t.shape[0] != 3 or t.shape[1] < 1 or t.shape[2] < 1:
            raise ValueError(f"batch_canvas_plan takes [3, h, w] images, not a {what} image of shape {tuple(t.shape)}")
        if t.dtype not in (torch.uint8, torch.float32):
            raise ValueError(f"batch_canvas_plan takes raw uint8 or fp32 images, not a {what} image of {t.dtype}")
        if t.dtype != flat[0].dtype:
            raise ValueError(f"batch_canvas_plan: the {what} images mix {flat[0].dtype} and {t.dtype}; one dtype per group")
    return flat, blocks


def batch_canvas_plan(queries, supports=(), div: int = 32, q_canvas: Optional[Tuple[int, int]] = None,
                      s_canvas: Optional[Tuple[int, int]] = None, capacity: Optional[Tuple[int, int]] = None,
                      full_slab: bool = False) -> BatchCanvasPlan:
    """Host plan of one step's batch canvases: the query images (a list of [3, h, w] host tensors, sizes may differ) and the support
    crops (a list of [3, h, w] or [N, 3, h, w] host tensors) packed into one pinned buffer, table and slab together, so that ONE
    host-to-device copy per step replaces one upload per image.  A group's canvas is its largest height and width rounded up to `div`
    (ImageList.from_tensors), or `q_canvas` / `s_canvas` as given.  `capacity` = (query jobs, support jobs) of the launch (default: the
    images given); rows beyond the images given are empty jobs, whose canvases come out all zero.  `full_slab`: the slab is sized for
    images that fill their canvases -- the geometry, and with it the launch, then depends on nothing but the canvases, the capacities
    and the dtypes (a captured launch).  ValueError: an image larger than its canvas, two dtypes within a group, more images than the
    capacity, an image on the device."""
    both = [_canvas_group(queries, "query"), _canvas_group(supports, "support")]
    groups, blocks = [b[0] for b in both], [b[1] for b in both]
    cap =[len(groups[0]), len(groups[1])] if capacity is None else [int(capacity[0]), int(capacity[1])]
    canv, u8 = [], []
    for g, (imgs, given, what) in enumerate(zip(groups, (q_canvas, s_canvas), ("query", "support"))):
        if len(imgs) > cap[g]:
            raise ValueError(f"batch_canvas_plan: {len(imgs)} {what} images, the capacity is {cap[g]}")
        if given is not None:
            Hc, Wc = int(given[0]), int(given[1])
        elif imgs:
            Hc, Wc = (-(-max(int(t.shape[d]) for t in imgs) // div) * div for d in (1, 2))
        else:
            Hc, Wc = 0, 0
        for i, t in enumerate(imgs):
            if t.shape[1] > Hc or t.shape[2] > Wc:
                raise ValueError(f"batch_canvas_plan: {what} image {i} of {t.shape[1]} x {t.shape[2]} is larger than its {Hc} x {Wc} canvas")
        if cap[g] and (Hc < 1 or Wc < 4 or Wc % 4 or max(Hc, Wc) > 8192):
            raise ValueError(f"batch_canvas_plan: {what} canvas {Hc} x {Wc} (sides 1 .. 8192, the width a multiple of 4)")
        canv.append((Hc, Wc))
        u8.append(bool(imgs[0].dtype == torch.uint8) if imgs else True)
    if cap[0] + cap[1] < 1 or cap[0] + cap[1] > 65535:
        raise ValueError(f"batch_canvas_plan: {cap[0]} + {cap[1]} jobs (1 .. 65535 in all)")
    up16 = lambda n: (n + 15) // 16 * 16                 # noqa: E731
    esz = [1 if u else 4 for u in u8]
    table_bytes = up16((cap[0] + cap[1]) * BATCH_CANVAS_JOB_INTS * 4)
    packed = sum(up16(3 * int(t.shape[1]) * int(t.shape[2]) * esz[g]) for g in range(2) for t in groups[g])
    slab_bytes = sum(cap[g] * up16(3 * canv[g][0] * canv[g][1] * esz[g]) for g in range(2)) if full_slab else max(packed, 16)
    geom = BatchCanvasGeom((cap[0], canv[0], u8[0], cap[1], canv[1], u8[1], table_bytes, slab_bytes))
    host = torch.empty(table_bytes + slab_bytes, dtype=torch.uint8, pin_memory=torch.cuda.is_available())
    table = host[:(cap[0] + cap[1]) * BATCH_CANVAS_JOB_INTS * 4].view(torch.int32).view(cap[0] + cap[1], BATCH_CANVAS_JOB_INTS)
    jobs = cap[0] + cap[1]
    rows = np.zeros((jobs, BATCH_CANVAS_JOB_INTS), dtype=np.int64)
    first = (0, cap[0])
    for g in range(2):
        j0, n = first[g], len(groups[g])
        rows[j0:j0 + n, _BCJ_H] = [int(t.shape[1]) for t in groups[g]]
        rows[j0:j0 + n, _BCJ_W] = [int(t.shape[2]) for t in groups[g]]
        rows[j0:j0 + cap[g], _BCJ_HC], rows[j0:j0 + cap[g], _BCJ_WC] = canv[g]
        rows[j0:j0 + cap[g], _BCJ_DST] = (first[g] and cap[0] * 3 * canv[0][0] * canv[0][1]) + np.arange(cap[g]) * (3 * canv[g][0] * canv[g][1])
    nbytes = 3 * rows[:, _BCJ_H] * rows[:, _BCJ_W] * np.repeat(esz, cap)
    src = np.concatenate([[0], np.cumsum((nbytes + 15) // 16 * 16)])                     # every image at a 16-byte boundary
    rows[:, _BCJ_SRC] = src[:-1]
    for at in (_BCJ_SRC, _BCJ_DST):
        rows[:, at + 1], rows[:, at] = rows[:, at] >> 32, rows[:, at] & 0xffffffff
    table.copy_(torch.from_numpy(rows.astype(np.uint32).view(np.int32)))
    for g in range(2):
        for i0, t in blocks[g]:                                                           # a tensor of crops whose images tile the slab: one copy
            n, j = int(t.shape[0]), first[g] + i0
            nb = int(nbytes[j])
            for k in ([None] if nb % 16 == 0 or n == 1 else range(n)):
                a = table_bytes + int(src[j + (k or 0)])
                piece = host[a:a + (n if k is None else 1) * nb]
                piece = (piece if u8[g] else piece.view(torch.float32)).view(-1, *t.shape[1:])
                piece.copy_(t if k is None else t[k:k + 1])
    return BatchCanvasPlan(host, table_bytes + int(src[-1]), table, geom)


def batch_canvas(buf: torch.Tensor, geom: BatchCanvasGeom, pixel_mean: torch.Tensor, pixel_std: torch.Tensor,
                 out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The query and the support canvas of a step from ONE launch (ore_batch_canvas_fwd): buf = the device copy of a BatchCanvasPlan's
    buffer (`plan.host[:plan.used]` at its start; a buffer of a captured launch is written again before every replay), geom = the
    plan's geometry, pixel_mean / pixel_std = the model's buffers on the device.  Returns (xq [n_query, 3, Hq, Wq], xs [n_support, 3, Hs,
    Ws]) fp32, both views of `out` (allocated if not given): (float(raw) - mean) / std inside every image, +0.0 in the padding -- the
    tensors the mixed-size branch of train_forward.train_core builds with a handful of torch ops per image."""
    assert buf.is_cuda and buf.dtype == torch.uint8 and buf.is_contiguous() and buf.numel() >= geom.table_bytes + geom.slab_bytes, \
        "batch_canvas: buf is the uint8 device buffer [table | slab] of the plan's geometry"
    mean, std = _f32(pixel_mean.reshape(-1)), _f32(pixel_std.reshape(-1))
    assert mean.numel() == 3 and std.numel() == 3 and mean.device == buf.device and std.device == buf.device
    n = geom.out_floats
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=buf.device)
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= n
    with torch.cuda.device(buf.device):
        _chk(lib().ore_batch_canvas_fwd(buf.data_ptr() + geom.table_bytes, geom.slab_bytes, _ptr(buf), geom.n_query, geom.q_canvas[0],
                                        geom.q_canvas[1], int(geom.q_u8), geom.n_support, geom.s_canvas[0], geom.s_canvas[1], int(geom.s_u8),
                                        _ptr(mean), _ptr(std), _ptr(out), out.numel(), _stream()), "ore_batch_canvas_fwd")
    flat = out.view(-1)
    nq = geom.n_query * 3 * geom.q_canvas[0] * geom.q_canvas[1]
    return (flat[:nq].view(geom.n_query, 3, *geom.q_canvas), flat[nq:n].view(geom.n_support, 3, *geom.s_canvas))
