"""Tiled (sliced) inference for frames larger than one detector pass: the frame is cut into overlapping tiles at native resolution,
every tile is detected, one resized full-frame pass adds the objects larger than a tile overlap, the rows go back into frame
coordinates, fragments cut by a tile seam are dropped and ONE class-aware NMS merges the rest (the merge of GeneralizedRCNNWithTTA,
fast_rcnn_inference_single_image).

The whole frame stays on the device: one upload, one gather launch that writes every tile as a planar uint8 image
(orehip.tile_gather_u8), one device resize for the full-frame pass (orehip.resize_bilinear_u8), one engine replay per pass -- `fold`
tiles per pass through Engine.eval_forward_batch -- with the rows of every image collected behind it (ore_tile_collect_fwd: seam rule,
offset, appended at a device-side offset) and one merge (ore_tta_merge_fwd), all queued on the current stream; the host waits once, for
the merged count.  With track= the merged rows get ids that persist from frame to frame (orehip.WideBoxTracker, association contract
"track v1"): the update is queued behind the merge, on the merged record and its device-side count, before that one wait.  With support_classes set (N-way) the engine's merged rows exist only in the record of a finished pass, so the host
polls once per source.

Seam rule: a tile row whose box comes within `margin` pixels of a tile side that is not a frame side is taken to be the fragment of an
object the seam cut, and is rejected; rows of the full-frame pass are never rejected.  An object whose extent is at most overlap - 2 *
margin lies whole, and clear of the margin, in at least one tile; larger objects rely on the full-frame pass.  orehip.tile_plan,
tile_gather_host and tile_collect_host state the arithmetic on the host; the kernels are held to them bit for bit
(tests/test_tile_host.py, tests/test_hip_tiles.py)."""
import numpy as np
import torch
from torch import nn

__all__ = ["TiledInference", "check_tiling_limits", "merge_tracker"]

FRAME_MAX_SIDE = 8192                      # ore_tile_gather_u8_fwd / ore_resize_bilinear_u8_fwd
MAX_TILES = 128                            # ore_tile_gather_u8_fwd
MIN_TILE_SIDE = 64
MERGE_POOL_ROWS = 8192                     # ore_tta_merge_fwd
DETECT_MAX_LOCATIONS = 30720               # locations of the stride-8 level the detection tail caches in LDS (csrc/ore_detect.hip)
SCORE_THRESH = 1e-8                        # the merge's score threshold, as GeneralizedRCNNWithTTA._merge_detections


def _pair(v, what):
    v = tuple(int(x) for x in v) if isinstance(v, (tuple, list)) else (int(v), int(v))
    if len(v) != 2:
        raise ValueError(f"TiledInference: {what} is one number or (y, x), got {v!r}")
    return v


def _locations(h, w):
    """Locations of the stride-8 level of an [h, w] input (padded to a multiple of 32)."""
    return ((h + 31) // 32 * 4) * ((w + 31) // 32 * 4)


def check_tile_shape(tile, overlap):
    """ValueError for a tile / overlap pair no frame can be cut with."""
    for t, o in zip(tile, overlap):
        if t < MIN_TILE_SIDE:
            raise ValueError(f"TiledInference: tile {tile[0]}x{tile[1]}: a tile side is at least {MIN_TILE_SIDE}")
        if not 0 <= o < t:
            raise ValueError(f"TiledInference: overlap {overlap[0]}x{overlap[1]} must be >= 0 and below the tile {tile[0]}x{tile[1]}")


def check_tiling_limits(frame_hw, plan, full_hw, rows):
    """ValueError for a frame the device cannot run, before any GPU work.  plan: orehip.tile_plan of the frame; full_hw: the size of the
    resized full-frame pass or None; rows: the detection rows one engine pass returns at most."""
    h, w = frame_hw
    if not (1 <= h <= FRAME_MAX_SIDE and 1 <= w <= FRAME_MAX_SIDE):
        raise ValueError(f"TiledInference: frame {h}x{w}: the device gather and resize take sides 1 .. {FRAME_MAX_SIDE}")
    n = plan["ny"] * plan["nx"]
    th, tw = plan["th"], plan["tw"]
    if n > MAX_TILES:
        raise ValueError(f"TiledInference: {plan['ny']}x{plan['nx']} = {n} tiles of {th}x{tw} for a {h}x{w} frame, one gather takes {MAX_TILES}; "
                         "use a larger tile or a smaller overlap")
    sources = n + (1 if full_hw is not None else 0)
    if sources * rows > MERGE_POOL_ROWS:
        raise ValueError(f"TiledInference: {sources} sources x {rows} detection rows = {sources * rows} candidates for a {h}x{w} frame, the "
                         f"merge pool takes {MERGE_POOL_ROWS}; use a larger tile or lower TEST.DETECTIONS_PER_IMAGE")
    if _locations(th, tw) > DETECT_MAX_LOCATIONS:
        raise ValueError(f"TiledInference: a {th}x{tw} tile has {_locations(th, tw)} stride-8 locations, the detection tail takes "
                         f"{DETECT_MAX_LOCATIONS} per image; use a smaller tile")
    if full_hw is not None and _locations(*full_hw) > DETECT_MAX_LOCATIONS:
        raise ValueError(f"TiledInference: the full-frame pass at {full_hw[0]}x{full_hw[1]} has {_locations(*full_hw)} stride-8 locations, the "
                         f"detection tail takes {DETECT_MAX_LOCATIONS} per image; lower INPUT.MIN_SIZE_TEST / MAX_SIZE_TEST or pass "
                         "full_frame=False")


def merge_tracker(who, track, rows, device):
    """The tracker behind a merge that keeps `rows` record rows, from a wrapper's track= argument: None / False -> None; True -> an
    orehip.WideBoxTracker on `device` sized for the merge (max_rows = rows, capacity = rows live rows plus as many survivors, within
    the kernel's limit); a tracker object as given, if it is on `device` and takes `rows` rows."""
    import orehip
    if track is None or track is False:
        return None
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if track is True:
        return orehip.WideBoxTracker(device, capacity=min(2 * rows, orehip.TRACK_WIDE_MAX_TRACKS), max_rows=rows)
    if not isinstance(track, orehip.BoxTracker) or track.device != device:
        raise ValueError(f"{who}: track is None, True or an orehip.BoxTracker / WideBoxTracker on the model's device {device}")
    if rows > track._row_limit():
        raise ValueError(f"{who}: the merge keeps {rows} rows, the tracker takes {track._row_limit()}; use an orehip.WideBoxTracker "
                         f"with max_rows >= {rows}")
    return track


def enqueue_track(tracker, p):
    """The tracker's update behind a merge, on the current stream: reads the merged record's views and its device-side count."""
    import orehip
    boxes, scores, classes = orehip.record_views(p.rec, p.rows, p.rows)
    return tracker.update(boxes, scores, classes, p.count)


class _Pending:
    """One frame between `_enqueue` and `_finish`: the result record, its device count, the output size, the pool and the plan; with
    a tracker, the ids of the record's rows."""
    __slots__ = ("rec", "count", "rows", "out_hw", "pool", "plan", "full_hw", "ids")


class _Slot:
    """One of the wrapper's engines with what it was built for."""
    __slots__ = ("engine", "key", "hw", "bufs")


class TiledInference(nn.Module):
    """Sliced inference over the CenterNet2Detector of this package (module docstring).  `__call__(batched_inputs)` takes request dicts
    that carry the frame as "image_raw" ([h, w, 3] uint8: numpy array, CPU tensor or device tensor; "swap_rb" exchanges channels 0 and
    2), as "file_name" (read in the model's input format) or as "image" ([3, h, w] uint8, taken as the frame itself), and returns
    [{"instances": Instances}] with pred_boxes / scores / pred_classes in the frame's own coordinates: "height" / "width", if present,
    must equal the frame's size.

    tile = (th, tw) and overlap (one number or (y, x)) give orehip.tile_plan; margin is the seam rule's; full_frame adds the pass over
    the frame resized to INPUT.MIN_SIZE_TEST / MAX_SIZE_TEST as source 0; fold tiles go through one engine pass (N-way: ignored, one
    pass per source); the merge keeps max_detections rows (default TEST.DETECTIONS_PER_IMAGE) behind score threshold 1e-8 and
    MODEL.ROI_HEADS.NMS_THRESH_TEST.  Per source the rows are those `model.inference([{"image": source}], do_postprocess=False)`
    returns.  The wrapper owns its engines -- one of `fold` images at the tile's size, one at the resized frame's -- keyed like
    model.engine() and rebuilt when the key changes; the model's own cached engine is left alone.  Frames the device cannot run
    (check_tiling_limits) are a ValueError before any GPU work; no source is ever skipped.

    track=True follows the merged detections from frame to frame in the order of the calls: an orehip.WideBoxTracker sized for
    max_detections, on the model's device (or pass a tracker of your own).  The result's Instances then carries track_ids, and
    track_stats() counts the tracks started.  The frame still has one host wait."""

    def __init__(self, cfg, model, tile=(640, 640), overlap=128, margin=2.0, full_frame=True, fold=1, max_detections=None, track=None):
        super().__init__()
        from fewx.modeling.fsod.fsod_cen import CenterNet2Detector
        while not isinstance(model, CenterNet2Detector) and isinstance(getattr(model, "module", None), nn.Module):
            model = model.module                              # FlatDataParallel / DistributedDataParallel
        if not isinstance(model, CenterNet2Detector):
            raise TypeError(f"TiledInference wraps a CenterNet2Detector, not {type(model).__name__}")
        self.cfg = cfg.clone()
        self.model = model
        self.tile, self.overlap = _pair(tile, "tile"), _pair(overlap, "overlap")
        check_tile_shape(self.tile, self.overlap)
        self.margin = float(margin)
        if not self.margin >= 0.0:
            raise ValueError(f"TiledInference: margin {margin} must be >= 0")
        self.full_frame = bool(full_frame)
        self.fold = int(fold)
        if not 1 <= self.fold <= MAX_TILES:
            raise ValueError(f"TiledInference: fold {fold} outside 1 .. {MAX_TILES}")
        self.topk = int(cfg.TEST.DETECTIONS_PER_IMAGE if max_detections is None else max_detections)
        if not 1 <= self.topk <= MERGE_POOL_ROWS:
            raise ValueError(f"TiledInference: max_detections {self.topk} outside 1 .. {MERGE_POOL_ROWS}")
        self.nms_thresh = float(cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST)
        self.test_size = (int(cfg.INPUT.MIN_SIZE_TEST), int(cfg.INPUT.MAX_SIZE_TEST))
        self._slots = {}
        self._pools = {}
        self.tracker = merge_tracker("TiledInference", track, self.topk + (self.topk & 1), model.device)

    def track_stats(self):
        """BoxTracker.stats() of the frames so far: tracks, started (the particle count), frames, dropped.  One host sync."""
        if self.tracker is None:
            return {"tracks": 0, "started": 0, "frames": 0, "dropped": 0}
        return self.tracker.stats()

    # ---- plan and limits (host) ---------------------------------------------------------------------------------
    def _rows(self):
        """The detection rows one engine pass returns at most: the second stage's top-k, within the result record."""
        import orehip
        return min(max(int(self.model.roi_heads.test_topk), 1), int(orehip.lib().ore_det_record_rows()))

    def plan(self, h, w):
        """(tile plan, size of the full-frame pass or None) of an [h, w] frame, checked against the device's limits."""
        import orehip
        plan = orehip.tile_plan(h, w, self.tile, self.overlap)
        full_hw = orehip.resize_shortest_edge_shape(h, w, *self.test_size) if self.full_frame and 1 <= min(h, w) else None
        check_tiling_limits((h, w), plan, full_hw, self._rows())
        return plan, full_hw

    # ---- engines and pools --------------------------------------------------------------------------------------
    def _engine(self, name, need_hw, max_batch):
        """The wrapper's engine `name` ("tile" / "full"): rebuilt when the model's engine key changes (weights, support set, device,
        precision, class selection) or a frame needs more room than it has."""
        import orehip
        m = self.model
        key = (m._engine_key_now(), max_batch)
        s = self._slots.get(name)
        if s is None or s.key != key or need_hw[0] > s.hw[0] or need_hw[1] > s.hw[1]:
            hw = tuple(need_hw) if s is None else (max(need_hw[0], s.hw[0]), max(need_hw[1], s.hw[1]))
            if s is not None:
                s.engine.close()
                del self._slots[name]
            try:
                e = m.make_engine(max_batch=max_batch, classes=key[0][3], max_hw=hw)
            except orehip.OreError as err:
                raise ValueError(f"TiledInference: no engine for {max_batch} input(s) up to {hw[0]}x{hw[1]}: {err}") from err
            if not getattr(e, "has_roi", False):
                e.close()
                raise ValueError("TiledInference needs the second stage inside the engine (a support set with rcnn_8 features)")
            s = self._slots[name] = _Slot()
            s.engine, s.key, s.hw, s.bufs = e, key, hw, {}
        return s

    @staticmethod
    def _det_bufs(slot, b, batched):
        """(boxes, scores, count) of image b of the slot's engine, looked up once."""
        tag = (b, batched)
        if tag not in slot.bufs:
            sfx = f"#{b}" if batched else ""
            slot.bufs[tag] = tuple(slot.engine.buffer(n + sfx) for n in ("det_boxes", "det_scores", "det_count"))
        return slot.bufs[tag]

    def _pool(self, sources, rows):
        import orehip
        key = (sources, rows, str(self.model.device))
        p = self._pools.get(key)
        if p is None:
            p = self._pools[key] = orehip.TilePool(sources, rows, self.model.device)
        return p

    # ---- requests -----------------------------------------------------------------------------------------------
    def _source(self, inp):
        """(kind, host-or-device frame, its (h, w), swap_rb): kind "raw" = [h, w, 3], "image" = [3, h, w]."""
        if "image" in inp and "image_raw" in inp:
            raise ValueError('a request carries either "image" or "image_raw", not both')
        if "image" in inp:
            img = inp["image"]
            if not torch.is_tensor(img):
                img = torch.from_numpy(np.ascontiguousarray(img))
            if img.dim() != 3 or img.shape[0] != 3 or img.dtype != torch.uint8:
                raise ValueError(f'TiledInference cuts 8-bit frames: "image" must be [3, h, w] uint8, got {tuple(img.shape)} {img.dtype}')
            kind, frame, hw, swap = "image", img, (int(img.shape[1]), int(img.shape[2])), False
        else:
            if "image_raw" in inp:
                raw = inp["image_raw"]
            elif "file_name" in inp:                          # _maybe_read_image: read in the model's input format
                from fewx.data.dataset_mapper import _pil_read_image
                raw = _pil_read_image(inp["file_name"], self.model.input_format)
            else:
                raise ValueError('a TiledInference request needs "image", "image_raw" or "file_name"')
            if isinstance(raw, np.ndarray):
                raw = torch.from_numpy(np.ascontiguousarray(raw))
            if raw.dim() != 3 or raw.shape[2] != 3 or raw.dtype != torch.uint8:
                raise ValueError(f"image_raw must be [h, w, 3] uint8, got {tuple(raw.shape)} {raw.dtype}")
            kind, frame, hw, swap = "raw", raw, (int(raw.shape[0]), int(raw.shape[1])), bool(inp.get("swap_rb", False))
        want = (int(inp.get("height", hw[0])), int(inp.get("width", hw[1])))
        if want != hw:
            raise ValueError(f'TiledInference answers in the frame\'s own coordinates: "height" / "width" {want[0]}x{want[1]} differ from '
                             f"the frame's {hw[0]}x{hw[1]}")
        return kind, frame, hw, swap

    def forward(self, batched_inputs):
        return [self._inference_one_frame(x) for x in batched_inputs]

    @torch.no_grad()
    def _inference_one_frame(self, inp):
        assert not self.model.training, "TiledInference is an evaluation wrapper: model.eval() first"
        self.model.init_model()
        return self._finish(self._enqueue(inp))

    def _finish(self, p):
        """The one host wait of a frame: the merged count; then the record is cut into the result."""
        import orehip
        from detectron2.structures import Boxes, Instances
        k = int(p.count.item())
        boxes, scores, classes = orehip.record_views(p.rec, p.rows, k)
        res = Instances(p.out_hw)
        res.pred_boxes = Boxes(boxes)
        res.scores = scores
        res.pred_classes = classes
        if p.ids is not None:
            res.track_ids = p.ids[:k]
        return {"instances": res}

    # ---- the device path ----------------------------------------------------------------------------------------
    def _enqueue(self, inp):
        """Everything of one frame up to the merged record, queued on the current stream; single-class: no host synchronisation."""
        import orehip
        m = self.model
        kind, src, (h, w), swap = self._source(inp)
        plan, full_hw = self.plan(h, w)                       # every limit, before any GPU work
        n_tiles, th, tw = plan["ny"] * plan["nx"], plan["th"], plan["tw"]
        rows = self._rows()
        nway = m._support_selection() is not None
        fold = 1 if nway else min(self.fold, n_tiles)
        tile_slot = self._engine("tile", (th, tw), fold)
        full_slot = self._engine("full", full_hw, 1) if full_hw is not None else None
        for s in (tile_slot, full_slot):
            if s is not None and int(getattr(s.engine, "_det_cap", rows)) != rows:
                raise ValueError(f"TiledInference: the engine returns {s.engine._det_cap} detection rows per pass, the pool was sized for {rows}")
        if kind == "raw":
            hwc = m._upload_raw(src)
        else:                                                 # a planar frame -> the interleaved layout the gather and the resize read
            hwc = orehip.to_device(src, m.device).permute(1, 2, 0).contiguous()
        with torch.cuda.device(m.device):
            tiles = orehip.tile_gather_u8(hwc, plan, swap_rb=swap)
            full = orehip.resize_bilinear_u8(hwc, full_hw[0], full_hw[1], swap_rb=swap) if full_hw is not None else None
            first = 1 if full is not None else 0
            pool = self._pool(n_tiles + first, rows)
            tile_args = [dict(sx=1.0, sy=1.0, ox=float(x0), oy=float(y0), src_hw=(th, tw), edges=orehip.tile_edges(plan, i, h, w),
                              margin=self.margin) for i, (y0, x0) in enumerate(plan["origins"])]
            full_args = dict(sx=w * 1.0 / full_hw[1], sy=h * 1.0 / full_hw[0], ox=0.0, oy=0.0, src_hw=full_hw, edges=0,
                             margin=self.margin) if full is not None else None
            if nway:                                          # the merged N-way rows arrive with a finished pass: one poll per source
                if full is not None:
                    b, s, c = full_slot.engine.detect_classes(full, full_hw[0], full_hw[1])
                    orehip.tile_collect(pool, 0, b, s, c, int(len(s)), rows, **full_args)
                for i in range(n_tiles):
                    b, s, c = tile_slot.engine.detect_classes(tiles[i], th, tw)
                    orehip.tile_collect(pool, first + i, b, s, c, int(len(s)), rows, **tile_args[i])
            else:
                if full is not None:
                    full_slot.engine.eval_forward(full, use_graph=True)
                    b, s, n = self._det_bufs(full_slot, 0, False)
                    orehip.tile_collect(pool, 0, b, s, None, n, rows, **full_args)
                for j in range(0, n_tiles, fold):
                    part = range(j, min(j + fold, n_tiles))
                    if self.fold > 1:
                        tile_slot.engine.eval_forward_batch(tiles[part.start:part.stop], use_graph=True)
                    else:
                        tile_slot.engine.eval_forward(tiles[j], use_graph=True)
                    for k, i in enumerate(part):
                        b, s, n = self._det_bufs(tile_slot, k, self.fold > 1)
                        orehip.tile_collect(pool, first + i, b, s, None, n, rows, **tile_args[i])
            p = _Pending()
            p.rec, p.count = orehip.tta_merge(pool, h, w, SCORE_THRESH, self.nms_thresh, self.topk)
            p.rows, p.out_hw, p.pool, p.plan, p.full_hw = self.topk + (self.topk & 1), (h, w), pool, plan, full_hw
            p.ids = enqueue_track(self.tracker, p) if self.tracker is not None else None
            return p
