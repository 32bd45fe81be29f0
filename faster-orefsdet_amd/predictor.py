"""The demo's predictors (ref:predictor.py): VisualizationDemo draws a detector's boxes on images and video frames, AsyncPredictor keeps
several frames in flight.  Drawing is the package's device overlay (orehip.overlay_draw, render contract "overlay v1"), not matplotlib;
AsyncPredictor is one process with several engines on several HIP streams, not one process per GPU.  TiledPredictor is DefaultPredictor's
contract over fewx.modeling.TiledInference, for frames larger than one detector pass.  Both predictors can lay a heat map of the pass
under the boxes (heatmap=...: orehip.heatmap_draw, render contract "heatmap v1"): objectness, attention or a feature channel.
Both can follow the detections across the frames of a video (track=...: orehip.BoxTracker, association contract "track v1"): ids that
persist, and boxes coloured and labelled by them."""
from collections import deque

import numpy as np
import torch

from detectron2.data import MetadataCatalog
from detectron2.engine.defaults import DefaultPredictor
from detectron2.utils.video_visualizer import VideoVisualizer
from detectron2.utils.visualizer import ColorMode, VisImage, Visualizer, default_overlay_params, thing_classes

__all__ = ["AsyncPredictor", "TiledPredictor", "VisualizationDemo", "heatmap_args"]

HEATMAP_KEYS = ("kind", "slot", "lut", "alpha", "alpha_mode")


def heatmap_args(heatmap, who="heatmap"):
    """A heatmap= argument -- a kind ("objectness", "attention", "<buffer>[:<channel>]") or a dict with "kind" and any of slot, lut,
    alpha, alpha_mode -- as the checked keyword set {kind, slot, lut, alpha, alpha_mode}; None stays None.  Everything that can be
    refused without an engine is refused here (ValueError): the kind's form, the table, alpha, the slot's type."""
    import orehip
    if heatmap is None:
        return None
    kw = {"slot": 0, "lut": "jet", "alpha": 128, "alpha_mode": "constant"}
    if isinstance(heatmap, str):
        kw["kind"] = heatmap
    elif isinstance(heatmap, dict):
        unknown = sorted(set(heatmap) - set(HEATMAP_KEYS), key=str)
        if unknown or "kind" not in heatmap:
            raise ValueError(f"{who}: a dict takes {', '.join(HEATMAP_KEYS)} (kind is needed); not {', '.join(map(str, unknown)) or 'one without kind'}")
        kw.update(heatmap)
    else:
        raise ValueError(f"{who}: None, a kind or a dict of {', '.join(HEATMAP_KEYS)}")
    try:
        orehip.heat_kind(kw["kind"])
        orehip._heatmap_style(kw["alpha"], kw["alpha_mode"])
        kw["lut"] = kw["lut"] if isinstance(kw["lut"], str) and kw["lut"] in orehip.HEATMAP_LUTS else orehip.heatmap_lut(kw["lut"])
    except orehip.OreError as err:
        raise ValueError(f"{who}: {err}") from err
    if isinstance(kw["slot"], bool) or not isinstance(kw["slot"], (int, np.integer)) or kw["slot"] < 0:
        raise ValueError(f"{who}: slot {kw['slot']!r} is a non-negative integer")
    return kw


def _heatmap_fits(kw, engine, who):
    """What of a checked heatmap= needs the engine: the channel exists, the slot is a class slot of the pass.  Host only."""
    import orehip
    what = orehip.heat_kind(kw["kind"])
    ch = engine.buffer_dims(what["buffers"][0])[2]
    if what["channel"] != "mean" and what["channel"] >= ch:
        raise ValueError(f"{who}: {kw['kind']!r}: the buffer has {ch} channels")
    slots = len(getattr(engine, "class_ids", None) or ()) or 1
    if kw["slot"] >= slots:
        raise ValueError(f"{who}: slot {kw['slot']}: the pass has {slots} class slot(s)")


def _draw_heatmap(frame, engine, kw, out=None):
    """The heat map of the engine's last pass over a BGR device frame, on the current stream."""
    import orehip
    return orehip.heatmap_draw(frame, engine.heat_source(kw["kind"], kw["slot"]), out=out, lut=kw["lut"], alpha=kw["alpha"],
                               alpha_mode=kw["alpha_mode"], channel_order="BGR")


class TiledPredictor:
    """DefaultPredictor's contract with sliced inference behind it:

        pred = TiledPredictor(cfg, tile=(640, 640), overlap=128)
        outputs = pred(bgr_frame)          # {"instances": Instances} at the frame's own size

    builds the model as DefaultPredictor does (cfg.MODEL.WEIGHTS, the metadata of cfg.DATASETS.TEST[0]) and wraps it in
    fewx.modeling.TiledInference(cfg, model, **tiling).  The frame is BGR [h, w, 3] uint8 (numpy array, CPU or device tensor);
    cfg.INPUT.FORMAT == "RGB" exchanges the channels on the device.  track=True (or an orehip tracker) follows the merged detections
    across the frames in the order of the calls: outputs["instances"].track_ids, and track_stats() counts the tracks started.
    rectify=orehip.Rectifier(...) warps the uploaded frame into the rectifier's plane in front of the tile gather (contract "rectify
    v1"): the tiles are cut from the rectified frame and the Instances are at rectify.out_hw."""

    def __init__(self, cfg, track=None, rectify=None, **tiling):
        from fewx.modeling import TiledInference
        self.predictor = DefaultPredictor(cfg, rectify=rectify)
        self.cfg, self.model = self.predictor.cfg, self.predictor.model
        self.metadata = getattr(self.predictor, "metadata", None)
        self.input_format = self.predictor.input_format
        self.tiled = TiledInference(self.cfg, self.model, track=track, **tiling)

    def track_stats(self):
        """TiledInference.track_stats(): tracks, started (the particle count), frames, dropped.  One host sync."""
        return self.tiled.track_stats()

    def __call__(self, original_image):
        if self.predictor.rectify is not None:                # upload and warp in front of the tile gather
            original_image = self.predictor._rectified(original_image)
        return self.tiled([{"image_raw": original_image, "swap_rb": self.input_format == "RGB"}])[0]


class _Slot:
    """One frame's worth of machinery: an engine, its stream, a pinned staging buffer, the event behind the frame's last kernel."""
    __slots__ = ("engine", "stream", "stage", "event", "count")


class _Pass:
    """A frame between `put` and `get`."""
    __slots__ = ("slot", "rec", "raw", "vis", "hw", "ids")


class AsyncPredictor:
    """A predictor that runs frames asynchronously: `put(image)` enqueues one BGR frame ([h, w, 3] uint8: numpy array, CPU tensor or
    device tensor), `get()` returns the oldest frame's {"instances": Instances} -- results come back in `put` order.  `predictor(image)`
    is put + get.  One process, no workers and no threads: `inflight` engines (model.make_engine()), each with its own HIP stream,
    pinned staging buffer and result record.  `put` enqueues upload, device resize and the detection pass on the next slot's stream and
    returns; when every slot is busy it first completes the oldest pass.  `get` performs the frame's one host wait.

    put(image, draw=True) -- or draw={overlay_draw keyword arguments} -- also enqueues the detection overlay behind the pass, on the
    same stream, reading the pass's record and its device-side count: the result then carries "vis_image", the annotated frame on the
    device in the input's channel order (BGR), still with one host wait per frame.  put(image, heatmap=kind) -- or a dict, see
    heatmap_args -- enqueues a heat map of the pass behind it, before the overlay: "vis_image" then shows the heat map with the boxes
    (if drawn) on top.  put(image, track=tracker) -- an orehip.BoxTracker on the model's device, the caller's -- enqueues the tracker's
    update behind the pass, on the same stream, on the pending record and the device-side count: the result's Instances then carries
    track_ids, and a drawn frame is coloured and labelled by them (color_by "track") unless draw says otherwise.  The tracker orders
    its updates across the slots' streams on the device, so the frames are associated in `put` order with the passes still overlapping.
    put(image, rectify=R) -- an orehip.Rectifier -- warps the frame into R's plane behind the slot's upload, on the slot's stream
    (contract "rectify v1", one launch): the pass, the heat map, the tracker and the overlay see the rectified frame, the Instances and
    "vis_image" are at R.out_hw, and there is still one host wait per frame.

    1 <= inflight <= 4: a process opens 4 hardware queues by default, and this class does not ask for more.  num_gpus must be 1: one
    process per device is a launcher's job.  The engines are keyed like model.engine(): a `put` that finds the weights or the support
    set changed completes what is pending, then rebuilds them."""

    MAX_INFLIGHT = 4

    def __init__(self, cfg, num_gpus: int = 1, inflight: int = 4):
        if num_gpus != 1:
            raise ValueError(f"AsyncPredictor: num_gpus {num_gpus}: one process drives one device (start one process per GPU)")
        if not isinstance(inflight, int) or not 1 <= inflight <= self.MAX_INFLIGHT:
            raise ValueError(f"AsyncPredictor: inflight {inflight} outside 1 .. {self.MAX_INFLIGHT} (the hardware queues of one process)")
        self.inflight = inflight
        self.predictor = DefaultPredictor(cfg)            # the one-image predictor over the same model
        self.cfg, self.model = self.predictor.cfg, self.predictor.model
        self.metadata = getattr(self.predictor, "metadata", None)
        self.input_format = self.predictor.input_format
        self._slots, self._key = [], None
        self._pending, self._done = deque(), deque()
        self._next = 0

    # ---- engines ------------------------------------------------------------------------------------------------
    def _close_engines(self):
        for s in self._slots:
            s.engine.close()
        self._slots, self._key = [], None

    def _ensure_engines(self):
        m = self.model
        m.init_model()
        key = m._engine_key_now()
        if self._key == key and self._slots:
            return
        while self._pending:                                  # passes of the old engines finish on the old engines
            self._done.append(self._complete(self._pending.popleft()))
        self._close_engines()
        dev = m.device
        with torch.cuda.device(dev):
            for _ in range(self.inflight):
                s = _Slot()
                s.engine = m.make_engine(classes=key[3])
                if not getattr(s.engine, "has_roi", False):
                    s.engine.close()
                    self._close_engines()
                    raise ValueError("AsyncPredictor needs the second stage inside the engine (a support set with rcnn_8 features)")
                s.stream = torch.cuda.Stream(device=dev)
                s.stage, s.event = None, torch.cuda.Event()
                s.count = s.engine.buffer("final_count").view(torch.int32).reshape(-1)[:1]
                self._slots.append(s)
        self._key, self._next = key, 0

    # ---- put / get ----------------------------------------------------------------------------------------------
    DRAW_KEYS = ("score_thresh", "line_width", "text_scale", "edge_alpha", "label_alpha", "palette", "color_by", "names")

    def _draw_args(self, draw, h, w, tracked=False):
        """The overlay's keyword arguments of one frame, checked here, before anything of the frame is enqueued: what can be
        refused on the host is refused while the slot's engine is still idle."""
        import orehip
        kw = dict(default_overlay_params(h, w), names=thing_classes(self.metadata), color_by="track" if tracked else "instance",
                  palette=np.ascontiguousarray(orehip.OVERLAY_PALETTE[:, ::-1]))           # the frame is BGR
        if isinstance(draw, dict):
            unknown = sorted(set(draw) - set(self.DRAW_KEYS))
            if unknown:
                raise ValueError(f"AsyncPredictor.put: draw takes {', '.join(self.DRAW_KEYS)}; not {', '.join(map(str, unknown))}")
            kw.update(draw)
        elif draw is not True:
            raise ValueError("AsyncPredictor.put: draw is True or a dict of overlay_draw keyword arguments")
        if not (1 <= int(kw["line_width"]) <= 16 and 0 <= int(kw["text_scale"]) <= 8 and 0 <= int(kw.get("edge_alpha", 0)) <= 255
                and 0 <= int(kw.get("label_alpha", 0)) <= 255):
            raise ValueError("AsyncPredictor.put: line_width 1 .. 16, text_scale 0 .. 8, alphas 0 .. 255")
        kw["palette"] = orehip._overlay_palette(kw["palette"])
        if orehip._overlay_color_by(kw["color_by"], has_ids=False) == 2 and not tracked:
            raise ValueError('AsyncPredictor.put: color_by "track" needs track=')
        return kw

    @torch.no_grad()
    def put(self, image, draw=None, heatmap=None, track=None, rectify=None):
        import orehip
        if isinstance(image, np.ndarray):
            image = torch.from_numpy(np.ascontiguousarray(image))
        if not torch.is_tensor(image) or image.dim() != 3 or image.shape[2] != 3 or image.dtype != torch.uint8:
            raise ValueError("AsyncPredictor.put takes an [h, w, 3] uint8 BGR image")
        h, w = int(image.shape[0]), int(image.shape[1])
        if rectify is not None and not isinstance(rectify, orehip.Rectifier):
            raise ValueError("AsyncPredictor.put: rectify is an orehip.Rectifier")
        oh, ow = (h, w) if rectify is None else rectify.out_hw     # the size everything behind the upload sees
        if track is not None and not (isinstance(track, orehip.BoxTracker) and track.device == torch.device(self.model.device)):
            raise ValueError("AsyncPredictor.put: track is an orehip.BoxTracker on the model's device")
        try:
            draw_kw = self._draw_args(draw, oh, ow, track is not None) if draw else None
        except orehip.OreError as err:
            raise ValueError(f"AsyncPredictor.put: {err}") from err
        heat_kw = heatmap_args(heatmap, "AsyncPredictor.put: heatmap")
        self._ensure_engines()                                # rebuilds engines if need be; a tracker is the caller's and stays as it is
        if heat_kw is not None:
            _heatmap_fits(heat_kw, self._slots[self._next].engine, "AsyncPredictor.put: heatmap")
        if len(self._pending) == len(self._slots):
            self._done.append(self._complete(self._pending.popleft()))
        slot = self._slots[self._next]                        # completion is first in, first out: the next slot in turn is free
        m, e = self.model, slot.engine
        p = _Pass()
        p.slot, p.hw, p.vis, p.ids = slot, (oh, ow), None, None
        if image.is_cuda:                                     # the frame was produced on the caller's stream: the slot's stream follows it
            slot.stream.wait_stream(torch.cuda.current_stream(image.device))
        with torch.cuda.device(m.device), torch.cuda.stream(slot.stream):
            if image.is_cuda:
                raw = image.to(m.device).contiguous()
                ours = raw.data_ptr() != image.data_ptr()
                if not ours:
                    image.record_stream(slot.stream)
            else:
                n = h * w * 3
                if slot.stage is None or slot.stage.numel() < n:
                    slot.stage = torch.empty(max(n, 1 << 20), dtype=torch.uint8, pin_memory=True)
                stage = slot.stage[:n].view(h, w, 3)
                stage.copy_(image)                            # the slot's previous upload finished with its pass
                raw, ours = torch.empty(h, w, 3, dtype=torch.uint8, device=m.device), True
                raw.copy_(stage, non_blocking=True)
            if rectify is not None:                           # one more launch behind the upload: the slot's own tensor from here on
                raw, ours = rectify(raw), True
            nh, nw = orehip.resize_shortest_edge_shape(oh, ow, m._test_size[0], m._test_size[1])
            img = orehip.resize_bilinear_u8(raw, nh, nw, swap_rb=self.input_format == "RGB")
            p.rec = e.detect_classes_begin(img, oh, ow) if getattr(e, "class_ids", None) else e.detect_begin(img, oh, ow)
            p.raw = raw
            try:                                              # in place on the slot's own upload; a caller's device frame is left as it was
                if heat_kw is not None:
                    p.vis = _draw_heatmap(raw, e, heat_kw, out=raw if ours else None)
                    ours = True                               # the picture so far is this frame's own: the boxes go onto it in place
                if track is not None or draw_kw is not None:
                    R = e._rec_rows
                    boxes, scores, classes = orehip.record_views(p.rec, R, R)
                if track is not None:                         # the one launch behind the pass: every check that can refuse is behind us
                    p.ids = track.update(boxes, scores, classes, slot.count)
                if draw_kw is not None:
                    base = raw if p.vis is None else p.vis
                    p.vis = orehip.overlay_draw(base, boxes, scores, classes, slot.count, out=base if ours else None, ids=p.ids, **draw_kw)
            except BaseException:
                e.detect_end(p.rec)                           # the pass has begun: end it, so that the engine is free for the next put
                raise
            slot.event.record(slot.stream)
        self._pending.append(p)
        self._next = (self._next + 1) % len(self._slots)      # only now: a put that raised leaves its slot the next in turn

    def _complete(self, p):
        """The one host wait of a frame -- the event behind its last kernel -- then the record is cut at the count."""
        from detectron2.structures import Boxes, Instances
        slot = p.slot
        p.slot.event.synchronize()
        with torch.cuda.device(self.model.device), torch.cuda.stream(slot.stream):
            boxes, scores, classes = slot.engine.detect_end(p.rec)      # the count word is there: no second wait
        cur = torch.cuda.current_stream(self.model.device)
        p.rec.record_stream(cur)                              # allocated on the slot's stream, used from here on on the caller's
        res = Instances(p.hw)
        res.pred_boxes = Boxes(boxes)
        res.scores = scores
        res.pred_classes = classes
        if p.ids is not None:
            p.ids.record_stream(cur)
            res.track_ids = p.ids[:len(scores)]
        out = {"instances": res}
        if p.vis is not None:
            p.vis.record_stream(cur)
            out["vis_image"] = p.vis
        return out

    def get(self):
        if self._done:
            return self._done.popleft()
        if not self._pending:
            raise IndexError("AsyncPredictor.get: nothing was put")
        return self._complete(self._pending.popleft())

    def __len__(self):
        return len(self._pending) + len(self._done)

    def __call__(self, image, track=None, rectify=None):
        self.put(image, track=track, rectify=rectify)
        return self.get()

    def shutdown(self):
        while self._pending:
            self._complete(self._pending.popleft())
        self._done.clear()
        self._close_engines()

    @property
    def default_buffer_size(self):
        return self.inflight


class VisualizationDemo:
    """VisualizationDemo(cfg, instance_mode=ColorMode.IMAGE, parallel=False) (ref:predictor.py): run_on_image(bgr) -> (predictions,
    VisImage); run_on_video(frames) -> annotated BGR frames.  parallel=True predicts through an AsyncPredictor, which also draws.
    heatmap=kind -- "objectness", "attention", "<buffer>[:<channel>]", or a dict (heatmap_args) -- lays that heat map of the detection
    pass under the boxes; None (the default) draws the boxes alone.  track=True follows the detections across the frames of
    run_on_video (an orehip.BoxTracker, reset at the start of every call): ids that persist, boxes coloured and labelled by them;
    track_stats() then counts the tracks started.  track="belt" is the same with an orehip.BeltTracker, for a scene that moves as one
    (a conveyor belt): the frame's shift is voted and the tracks are moved by it in front of every update, `belt` holds BeltTracker
    keywords (bin, radius, ...), the tracker's frame is the size of each video's first frame, and track_stats() adds "shift", "travel",
    "votes" and "coasted".  run_on_image ignores it.  rectify=orehip.Rectifier(...): every frame is warped into the rectifier's plane
    behind its upload (contract "rectify v1"); predictions and drawn frames are at rectify.out_hw, which is also a belt tracker's frame."""

    def __init__(self, cfg, instance_mode=ColorMode.IMAGE, parallel=False, heatmap=None, track=False, belt=None, rectify=None):
        import orehip
        self.heatmap = heatmap_args(heatmap, "VisualizationDemo: heatmap")
        if rectify is not None and not isinstance(rectify, orehip.Rectifier):
            raise ValueError("VisualizationDemo: rectify is None or an orehip.Rectifier")
        self.rectify = rectify
        if isinstance(track, str) and track != "belt":
            raise ValueError(f'VisualizationDemo: track is False, True or "belt", got {track!r}')
        if belt is not None and track != "belt":
            raise ValueError('VisualizationDemo: belt= goes with track="belt"')
        self.track, self.tracker = bool(track), None
        self.track_motion, self.belt = ("belt" if track == "belt" else None), dict(belt or {})
        if instance_mode not in (ColorMode.IMAGE, ColorMode.SEGMENTATION):
            raise NotImplementedError(f"VisualizationDemo: {instance_mode} needs instance masks; boxes only")
        self.instance_mode, self.parallel = instance_mode, bool(parallel)
        self.predictor = AsyncPredictor(cfg) if self.parallel else DefaultPredictor(cfg)
        # the class names drawn into the labels: those of the first test dataset, as the predictor itself resolves them
        self.metadata = getattr(self.predictor, "metadata", None)
        if self.metadata is None:
            self.metadata = MetadataCatalog.get("demo")

    def _upload(self, image):
        """The BGR frame on the model's device, once: the detector and the overlay both read it there."""
        import orehip
        if isinstance(image, np.ndarray):
            image = torch.from_numpy(np.ascontiguousarray(image))
        frame = orehip.to_device(image, self.predictor.model.device).contiguous()
        if self.rectify is not None:
            with torch.cuda.device(frame.device):
                frame = self.rectify(frame)
        return frame

    def run_on_image(self, image):
        """image: [h, w, 3] uint8 in BGR order.  Returns the model's predictions and the drawn VisImage."""
        color_by = "class" if self.instance_mode == ColorMode.SEGMENTATION else "instance"
        if self.parallel:
            self.predictor.put(image, draw={"color_by": color_by}, heatmap=self.heatmap, rectify=self.rectify)
            out = self.predictor.get()
            return {"instances": out["instances"]}, VisImage(out["vis_image"], "BGR")
        frame = self._upload(image)
        predictions = self.predictor(frame)
        frame = self._heat(frame)
        vis = Visualizer(frame, self.metadata, instance_mode=self.instance_mode, channel_order="BGR")
        return predictions, vis.draw_instance_predictions(predictions["instances"])

    def _heat(self, frame):
        """The frame with the heat map of the pass the predictor has just run (a new tensor), or the frame itself without one."""
        if self.heatmap is None:
            return frame
        import orehip
        who = "VisualizationDemo: heatmap"
        engine_of = getattr(self.predictor.model, "engine", None)
        if not callable(engine_of):
            raise ValueError(f"{who}: this model has no engine whose pass could be drawn")
        engine = engine_of()                                  # the engine of the current weights and support set: the one the call ran on
        _heatmap_fits(self.heatmap, engine, who)
        try:
            return _draw_heatmap(frame, engine, self.heatmap)
        except orehip.OreError as err:                        # e.g. the engine has not run a pass
            raise ValueError(f"{who}: {err}") from err

    def _tracker(self):
        """The demo's tracker on the model's device, built on first use and empty at the start of every video."""
        import orehip
        if self.tracker is None:
            if self.track_motion == "belt":
                self.tracker = orehip.BeltTracker(self.predictor.model.device, **self.belt)
            else:
                self.tracker = orehip.BoxTracker(self.predictor.model.device)
        else:
            self.tracker.reset()
        return self.tracker

    def _framed(self, frames, tracker):
        """The frames as they come; a belt tracker learns the size of the first one (rectified: out_hw) before it is used."""
        first = True
        for frame in frames:
            if first:
                tracker.set_frame(self.rectify.out_hw if self.rectify is not None else tuple(int(v) for v in frame.shape[:2]))
            first = False
            yield frame

    def track_stats(self):
        """BoxTracker.stats() of the last run_on_video: tracks, started (the particle count), frames, dropped (track="belt": and shift,
        travel, votes, coasted).  One host sync."""
        if self.tracker is None:
            return {"tracks": 0, "started": 0, "frames": 0, "dropped": 0}
        return self.tracker.stats()

    @staticmethod
    def _frames(source):
        """A generator over the frames of `source`: an iterable as it is; a capture-like object (isOpened() / read() returning
        (ok, frame), the shape of cv2.VideoCapture) is polled until it closes or a read fails."""
        if not (callable(getattr(source, "isOpened", None)) and callable(getattr(source, "read", None))):
            yield from source
            return
        more = source.isOpened()
        while more:
            more, frame = source.read()
            if more:
                yield frame
                more = source.isOpened()

    def run_on_video(self, video):
        """video: an iterable of BGR frames, or an object with isOpened() / read().  Yields the annotated BGR frames ([h, w, 3] uint8
        numpy), in order; parallel=True keeps AsyncPredictor.default_buffer_size frames in flight."""
        frames = self._frames(video)
        tracker = None
        if self.track:
            tracker = self._tracker()
            if self.track_motion == "belt":
                frames = self._framed(frames, tracker)
        if self.parallel:
            draw = {"color_by": "track" if tracker is not None else "class"}
            pending = 0
            for frame in frames:
                if pending == self.predictor.default_buffer_size:
                    yield self.predictor.get()["vis_image"].cpu().numpy()
                    pending -= 1
                self.predictor.put(frame, draw=draw, heatmap=self.heatmap, track=tracker, rectify=self.rectify)
                pending += 1
            while pending:
                yield self.predictor.get()["vis_image"].cpu().numpy()
                pending -= 1
        else:
            video_visualizer = VideoVisualizer(self.metadata, self.instance_mode, channel_order="BGR", track=tracker if tracker is not None else False)
            for frame in frames:
                dev = self._upload(frame)
                predictions = self.predictor(dev)
                yield video_visualizer.draw_instance_predictions(self._heat(dev), predictions["instances"]).img.cpu().numpy()
