"""Test-time augmentation (d2z:modeling/test_time_augmentation.py DatasetMapperTTA, GeneralizedRCNNWithTTA): one image is detected at
every TEST.AUG.MIN_SIZES scale, plain and horizontally flipped, the detections go back to the output frame and ONE class-aware NMS
merges them (d2z:modeling/roi_heads/fast_rcnn.py fast_rcnn_inference_single_image).

With the default mapper the whole image stays on the device: one upload, the resized variants (orehip.resize_bilinear_u8, the bytes
of Pillow's BILINEAR; a flipped variant is a column-reversed copy of its sibling), one engine replay per variant with the rows
collected behind it (ore_tta_collect_fwd: inverse transform, appended at a device-side offset) and one merge (ore_tta_merge_fwd), all
queued on the current stream; the host waits once, for the merged count.  With support_classes set (N-way) the engine's merged rows
exist only in the record of a finished pass, so the host polls once per variant.

The functions of this file that work on numpy arrays are the host statement of that arithmetic; the kernels are held to them bit for
bit (tests/test_tta_host.py, tests/test_hip_tta.py)."""
import copy

import numpy as np
import torch
from torch import nn

__all__ = ["DatasetMapperTTA", "GeneralizedRCNNWithTTA"]

RESIZE_MAX_SIDE = 8192                     # ORE_RESIZE_MAX_SIDE (csrc/ore_resize_internal.h)
DETECT_MAX_LOCATIONS = 30720               # locations of the stride-8 level the detection tail caches in LDS (csrc/ore_detect.hip)
SCORE_THRESH = 1e-8                        # _merge_detections: fast_rcnn_inference_single_image(..., 1e-8, nms_thresh, topk)


# ------------------------------------------------------------------------------------------ variants and transforms (host)
def tta_variants(h, w, min_sizes, max_size, flip):
    """The variant list of DatasetMapperTTA for an [h, w] source, in its order: for every min_size `[resize]` and then, with flip,
    `[resize, flip]`.  Each entry: dict(min_size, h, w, flip), (h, w) = ResizeShortestEdge(min_size, max_size) of the source."""
    import orehip
    out = []
    for ms in min_sizes:
        nh, nw = orehip.resize_shortest_edge_shape(int(h), int(w), int(ms), int(max_size))
        out.append({"min_size": int(ms), "h": nh, "w": nw, "flip": False})
        if flip:
            out.append({"min_size": int(ms), "h": nh, "w": nw, "flip": True})
    return out


def variant_transforms(out_hw, img_hw, var):
    """The transform chain of one variant as DatasetMapperTTA records it -- pre-resize (output frame -> the mapper-resized image; left
    out when they agree), resize, flip -- as plain tuples: ("resize", h, w, new_h, new_w) / ("hflip", width)."""
    t = []
    if tuple(out_hw) != tuple(img_hw):
        t.append(("resize", int(out_hw[0]), int(out_hw[1]), int(img_hw[0]), int(img_hw[1])))
    t.append(("resize", int(img_hw[0]), int(img_hw[1]), int(var["h"]), int(var["w"])))
    if var["flip"]:
        t.append(("hflip", int(var["w"])))
    return tuple(t)


def _apply_box(boxes, apply_coords):
    """Transform.apply_box (fvcore transforms/transform.py): the four corners through apply_coords, then min / max."""
    idxs = np.array([(0, 1), (2, 1), (0, 3), (2, 3)]).flatten()
    coords = np.asarray(boxes).reshape(-1, 4)[:, idxs].reshape(-1, 2)
    coords = apply_coords(coords).reshape((-1, 4, 2))
    return np.concatenate((coords.min(axis=1), coords.max(axis=1)), axis=1)


def inverse_boxes(boxes, transforms):
    """`tfm.inverse().apply_box(boxes)` on a float32 array for a chain of variant_transforms: the inverses in reverse order, each an
    apply_box of its own.  HFlipTransform.apply_coords: x = width - x; ResizeTransform(h, w, new_h, new_w).inverse() =
    ResizeTransform(new_h, new_w, h, w), whose apply_coords multiplies x by float32(w * 1.0 / new_w) and y by float32(h * 1.0 / new_h)
    -- separately rounded fp32 operations, the ratio computed in double."""
    boxes = np.ascontiguousarray(boxes, dtype=np.float32).reshape(-1, 4)
    for t in reversed(tuple(transforms)):
        if t[0] == "hflip":
            width = np.float32(t[1])

            def f(c, width=width):
                c = c.copy()
                c[:, 0] = width - c[:, 0]
                return c
        elif t[0] == "resize":
            _, h, w, nh, nw = t
            rx, ry = np.float32(w * 1.0 / nw), np.float32(h * 1.0 / nh)

            def f(c, rx=rx, ry=ry):
                c = c.copy()
                c[:, 0] = c[:, 0] * rx
                c[:, 1] = c[:, 1] * ry
                return c
        else:
            raise ValueError(f"unknown transform {t!r}")
        boxes = _apply_box(boxes, f).astype(np.float32)
    return boxes


def _collect_params(transforms):
    """The arguments of ore_tta_collect_fwd for a chain of variant_transforms: dict(flip, variant_w, sx, sy, pre)."""
    t = list(transforms)
    flip = t[-1][0] == "hflip"
    if flip:
        vw = t.pop()[1]
    if not 1 <= len(t) <= 2 or any(x[0] != "resize" for x in t):
        raise ValueError(f"not a TTA chain (pre-resize, resize, flip): {transforms!r}")
    _, h, w, nh, nw = t[-1]
    pre = None
    if len(t) == 2:
        _, oh, ow, ih, iw = t[0]
        pre = (ow * 1.0 / iw, oh * 1.0 / ih)
    return dict(flip=flip, variant_w=vw if flip else nw, sx=w * 1.0 / nw, sy=h * 1.0 / nh, pre=pre)


def nms_numpy(boxes, scores, thr):
    """Greedy NMS in fp32 with the operation order of ore_nms_fwd / oracle/ref_decode.c: stable descending sort, suppress j when
    inter / (area_i + area_j - inter) > thr.  Returns the kept indices in that order."""
    boxes, scores = np.asarray(boxes, np.float32).reshape(-1, 4), np.asarray(scores, np.float32)
    order = np.argsort(-scores, kind="stable")
    area = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    dead = np.zeros(len(scores), bool)
    keep = []
    for a, i in enumerate(order):
        if dead[i]:
            continue
        keep.append(int(i))
        rest = order[a + 1:]
        xx1, yy1 = np.maximum(boxes[i, 0], boxes[rest, 0]), np.maximum(boxes[i, 1], boxes[rest, 1])
        xx2, yy2 = np.minimum(boxes[i, 2], boxes[rest, 2]), np.minimum(boxes[i, 3], boxes[rest, 3])
        inter = np.maximum(np.float32(0), xx2 - xx1) * np.maximum(np.float32(0), yy2 - yy1)
        with np.errstate(invalid="ignore", divide="ignore"):
            ovr = inter / (area[i] + area[rest] - inter)
        dead[rest[ovr > np.float32(thr)]] = True
    return np.asarray(keep, dtype=np.int64)


def merge_detections_host(boxes, scores, classes, out_hw, score_thresh, nms_thresh, topk, nms=nms_numpy):
    """fast_rcnn_inference_single_image as GeneralizedRCNNWithTTA._merge_detections calls it, on numpy arrays: rows with a non-finite
    value dropped, boxes clipped to out_hw, score > score_thresh, NMS per class id on the true coordinates, the survivors by score
    descending (equal scores in candidate order), the first topk.  Returns (boxes, scores, classes, candidate index of every row)."""
    boxes = np.ascontiguousarray(boxes, np.float32).reshape(-1, 4)
    scores, classes = np.asarray(scores, np.float32).reshape(-1), np.asarray(classes, np.int64).reshape(-1)
    h, w = np.float32(out_hw[0]), np.float32(out_hw[1])
    cand = np.nonzero(np.isfinite(boxes).all(1) & np.isfinite(scores))[0]
    b = boxes[cand].copy()
    b[:, 0::2] = np.minimum(np.maximum(b[:, 0::2], np.float32(0)), w)
    b[:, 1::2] = np.minimum(np.maximum(b[:, 1::2], np.float32(0)), h)
    live = scores[cand] > np.float32(score_thresh)
    cand, b = cand[live], b[live]
    s, c = scores[cand], classes[cand]
    kept = []
    for cls in np.unique(c):
        idx = np.nonzero(c == cls)[0]
        kept.extend(idx[np.asarray(nms(np.ascontiguousarray(b[idx]), np.ascontiguousarray(s[idx]), nms_thresh), dtype=np.int64)].tolist())
    kept = np.asarray(sorted(kept, key=lambda i: (-float(s[i]), i))[:int(topk)], dtype=np.int64)
    return b[kept], s[kept], c[kept], cand[kept]


def check_variant_limits(src_hw, variants):
    """ValueError for a variant list the device cannot run, before any GPU work: a resize side beyond 8192, or a variant whose stride-8
    pyramid level has more locations than the detection tail caches (30720)."""
    h, w = src_hw
    if not (1 <= h <= RESIZE_MAX_SIDE and 1 <= w <= RESIZE_MAX_SIDE):
        raise ValueError(f"TTA: source image {h}x{w}: the device resize takes sides 1 .. {RESIZE_MAX_SIDE}")
    big = [v for v in variants if max(v["h"], v["w"]) > RESIZE_MAX_SIDE]
    if big:
        raise ValueError("TTA: variant(s) %s of a %dx%d image exceed the device resize's largest side %d" %
                         (", ".join("%dx%d (min_size %d)" % (v["h"], v["w"], v["min_size"]) for v in big), h, w, RESIZE_MAX_SIDE))
    loc = lambda v: ((v["h"] + 31) // 32 * 4) * ((v["w"] + 31) // 32 * 4)
    big = [v for v in variants if not v["flip"] and loc(v) > DETECT_MAX_LOCATIONS] or [v for v in variants if loc(v) > DETECT_MAX_LOCATIONS]
    if big:
        raise ValueError("TTA: variant(s) %s of a %dx%d image exceed the detection tail's %d stride-8 locations per image; lower "
                         "TEST.AUG.MIN_SIZES / TEST.AUG.MAX_SIZE" %
                         (", ".join("%dx%d (min_size %d: %d locations)" % (v["h"], v["w"], v["min_size"], loc(v)) for v in big), h, w,
                          DETECT_MAX_LOCATIONS))


# ------------------------------------------------------------------------------------------ the mapper
class DatasetMapperTTA:
    """d2z:modeling/test_time_augmentation.py DatasetMapperTTA: a dataset dict with "image" (CHW uint8) -> one dict per variant with
    "image" (CHW uint8 tensor: ResizeShortestEdge through Pillow BILINEAR, columns reversed for a flipped variant) and "transforms"
    (variant_transforms: plain tuples, picklable).  DatasetMapperTTA(cfg) reads TEST.AUG; DatasetMapperTTA(min_sizes, max_size, flip)
    is detectron2's other signature."""

    def __init__(self, cfg_or_min_sizes, max_size=None, flip=None):
        if hasattr(cfg_or_min_sizes, "TEST"):
            aug = cfg_or_min_sizes.TEST.AUG
            min_sizes, max_size, flip = aug.MIN_SIZES, aug.MAX_SIZE, aug.FLIP
        else:
            min_sizes = cfg_or_min_sizes
            if max_size is None or flip is None:
                raise TypeError("DatasetMapperTTA(cfg) or DatasetMapperTTA(min_sizes, max_size, flip)")
        self.min_sizes, self.max_size, self.flip = tuple(int(s) for s in min_sizes), int(max_size), bool(flip)
        if not self.min_sizes:
            raise ValueError("DatasetMapperTTA: TEST.AUG.MIN_SIZES is empty")

    def variants(self, h, w):
        return tta_variants(h, w, self.min_sizes, self.max_size, self.flip)

    def __call__(self, dataset_dict):
        from PIL import Image
        image = dataset_dict["image"]
        image = image.cpu().numpy() if torch.is_tensor(image) else np.asarray(image)
        if image.dtype != np.uint8 or image.ndim != 3:
            raise ValueError(f"DatasetMapperTTA takes a CHW uint8 image, got {image.shape} {image.dtype}")
        hwc = np.ascontiguousarray(image.transpose(1, 2, 0))
        img_hw = hwc.shape[:2]
        out_hw = (int(dataset_dict.get("height", img_hw[0])), int(dataset_dict.get("width", img_hw[1])))
        ret = []
        for var in self.variants(*img_hw):
            new = np.asarray(Image.fromarray(hwc).resize((var["w"], var["h"]), Image.BILINEAR))
            if var["flip"]:
                new = new[:, ::-1]
            dic = copy.copy(dataset_dict)
            dic["transforms"] = variant_transforms(out_hw, img_hw, var)
            dic["image"] = torch.from_numpy(np.ascontiguousarray(new.transpose(2, 0, 1)))
            ret.append(dic)
        return ret


# ------------------------------------------------------------------------------------------ the wrapper
class _Pending:
    """One image between `_enqueue` and `_finish`: the result record, its device count and the output size."""
    __slots__ = ("rec", "count", "rows", "out_hw", "pool")


class GeneralizedRCNNWithTTA(nn.Module):
    """d2z:modeling/test_time_augmentation.py GeneralizedRCNNWithTTA for the CenterNet2Detector of this package (box detections only:
    MASK_ON / KEYPOINT_ON are false in every fsod config).  `__call__(batched_inputs)` takes the model's request dicts -- "image" (+
    "height" / "width"), "image_raw", or "file_name" (read as `_maybe_read_image` does) -- and returns [{"instances": Instances}] with
    pred_boxes / scores / pred_classes in the (height, width) frame.

    Per variant the rows are what `model.inference([{"image": variant}], do_postprocess=False)` returns (`_batch_inference`), taken
    back by `tfm.inverse().apply_box` (`_get_augmented_boxes`) and merged by fast_rcnn_inference_single_image with score threshold
    1e-8, MODEL.ROI_HEADS.NMS_THRESH_TEST and TEST.DETECTIONS_PER_IMAGE (`_merge_detections`).  Variants of an "image" request are
    resized from that image with the pre-transform in the chain (DatasetMapperTTA.__call__); an "image_raw" / "file_name" request is
    resized straight from the raw image.  tta_mapper=None takes the device path (module docstring); a custom mapper the host path:
    mapper -> model per variant -> host inverse -> the merge kernel.  batch_size is accepted and ignored: a pass holds one query image.
    The wrapper owns one engine sized for its largest variant; the model's own cached engine is left alone."""

    def __init__(self, cfg, model, tta_mapper=None, batch_size=3):
        super().__init__()
        from fewx.modeling.fsod.fsod_cen import CenterNet2Detector
        while not isinstance(model, CenterNet2Detector) and isinstance(getattr(model, "module", None), nn.Module):
            model = model.module                              # FlatDataParallel / DistributedDataParallel
        if not isinstance(model, CenterNet2Detector):
            raise TypeError(f"GeneralizedRCNNWithTTA wraps a CenterNet2Detector, not {type(model).__name__}")
        self.cfg = cfg.clone()
        self.model = model
        self.device_path = tta_mapper is None
        self.tta_mapper = DatasetMapperTTA(cfg) if tta_mapper is None else tta_mapper
        self.batch_size = batch_size
        self.nms_thresh = float(cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST)
        self.topk = int(cfg.TEST.DETECTIONS_PER_IMAGE)
        self._tta_engine = None
        self._tta_engine_key = None
        self._tta_engine_hw = (0, 0)
        self._pools = {}

    # ---- engine -------------------------------------------------------------------------------------------------
    def _engine(self, need_hw, what=""):
        """The wrapper's engine: rebuilt when the model's engine key changes (weights, support set, device, precision, class
        selection) or a variant needs more room than it has."""
        import orehip
        m = self.model
        key = m._engine_key_now()
        have = self._tta_engine_hw
        if self._tta_engine is None or self._tta_engine_key != key or need_hw[0] > have[0] or need_hw[1] > have[1]:
            if self._tta_engine is not None:
                self._tta_engine.close()
                self._tta_engine = None
            hw = (max(need_hw[0], have[0]), max(need_hw[1], have[1]))
            try:
                e = m.make_engine(classes=key[3], max_hw=hw)
            except orehip.OreError as err:
                raise ValueError(f"TTA: no engine for inputs up to {hw[0]}x{hw[1]}{what}: {err}") from err
            if not getattr(e, "has_roi", False):
                e.close()
                raise ValueError("TTA needs the second stage inside the engine (a support set with rcnn_8 features)")
            e._tta_bufs = None
            self._tta_engine, self._tta_engine_key, self._tta_engine_hw = e, key, hw
        return self._tta_engine

    def _pool(self, variants, rows):
        import orehip
        key = (variants, rows, str(self.model.device))
        p = self._pools.get(key)
        if p is None:
            p = self._pools[key] = orehip.TTAPool(variants, rows, self.model.device)
        return p

    # ---- requests -----------------------------------------------------------------------------------------------
    def _source(self, inp):
        """(kind, host-or-device image, its (h, w), out_hw, swap_rb): kind "raw" = [h, w, 3], "image" = [3, h, w]."""
        if "image" in inp and "image_raw" in inp:
            raise ValueError('a request carries either "image" or "image_raw", not both')
        if "image" in inp:
            img = inp["image"]
            if not torch.is_tensor(img):
                img = torch.from_numpy(np.ascontiguousarray(img))
            if img.dim() != 3 or img.shape[0] != 3 or img.dtype != torch.uint8:
                raise ValueError(f'TTA resamples 8-bit images: "image" must be [3, h, w] uint8, got {tuple(img.shape)} {img.dtype}')
            h, w = int(img.shape[1]), int(img.shape[2])
            return "image", img, (h, w), (int(inp.get("height", h)), int(inp.get("width", w))), False
        if "image_raw" in inp:
            raw = inp["image_raw"]
        elif "file_name" in inp:                              # _maybe_read_image: read in the model's input format
            from fewx.data.dataset_mapper import _pil_read_image
            raw = _pil_read_image(inp["file_name"], self.model.input_format)
        else:
            raise ValueError('a TTA request needs "image", "image_raw" or "file_name"')
        if isinstance(raw, np.ndarray):
            raw = torch.from_numpy(np.ascontiguousarray(raw))
        if raw.dim() != 3 or raw.shape[2] != 3 or raw.dtype != torch.uint8:
            raise ValueError(f"image_raw must be [h, w, 3] uint8, got {tuple(raw.shape)} {raw.dtype}")
        h, w = int(raw.shape[0]), int(raw.shape[1])
        return "raw", raw, (h, w), (int(inp.get("height", h)), int(inp.get("width", w))), bool(inp.get("swap_rb", False))

    def forward(self, batched_inputs):
        return [self._inference_one_image(x) for x in batched_inputs]

    @torch.no_grad()
    def _inference_one_image(self, inp):
        assert not self.model.training, "GeneralizedRCNNWithTTA is an evaluation wrapper: model.eval() first"
        self.model.init_model()
        return self._finish(self._enqueue(inp) if self.device_path else self._enqueue_host(inp))

    def _finish(self, p):
        """The one host wait of an image: the merged count; then the record is cut into the result."""
        import orehip
        from detectron2.structures import Boxes, Instances
        k = int(p.count.item())
        boxes, scores, classes = orehip.record_views(p.rec, p.rows, k)
        res = Instances(p.out_hw)
        res.pred_boxes = Boxes(boxes)
        res.scores = scores
        res.pred_classes = classes
        return {"instances": res}

    def _merge(self, pool, out_hw):
        import orehip
        p = _Pending()
        p.rec, p.count = orehip.tta_merge(pool, out_hw[0], out_hw[1], SCORE_THRESH, self.nms_thresh, self.topk)
        p.rows, p.out_hw, p.pool = self.topk + (self.topk & 1), tuple(out_hw), pool
        return p

    # ---- device path --------------------------------------------------------------------------------------------
    def _enqueue(self, inp):
        """Everything of one image up to the merged record, queued on the current stream; single-class: no host synchronisation."""
        import orehip
        m = self.model
        kind, src, src_hw, out_hw, swap = self._source(inp)
        variants = self.tta_mapper.variants(*src_hw)
        check_variant_limits(src_hw, variants)
        big = max(variants, key=lambda v: v["h"] * v["w"])
        e = self._engine((max(v["h"] for v in variants), max(v["w"] for v in variants)),
                         " (largest variant %dx%d, min_size %d)" % (big["h"], big["w"], big["min_size"]))
        if kind == "raw":
            hwc = m._upload_raw(src)
        else:                                                 # the mapper's planar image -> the resize kernel's interleaved layout
            hwc = orehip.to_device(src, m.device).permute(1, 2, 0).contiguous()
        with torch.cuda.device(m.device):
            # all variants first, so that no resize sits between two passes
            images, plain = [], {}
            for v in variants:
                key = (v["h"], v["w"])
                if key not in plain:
                    plain[key] = orehip.resize_bilinear_u8(hwc, v["h"], v["w"], swap_rb=swap)
                images.append(orehip.tta_hflip_u8(plain[key]) if v["flip"] else plain[key])
            nway = bool(getattr(e, "class_ids", None))
            rows = int(orehip.lib().ore_det_record_rows())
            pool = self._pool(len(variants), rows)
            if not nway and e._tta_bufs is None:
                e._tta_bufs = (e.buffer("det_boxes"), e.buffer("det_scores"), e.buffer("det_count"))
            for i, (v, img) in enumerate(zip(variants, images)):
                par = _collect_params(variant_transforms(out_hw, src_hw, v))
                if nway:                                      # the merged N-way rows arrive with a finished pass: one poll per variant
                    b, s, c = e.detect_classes(img, v["h"], v["w"])
                    orehip.tta_collect(pool, i, b, s, c, int(len(s)), rows, **par)
                else:
                    e.eval_forward(img, use_graph=True)
                    b, s, n = e._tta_bufs
                    orehip.tta_collect(pool, i, b, s, None, n, int(b.shape[0]), **par)
            return self._merge(pool, out_hw)

    # ---- host path (custom mapper) ------------------------------------------------------------------------------
    def _enqueue_host(self, inp):
        """mapper -> model.inference per variant -> inverse_boxes on the host -> the merge kernel."""
        import orehip
        m = self.model
        kind, src, src_hw, out_hw, swap = self._source(inp)
        src = src.cpu()
        if kind == "raw":
            src = src.permute(2, 0, 1)
            if swap:
                src = src.flip(0)
        dicts = self.tta_mapper({**{k: v for k, v in inp.items() if k not in ("image_raw", "swap_rb", "image")},
                                 "image": src.contiguous(), "height": out_hw[0], "width": out_hw[1]})
        all_b, all_s, all_c = [], [], []
        for d in dicts:
            r = m.inference([{"image": d["image"]}], do_postprocess=False)[0]
            all_b.append(inverse_boxes(r.pred_boxes.tensor.cpu().numpy(), d["transforms"]))
            all_s.append(r.scores.cpu().numpy())
            all_c.append(r.pred_classes.cpu().numpy())
        n = sum(len(s) for s in all_s)
        pool = self._pool(max(len(dicts), 1), int(orehip.lib().ore_det_record_rows()))
        if n > pool.cap:
            raise ValueError(f"TTA: {n} candidate rows exceed the merge pool of {pool.cap}")
        if n:
            pool.boxes[:n].copy_(torch.from_numpy(np.concatenate(all_b)))
            pool.scores[:n].copy_(torch.from_numpy(np.concatenate(all_s)))
            pool.classes[:n].copy_(torch.from_numpy(np.concatenate(all_c)))
        pool.n.fill_(n)
        with torch.cuda.device(m.device):
            return self._merge(pool, out_hw)
