"""d2z:utils/visualizer.py for box detections: ColorMode, VisImage and a Visualizer whose draw_instance_predictions renders boxes,
class names and scores by the package's own render contract ("overlay v1", include/ore_hip.h) instead of matplotlib: on the device
for device Instances (orehip.overlay_draw), on the host for host Instances (orehip.overlay_host) -- the same bytes either way.
draw_heatmap lays a heat map of a detection pass over the frame ("heatmap v1": orehip.heatmap_draw / heatmap_host).
Masks, keypoints, panoptic and semantic drawing are not built: those methods raise."""
from enum import Enum, unique
from math import isqrt

import numpy as np
import torch

__all__ = ["ColorMode", "VisImage", "Visualizer", "default_overlay_params", "draw_heat"]

_BOXES_ONLY = "this package draws boxes only (draw_instance_predictions); masks, keypoints, panoptic and semantic drawing are not built"


@unique
class ColorMode(Enum):
    """IMAGE: one colour per instance.  SEGMENTATION: one colour per class.  IMAGE_BW needs masks and is not built."""
    IMAGE = 0
    SEGMENTATION = 1
    IMAGE_BW = 2


def default_overlay_params(h, w):
    """Line width and text scale in detectron2's proportions (its default font size is max(sqrt(h * w) // 90, 10)), within the
    overlay's limits: F = max(isqrt(h * w) // 90, 10), line_width = max(1, F // 4), text_scale = max(1, (F + 5) // 11)."""
    F = max(isqrt(int(h) * int(w)) // 90, 10)
    return {"line_width": min(max(1, F // 4), 16), "text_scale": min(max(1, (F + 5) // 11), 8)}


def thing_classes(metadata):
    """metadata.thing_classes, or None where the metadata has none."""
    return getattr(metadata, "thing_classes", None)


class VisImage:
    """A drawn frame: [h, w, 3] uint8, a numpy array or a device tensor, in RGB or BGR order.  get_image() is always RGB numpy."""

    def __init__(self, img, channel_order="RGB"):
        assert channel_order in ("RGB", "BGR"), channel_order
        self.img, self.channel_order = img, channel_order
        self.height, self.width = int(img.shape[0]), int(img.shape[1])

    def get_image(self):
        img = self.img.cpu().numpy() if torch.is_tensor(self.img) else np.asarray(self.img)
        return img if self.channel_order == "RGB" else np.ascontiguousarray(img[:, :, ::-1])

    def save(self, filepath):
        from PIL import Image
        Image.fromarray(self.get_image()).save(filepath)


def draw_boxes(frame, predictions, *, channel_order, names, color_by, score_thresh=0.0, ids=None):
    """One frame + Instances -> VisImage.  Device Instances: the frame goes to their device and the kernel draws; host Instances:
    overlay_host.  The frame itself is left as it was.  ids: the rows' track ids (an orehip.BoxTracker update's) for color_by="track"."""
    import orehip
    if not predictions.has("pred_boxes") or not predictions.has("scores"):
        raise ValueError("the overlay draws pred_boxes with their scores (pred_classes optional)")
    boxes = predictions.pred_boxes
    boxes = boxes.tensor if hasattr(boxes, "tensor") else torch.as_tensor(boxes)
    scores = predictions.scores
    classes = predictions.pred_classes if predictions.has("pred_classes") else None
    h, w = int(frame.shape[0]), int(frame.shape[1])
    palette = orehip.OVERLAY_PALETTE if channel_order == "RGB" else np.ascontiguousarray(orehip.OVERLAY_PALETTE[:, ::-1])
    kw = dict(default_overlay_params(h, w), score_thresh=score_thresh, palette=palette, color_by=color_by, names=names)
    if ids is not None:
        kw["ids"] = ids.long().contiguous() if torch.is_tensor(ids) else np.asarray(ids, dtype=np.int64)
    if boxes.is_cuda:
        if not torch.is_tensor(frame):
            frame = torch.from_numpy(np.ascontiguousarray(frame))
        dev_frame = orehip.to_device(frame, boxes.device).contiguous()
        boxes = boxes.float().contiguous().reshape(-1, 4)
        out = orehip.overlay_draw(dev_frame, boxes, scores.float().contiguous(), None if classes is None else classes.long().contiguous(), **kw)
    else:
        host = frame.cpu().numpy() if torch.is_tensor(frame) else np.ascontiguousarray(frame)
        out = orehip.overlay_host(host, boxes.float().reshape(-1, 4), scores.float(), None if classes is None else classes.long(), **kw)
    return VisImage(out, channel_order)


def draw_heat(frame, source, *, channel_order, in_hw=None, **style):
    """One frame + a heat source -> VisImage.  source: an orehip.HeatSource or HeatLevels (device: the frame goes to its device and
    the kernel draws), or a sequence of (uint8 map, stride) with in_hw -- device maps draw on the device, host maps through
    heatmap_host: the same bytes either way.  style: lut, alpha, alpha_mode of orehip.heatmap_draw.  The frame itself is left as it was."""
    import orehip
    unknown = sorted(set(style) - {"lut", "alpha", "alpha_mode"})
    if unknown:
        raise ValueError(f"draw_heatmap takes lut, alpha, alpha_mode (and in_hw with bare maps); not {', '.join(unknown)}")
    if isinstance(source, orehip.HeatSource):
        dev = source.device
    elif isinstance(source, orehip.HeatLevels):
        dev = source.maps[0].device
    else:
        source = list(source)
        first = source[0][0] if source and isinstance(source[0], (tuple, list)) and len(source[0]) == 2 else None
        dev = first.device if torch.is_tensor(first) and first.is_cuda else None
    if dev is not None:
        if not torch.is_tensor(frame):
            frame = torch.from_numpy(np.ascontiguousarray(frame))
        out = orehip.heatmap_draw(orehip.to_device(frame, dev).contiguous(), source, in_hw, channel_order=channel_order, **style)
    else:
        host = frame.cpu().numpy() if torch.is_tensor(frame) else np.ascontiguousarray(frame)
        out = orehip.heatmap_host(host, source, in_hw, channel_order=channel_order, **style)
    return VisImage(out, channel_order)


class Visualizer:
    """Visualizer(img_rgb, metadata=None, scale=1.0, instance_mode=ColorMode.IMAGE): img_rgb is [h, w, 3] in 0 .. 255, a numpy array
    or a uint8 tensor (host or device).  The overlay draws at the frame's size, so scale must be 1.0.  channel_order="BGR" (an
    extension) tells that the frame is BGR: the palette follows and VisImage.get_image() still returns RGB."""

    def __init__(self, img_rgb, metadata=None, scale=1.0, instance_mode=ColorMode.IMAGE, *, channel_order="RGB"):
        if scale != 1.0:
            raise ValueError(f"Visualizer: scale {scale}: the overlay draws at the frame's own size (scale 1.0)")
        if instance_mode not in (ColorMode.IMAGE, ColorMode.SEGMENTATION):
            raise NotImplementedError(f"Visualizer: {instance_mode} needs instance masks; " + _BOXES_ONLY)
        if not torch.is_tensor(img_rgb):
            img_rgb = np.asarray(img_rgb).clip(0, 255).astype(np.uint8)
        if img_rgb.ndim != 3 or img_rgb.shape[2] != 3 or (torch.is_tensor(img_rgb) and img_rgb.dtype != torch.uint8):
            raise ValueError(f"Visualizer takes an [h, w, 3] image (tensors: uint8), got {tuple(img_rgb.shape)}")
        self.img = img_rgb
        self.metadata = metadata
        self.channel_order = channel_order
        self._instance_mode = instance_mode
        self.output = VisImage(img_rgb, channel_order)

    def draw_instance_predictions(self, predictions):
        """Boxes, class names (metadata.thing_classes) and scores of an Instances; ColorMode.IMAGE colours by instance,
        SEGMENTATION by class.  Returns the drawn VisImage."""
        self.output = draw_boxes(self.img, predictions, channel_order=self.channel_order, names=thing_classes(self.metadata),
                                 color_by="class" if self._instance_mode == ColorMode.SEGMENTATION else "instance")
        return self.output

    def draw_heatmap(self, source, **style):
        """A heat map of a detection pass over the image (draw_heat: an orehip.HeatSource / HeatLevels, or (map, stride) pairs with
        in_hw=; lut, alpha, alpha_mode).  The result becomes the image later draws start from, so boxes drawn afterwards lie on top
        of the heat map.  Returns the drawn VisImage."""
        self.output = draw_heat(self.img, source, channel_order=self.channel_order, **style)
        self.img = self.output.img
        return self.output

    def get_output(self):
        return self.output

    def draw_panoptic_seg_predictions(self, *args, **kwargs):
        raise NotImplementedError("draw_panoptic_seg_predictions: " + _BOXES_ONLY)

    def draw_sem_seg(self, *args, **kwargs):
        raise NotImplementedError("draw_sem_seg: " + _BOXES_ONLY)

    def draw_dataset_dict(self, *args, **kwargs):
        raise NotImplementedError("draw_dataset_dict: " + _BOXES_ONLY)
