"""d2z:engine/defaults.py under its own module path (`from detectron2.engine.defaults import DefaultPredictor`, as the reference's
demo/predictor.py imports it).  The trainer side of that file lives in detectron2.engine and is re-exported here;

    DefaultPredictor         d2z:engine/defaults.py:235-297     cfg -> model in eval mode with its weights; BGR image in, Instances out

is defined here.  Its resize is not the reference's CPU ResizeShortestEdge + Pillow: the raw image goes to the device and is resized
there to the same bytes (orehip.resize_bilinear_u8), as an "image_raw" request of the model."""
import torch

from detectron2.engine import (DefaultTrainer, SimpleTrainer, create_ddp_model, default_argument_parser, default_setup,  # noqa: F401
                               launch)

__all__ = ["DefaultPredictor", "DefaultTrainer", "SimpleTrainer", "create_ddp_model", "default_argument_parser", "default_setup", "launch"]


class DefaultPredictor:
    """A simple end-to-end predictor for one image on one device (d2z:engine/defaults.py:235-297):

        pred = DefaultPredictor(cfg)
        outputs = pred(bgr_image)          # {"instances": Instances} at the image's own size

    loads `cfg.MODEL.WEIGHTS` (an empty string loads nothing), takes `cfg.DATASETS.TEST[0]`'s metadata, always receives a BGR image
    ([h, w, 3] uint8) and converts it to `cfg.INPUT.FORMAT`, resizes to `cfg.INPUT.MIN_SIZE_TEST` / `MAX_SIZE_TEST`.  The few-shot
    support set comes from the model's `init_model()` on the first call, as for every eval call; `predictor.model.set_support_dict(...)`
    before that call installs one directly.  rectify=orehip.Rectifier(...): the camera looks at the scene obliquely; every image is
    uploaded and warped into the rectifier's plane on the device (contract "rectify v1") before the resize, and the Instances are in
    rectified coordinates, at rectify.out_hw.  None (the default) enqueues exactly what it always has."""

    def __init__(self, cfg, rectify=None):
        from detectron2.checkpoint import DetectionCheckpointer
        from detectron2.data import MetadataCatalog
        from detectron2.modeling import build_model
        self.cfg = cfg.clone()
        self.model = build_model(self.cfg)
        self.model.eval()
        if len(cfg.DATASETS.TEST):
            self.metadata = MetadataCatalog.get(cfg.DATASETS.TEST[0])
        DetectionCheckpointer(self.model).load(cfg.MODEL.WEIGHTS)
        self.input_format = cfg.INPUT.FORMAT
        assert self.input_format in ["RGB", "BGR"], self.input_format
        if rectify is not None and not (callable(rectify) and hasattr(rectify, "out_hw")):
            raise ValueError("DefaultPredictor: rectify is None or an orehip.Rectifier")
        self.rectify = rectify

    def _rectified(self, image):
        """The image on the model's device, warped by self.rectify on the current stream."""
        import numpy as np
        import orehip
        if isinstance(image, np.ndarray):
            image = torch.from_numpy(np.ascontiguousarray(image))
        if not torch.is_tensor(image) or image.dim() != 3 or image.shape[2] != 3 or image.dtype != torch.uint8:
            raise ValueError("DefaultPredictor: a rectified image is [h, w, 3] uint8")
        dev = torch.device(self.model.device)
        with torch.cuda.device(dev):
            return self.rectify(orehip.to_device(image, dev).contiguous())

    def __call__(self, original_image):
        """original_image: [h, w, 3] uint8 in BGR order (numpy array, CPU or device tensor).  Returns the model's output for it:
        {"instances": Instances} with pred_boxes / scores / pred_classes at (h, w); with rectify=, at rectify.out_hw."""
        with torch.no_grad():
            if self.rectify is not None:
                original_image = self._rectified(original_image)
            height, width = original_image.shape[:2]
            inputs = {"image_raw": original_image, "swap_rb": self.input_format == "RGB", "height": int(height), "width": int(width)}
            return self.model([inputs])[0]
