"""CPU: the host side of test-time augmentation (detectron2/modeling/test_time_augmentation.py) -- the variant list and the mapper's
images against Pillow, the inverse box transforms against a numpy restatement of fvcore's HFlipTransform / detectron2's
ResizeTransform written here, the host merge against hand-made cases, and the limit / type errors, which need no GPU."""
import os
import pickle

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import PKG

MIN_SIZES, MAX_SIZE = [256, 320, 416], 640
# ResizeShortestEdge(min_size, 640) of the two inputs; 300x500 at 416 would be 416x693: capped to 384x640
SHAPES = {(300, 500): [(256, 427), (320, 533), (384, 640)], (480, 640): [(256, 341), (320, 427), (416, 555)]}


def _cfg(extra=()):
    from fewx.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(PKG, "configs", "fsod", "finetune_vovnet.yaml"))
    cfg.merge_from_list(["MODEL.WEIGHTS", "", "MODEL.DEVICE", "cpu"] + list(extra))
    return cfg


def _tta_cfg(flip=True):
    return _cfg(["TEST.AUG.MIN_SIZES", MIN_SIZES, "TEST.AUG.MAX_SIZE", MAX_SIZE, "TEST.AUG.FLIP", flip])


@pytest.mark.parametrize("flip", [True, False])
@pytest.mark.parametrize("hw", sorted(SHAPES), ids=lambda v: "%dx%d" % v)
def test_variant_list_and_mapper_images(hw, flip):
    """len(min_sizes) * (2 if flip else 1) variants, per min_size [resize] then [resize, flip]; the images are Pillow's BILINEAR resize
    and its column-reversed copy; the chain is resize (+ flip), with the pre-resize in front when the output size differs."""
    from detectron2.modeling import DatasetMapperTTA
    from detectron2.modeling import test_time_augmentation as T
    h, w = hw
    img = np.random.default_rng(h + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    for mapper in (DatasetMapperTTA(_tta_cfg(flip)), DatasetMapperTTA(MIN_SIZES, MAX_SIZE, flip)):
        got = mapper.variants(h, w)
        want = [(ms, s, f) for ms, s in zip(MIN_SIZES, SHAPES[hw]) for f in ((False, True) if flip else (False,))]
        assert [(v["min_size"], (v["h"], v["w"]), v["flip"]) for v in got] == want
    chw = torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1)))
    for extra, pre in (({}, ()), ({"height": 2 * h, "width": 2 * w + 1}, (("resize", 2 * h, 2 * w + 1, h, w),))):
        dicts = mapper({"image": chw, "image_id": 5, **extra})
        assert len(dicts) == len(want)
        for d, (ms, (nh, nw), f) in zip(dicts, want):
            ref = np.asarray(Image.fromarray(img).resize((nw, nh), Image.BILINEAR))
            ref = ref[:, ::-1] if f else ref
            assert d["image"].dtype == torch.uint8 and np.array_equal(d["image"].numpy(), ref.transpose(2, 0, 1))
            assert d["transforms"] == pre + (("resize", h, w, nh, nw),) + ((("hflip", nw),) if f else ())
            assert d["image_id"] == 5 and pickle.loads(pickle.dumps(d["transforms"])) == d["transforms"]
    assert torch.equal(chw, torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1))))      # the input is left alone
    with pytest.raises(TypeError):
        DatasetMapperTTA(MIN_SIZES)


# ---- fvcore HFlipTransform / detectron2 ResizeTransform on float32 arrays, from their formulas:
#   HFlipTransform.apply_coords:  coords[:, 0] = self.width - coords[:, 0]
#   ResizeTransform.apply_coords: coords[:, 0] = coords[:, 0] * (self.new_w * 1.0 / self.w); coords[:, 1] likewise with new_h / h
#   Transform.apply_box: the corners (x0,y0) (x1,y0) (x0,y1) (x1,y1) through apply_coords, then min and max over the four
#   inverse(): HFlip -> itself; Resize(h, w, new_h, new_w) -> Resize(new_h, new_w, h, w); TransformList.inverse: reversed order
def _ref_apply_box(box, coords_fn):
    x0, y0, x1, y1 = (box[:, i] for i in range(4))
    corners = np.stack([np.stack([x0, y0], 1), np.stack([x1, y0], 1), np.stack([x0, y1], 1), np.stack([x1, y1], 1)], 1)   # [n, 4, 2]
    out = coords_fn(corners.reshape(-1, 2).astype(np.float32)).reshape(-1, 4, 2)
    return np.concatenate([out.min(1), out.max(1)], 1)


def _ref_inverse(box, chain):
    box = box.astype(np.float32)
    for t in chain[::-1]:
        if t[0] == "hflip":
            def fn(c, W=t[1]):
                c[:, 0] = W - c[:, 0]
                return c
        else:
            def fn(c, t=t):
                _, h, w, nh, nw = t                         # the inverse maps (nh, nw) back to (h, w)
                c[:, 0] = c[:, 0] * np.float32(w * 1.0 / nw)
                c[:, 1] = c[:, 1] * np.float32(h * 1.0 / nh)
                return c
        box = _ref_apply_box(box, fn)
        assert box.dtype == np.float32
    return box


def test_inverse_transform_arithmetic():
    """inverse_boxes (what ore_tta_collect_fwd is held to) == the restatement above, bit for bit, on random boxes that reach outside
    the image, for every variant of both inputs with and without the pre-resize."""
    from detectron2.modeling import test_time_augmentation as T
    rng = np.random.default_rng(11)
    for (h, w) in SHAPES:
        for out_hw in ((h, w), (2 * h + 1, 3 * w - 7)):
            for v in T.tta_variants(h, w, MIN_SIZES, MAX_SIZE, True):
                chain = T.variant_transforms(out_hw, (h, w), v)
                assert len(chain) == 1 + (out_hw != (h, w)) + v["flip"]
                p = rng.uniform(-0.2, 1.2, (500, 2, 2)).astype(np.float32) * np.float32([v["w"], v["h"]])
                box = np.concatenate([p.min(1), p.max(1)], 1).astype(np.float32)
                box[:7] = box[:7, [2, 1, 0, 3]]                                   # a few with x0 > x1: min / max must reorder them
                got, want = T.inverse_boxes(box, chain), _ref_inverse(box, chain)
                assert got.dtype == np.float32 and np.array_equal(got, want)
                par = T._collect_params(chain)                                    # the kernel's arguments say the same chain
                assert par["flip"] == v["flip"] and par["variant_w"] == v["w"] and (par["pre"] is None) == (out_hw == (h, w))
                assert (par["sx"], par["sy"]) == (w * 1.0 / v["w"], h * 1.0 / v["h"])
                if par["pre"]:
                    assert par["pre"] == (out_hw[1] * 1.0 / w, out_hw[0] * 1.0 / h)


def _merge(boxes, scores, classes, out_hw=(100, 100), thr=0.5, topk=100):
    from detectron2.modeling.test_time_augmentation import merge_detections_host
    return merge_detections_host(np.asarray(boxes, np.float32), np.asarray(scores, np.float32), np.asarray(classes, np.int64), out_hw, 1e-8,
                                 thr, topk)


def test_host_merge_cases():
    from oracle import decode as odec
    from detectron2.modeling.test_time_augmentation import merge_detections_host
    # cross-variant suppression: candidate 2 (a later variant's row of the same object) outscores and suppresses candidate 0
    b, s, c, idx = _merge([[10, 10, 50, 50], [60, 60, 90, 90], [11, 10, 50, 50]], [0.8, 0.7, 0.9], [0, 0, 0])
    assert idx.tolist() == [2, 1] and s.tolist() == [np.float32(0.9), np.float32(0.7)]
    # two classes with identical boxes: both stay
    b, s, c, idx = _merge([[10, 10, 50, 50], [10, 10, 50, 50]], [0.8, 0.7], [3, 8])
    assert idx.tolist() == [0, 1] and c.tolist() == [3, 8]
    # equal scores keep candidate order, also across classes, and the earlier one wins an overlap
    b, s, c, idx = _merge([[0, 0, 10, 10], [20, 20, 30, 30], [0, 0, 10, 10.5], [40, 40, 50, 50]], [0.5, 0.5, 0.5, 0.5], [1, 0, 1, 0])
    assert idx.tolist() == [0, 1, 3]
    # top-k cut in score order
    boxes = [[10 * i, 0, 10 * i + 8, 8] for i in range(10)]
    b, s, c, idx = _merge(boxes, np.linspace(0.1, 1.0, 10), [0] * 10, out_hw=(8, 200), topk=4)
    assert idx.tolist() == [9, 8, 7, 6]
    # rows with a NaN / inf are dropped before anything else, a score at the threshold leaves, boxes are clipped and degenerate ones stay
    b, s, c, idx = _merge([[np.nan, 0, 5, 5], [0, 0, 5, 5], [0, 0, np.inf, 5], [-4, -4, 120, 30], [50, 50, 50, 50], [1, 1, 2, 2]],
                          [0.9, 0.8, 0.7, 0.6, 0.5, 1e-8], [0] * 6)
    assert idx.tolist() == [1, 3, 4] and b[1].tolist() == [0, 0, 100, 30] and b[2].tolist() == [50, 50, 50, 50]
    assert len(_merge(np.zeros((0, 4)), [], [])[3]) == 0
    # the built-in NMS and the oracle's C NMS (the GPU tests' choice) agree on a crowded random set
    rng = np.random.default_rng(2)
    xy = rng.uniform(0, 80, (400, 2)).astype(np.float32)
    boxes = np.concatenate([xy, xy + rng.uniform(5, 40, (400, 2)).astype(np.float32)], 1)
    scores, classes = rng.uniform(0, 1, 400).astype(np.float32), rng.integers(0, 3, 400)
    scores[::7] = scores[3]
    a = merge_detections_host(boxes, scores, classes, (100, 100), 1e-8, 0.5, 50)
    o = merge_detections_host(boxes, scores, classes, (100, 100), 1e-8, 0.5, 50, nms=odec.nms)
    assert all(np.array_equal(x, y) for x, y in zip(a, o)) and len(a[3]) == 50


def _cpu_model(cfg):
    from detectron2.modeling import build_model
    m = build_model(cfg).eval()
    m.set_support_dict({k: {0: torch.zeros(1, 128, s, s)} for k, s in (("p3", 32), ("p4", 16), ("p5", 8))})
    return m


def test_limits_and_types_without_gpu():
    """A variant the detection tail cannot hold is a ValueError that names it and the limit, raised before any GPU work (the model is
    on the CPU here); so is a resize side beyond 8192; a model that is not the detector is a TypeError."""
    from detectron2.modeling import GeneralizedRCNNWithTTA
    from detectron2.modeling import test_time_augmentation as T
    cfg = _cfg()
    assert list(cfg.TEST.AUG.MIN_SIZES) == [400, 500, 600, 700, 800, 900, 1000, 1100, 1200] and cfg.TEST.AUG.MAX_SIZE == 4000
    with pytest.raises(TypeError, match="CenterNet2Detector"):
        GeneralizedRCNNWithTTA(cfg, torch.nn.Linear(2, 2))
    model = _cpu_model(cfg)
    tta = GeneralizedRCNNWithTTA(cfg, _Wrapped(model))
    assert tta.model is model and tta.device_path and (tta.topk, tta.nms_thresh) == (100, 0.9)
    frame = np.zeros((1080, 1920, 3), dtype=np.uint8)
    with pytest.raises(ValueError, match=r"1200x2133 \(min_size 1200.*30720") as ei:
        tta([{"image_raw": frame}])
    assert "1100x1956" in str(ei.value) and "1000x1778" not in str(ei.value)
    with pytest.raises(ValueError, match="8192"):
        GeneralizedRCNNWithTTA(_cfg(["TEST.AUG.MIN_SIZES", [9000], "TEST.AUG.MAX_SIZE", 20000]), model)([{"image_raw": np.zeros((64, 64, 3), np.uint8)}])
    with pytest.raises(ValueError, match="uint8"):
        tta([{"image": torch.zeros(3, 64, 64)}])
    with pytest.raises(ValueError, match="not both"):
        tta([{"image": torch.zeros(3, 64, 64, dtype=torch.uint8), "image_raw": frame}])
    # the largest variants the tail holds pass the check
    T.check_variant_limits((1080, 1920), T.tta_variants(1080, 1920, [400, 1000], 4000, True))


class _Wrapped(torch.nn.Module):
    """A DistributedDataParallel-like wrapper: the model under `.module`."""

    def __init__(self, module):
        super().__init__()
        self.module = module
