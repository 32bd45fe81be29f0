"""CPU: the host side of the device resize (orehip.resize_plan / resize_shortest_edge_shape), DefaultPredictor's import surface and
the mapper's device_resize switch.  Pillow's own output, computed here, is the definition of the resample."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import PKG

# (h, w) -> (nh, nw): both directions, ratios 0.04 .. 25, an identity, one-axis-only cases, window clamping at a tiny input, ksize 51,
# and (last, behind the pairs other tests take by position) two outputs smaller than one 16 x 64 tile of the device kernel: narrower
# than 16 columns, and a row shorter than one 4-byte store under 65-tap windows
PAIRS = [((480, 640), (600, 800)), ((1200, 1600), (600, 800)), ((1080, 1920), (563, 1000)), ((333, 500), (600, 901)),
         ((37, 53), (600, 859)), ((768, 1024), (600, 800)), ((600, 800), (600, 800)), ((2000, 3000), (600, 900)),
         ((500, 333), (901, 600)), ((3, 5), (320, 533)), ((8000, 6000), (320, 240)), ((37, 53), (7, 13)), ((64, 96), (16, 3))]


def pil_resize(img, nh, nw):
    return np.asarray(Image.fromarray(img).resize((nw, nh), Image.BILINEAR))


def resample_rows(img, bounds, coeffs):
    """One pass along axis 0 of [n, m, c] uint8 with the planner's tables: clip8((2^21 + sum(src * k)) >> 22)."""
    n_out, ks = coeffs.shape
    src = img.astype(np.int64)
    acc = np.full((n_out,) + img.shape[1:], 1 << 21, dtype=np.int64)
    for t in range(ks):
        live = bounds[:, 1] > t
        idx = np.minimum(bounds[:, 0] + t, img.shape[0] - 1)
        acc += np.where(live, coeffs[:, t], 0).astype(np.int64)[:, None, None] * src[idx]
    return np.clip(acc >> 22, 0, 255).astype(np.uint8)


@pytest.fixture(scope="module")
def ore():
    import orehip
    if not os.path.exists(orehip.LIB_PATH):
        orehip.build()
    orehip.lib()
    return orehip


@pytest.mark.parametrize("hw,nhw", PAIRS, ids=["%dx%d-%dx%d" % (a + b) for a, b in PAIRS])
def test_planner_equals_pillow(ore, hw, nhw):
    """The planner's windows and 22-bit weights, applied in numpy as two passes with a uint8 intermediate (horizontal first), give
    Pillow's bytes: 0 differing."""
    (h, w), (nh, nw) = hw, nhw
    img = np.random.default_rng(h * 10007 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    xb, kx = ore.resize_plan(w, nw)
    yb, ky = ore.resize_plan(h, nh)
    for b, k, n_in in ((xb, kx, w), (yb, ky, h)):
        scale = max(n_in / len(b), 1.0)
        assert k.shape[1] == 2 * int(np.ceil(scale)) + 1
        assert (b[:, 0] >= 0).all() and (b[:, 1] >= 1).all() and (b[:, 0] + b[:, 1] <= n_in).all() and (b[:, 1] <= k.shape[1]).all()
        assert (np.diff(b[:, 0]) >= 0).all() and (np.diff(b[:, 0] + b[:, 1]) >= 0).all()        # what the kernel's tile staging relies on
    mid = resample_rows(img.transpose(1, 0, 2), xb, kx).transpose(1, 0, 2)
    got = resample_rows(mid, yb, ky)
    want = pil_resize(img, nh, nw)
    assert got.shape == want.shape
    assert int((got != want).sum()) == 0


def test_planner_rejects_bad_sizes(ore):
    for n_in, n_out in ((0, 10), (10, 0), (8193, 10), (10, 8193)):
        with pytest.raises(ore.OreError):
            ore.resize_plan(n_in, n_out)
    assert ore.resize_plan(8192, 1)[1].shape == (1, 2 * 8192 + 1)


def _cfg(extra=()):
    from fewx.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(PKG, "configs", "fsod", "finetune_vovnet.yaml"))
    cfg.merge_from_list(list(extra))
    return cfg


@pytest.mark.parametrize("size,max_size", [(320, 1000), (600, 1000)])
def test_shortest_edge_shape_equals_mapper(ore, size, max_size):
    """resize_shortest_edge_shape == the size DatasetMapperWithSupport._resize_flip resizes to, on 200 seeded sizes in [32, 4000]^2
    under both shipped test sizes (finetune_vovnet.yaml 320 / 1000, Base-FSOD-C4.yaml 600 / 1000)."""
    from fewx.data.dataset_mapper import DatasetMapperWithSupport
    cfg = _cfg(["INPUT.MIN_SIZE_TEST", size, "INPUT.MAX_SIZE_TEST", max_size])
    m = DatasetMapperWithSupport(cfg, is_train=False)
    rng = np.random.default_rng(5)
    for h, w in rng.integers(32, 4001, (200, 2)):
        out, _ = m._resize_flip(np.zeros((h, w, 3), dtype=np.uint8), np.random.default_rng(0))
        assert ore.resize_shortest_edge_shape(int(h), int(w), size, max_size) == out.shape[:2], (h, w)


def test_default_predictor_surface():
    """detectron2.engine.defaults imports, DefaultPredictor is re-exported, and on a machine without the GPU the constructor either
    works or fails with the package's own device error -- never an ImportError."""
    import detectron2.engine
    from detectron2.engine.defaults import DefaultPredictor
    assert detectron2.engine.DefaultPredictor is DefaultPredictor and "DefaultPredictor" in detectron2.engine.__all__
    cfg = _cfg(["MODEL.WEIGHTS", "", "MODEL.DEVICE", "cuda" if torch.cuda.is_available() else "cpu"])
    p = DefaultPredictor(cfg)
    assert p.input_format == "BGR" and not p.model.training
    assert p.cfg is not cfg and p.cfg.INPUT.MIN_SIZE_TEST == 320
    if not torch.cuda.is_available():
        p.model.set_support_dict({k: {0: torch.zeros(1, 128, s, s)} for k, s in (("p3", 32), ("p4", 16), ("p5", 8))})
        with pytest.raises((RuntimeError, AssertionError), match="MI355X"):
            p(np.zeros((48, 64, 3), dtype=np.uint8))
    with pytest.raises(AssertionError):
        DefaultPredictor(_cfg(["MODEL.WEIGHTS", "", "MODEL.DEVICE", "cpu", "INPUT.FORMAT", "L"]))


def test_mapper_device_resize():
    """device_resize=True: a test-time record carries image_raw (HWC uint8, the original size) with height / width and no image; the
    default returns what it returned before; with is_train=True it raises."""
    from fewx.data.dataset_mapper import DatasetMapperWithSupport
    cfg = _cfg()
    img = np.random.default_rng(3).integers(0, 256, (120, 200, 3), dtype=np.uint8)
    read = lambda path, format="BGR": img
    rec = {"file_name": "x.png", "image_id": 7, "height": 120, "width": 200, "annotations": [{"bbox": [1, 2, 3, 4], "id": 1}]}
    a = DatasetMapperWithSupport(cfg, is_train=False, read_image=read)(rec)
    b = DatasetMapperWithSupport(cfg, is_train=False, read_image=read, device_resize=False)(rec)
    assert sorted(a) == sorted(b) and torch.equal(a["image"], b["image"]) and "image_raw" not in a and "annotations" not in a
    assert {k: v for k, v in a.items() if k != "image"} == {k: v for k, v in b.items() if k != "image"}
    assert tuple(a["image"].shape) == (3, 320, 533)
    assert np.array_equal(a["image"].numpy(), pil_resize(img, 320, 533).transpose(2, 0, 1))
    d = DatasetMapperWithSupport(cfg, is_train=False, read_image=read, device_resize=True)(rec)
    assert "image" not in d and "annotations" not in d
    assert d["image_raw"].dtype == torch.uint8 and np.array_equal(d["image_raw"].numpy(), img)
    assert (d["height"], d["width"], d["image_id"]) == (120, 200, 7)
    rec2 = {"file_name": "x.png", "image_id": 8}
    d2 = DatasetMapperWithSupport(cfg, is_train=False, read_image=read, device_resize=True)(rec2)
    assert (d2["height"], d2["width"]) == (120, 200)
    with pytest.raises(ValueError):
        DatasetMapperWithSupport(cfg, is_train=True, support_df=object(), read_image=read, device_resize=True)
