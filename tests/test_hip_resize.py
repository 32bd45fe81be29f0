"""GPU: the device resize (csrc/ore_resize.hip) against Pillow, byte for byte, and the raw-image request form built on it:
CenterNet2Detector with "image_raw", DefaultPredictor, inference_many, N-way.  Pillow's output, computed here, is the reference."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import PKG
from oracle import ref_model as R
from test_resize_host import PAIRS, pil_resize

pytestmark = pytest.mark.gpu

# The one-launch form stages a 16 x 64 output tile's source rows and its intermediate in at most 64 KiB of LDS (ore_hip.h); a tile
# of 8000x6000 -> 320x240 (ratio 25, 51-tap windows) would need several times that, so that pair runs as two launches through a
# workspace.  Every other pair fits.
WORKSPACE_PAIRS = {((8000, 6000), (320, 240))}


@pytest.fixture(scope="module")
def ore():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import orehip
    orehip.lib()
    return orehip


def random_image(h, w):
    return np.random.default_rng(h * 10007 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)


def ramp_image(h, w):
    """Smooth and different in every channel: a one-off row / column shift changes most bytes."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([255.0 * x / max(w - 1, 1), 255.0 * y / max(h - 1, 1), 127.5 + 127.5 * np.sin(x / 7.0 + y / 11.0)], -1)
    return np.ascontiguousarray(np.round(img).astype(np.uint8))


def guarded(ore_, img, nh, nw, **kw):
    """resize_bilinear_u8 into the middle of a buffer of 0xA5 bytes; returns the output and checks both guard bands."""
    n, band = 3 * nh * nw, 4096
    buf = torch.full((n + 2 * band,), 0xA5, dtype=torch.uint8, device="cuda")
    out = buf[band:band + n].view(3, nh, nw)
    got = ore_.resize_bilinear_u8(torch.from_numpy(img).cuda(), nh, nw, out=out, **kw)
    assert got.data_ptr() == out.data_ptr()
    host = buf.cpu().numpy()
    assert (host[:band] == 0xA5).all() and (host[band + n:] == 0xA5).all(), "bytes outside the output were written"
    return host[band:band + n].reshape(3, nh, nw)


@pytest.mark.parametrize("hw,nhw", PAIRS, ids=["%dx%d-%dx%d" % (a + b) for a, b in PAIRS])
def test_resize_equals_pillow(ore, hw, nhw):
    """Bit-exact against Pillow on random bytes and on a ramp, channel swap off and on, in the form the library chooses -- which is
    asserted, so that both forms are known to be covered -- with the output's guard bands untouched."""
    (h, w), (nh, nw) = hw, nhw
    want_form = ore.RESIZE_FORM_WORKSPACE if (hw, nhw) in WORKSPACE_PAIRS else ore.RESIZE_FORM_LDS
    assert ore.resize_form(h, w, nh, nw) == want_form
    for img in (random_image(h, w), ramp_image(h, w)):
        want = pil_resize(img, nh, nw).transpose(2, 0, 1)
        for swap in (False, True):
            got = guarded(ore, img, nh, nw, swap_rb=swap)
            ref = want[::-1] if swap else want
            diff = int((got != ref).sum())
            print(f"{h}x{w}->{nh}x{nw} swap={swap} form={want_form}: {diff} differing bytes")
            assert np.array_equal(got, ref)


@pytest.mark.parametrize("hw,nhw", [p for p in PAIRS if p not in WORKSPACE_PAIRS][:6], ids=lambda v: "%dx%d" % v)
def test_resize_forms_agree(ore, hw, nhw):
    """The two-launch form, forced where the one-launch form is the choice, writes the same bytes (Pillow's); forcing the LDS form
    where it does not fit is an error, not a fallback."""
    (h, w), (nh, nw) = hw, nhw
    img = random_image(h, w)
    want = pil_resize(img, nh, nw).transpose(2, 0, 1)
    assert np.array_equal(guarded(ore, img, nh, nw, form=ore.RESIZE_FORM_WORKSPACE), want)
    assert np.array_equal(guarded(ore, img, nh, nw, form=ore.RESIZE_FORM_LDS), want)


def test_resize_lds_form_refused_where_it_does_not_fit(ore):
    img = torch.zeros(8000, 6000, 3, dtype=torch.uint8, device="cuda")
    with pytest.raises(ore.OreError, match="LDS form"):
        ore.resize_bilinear_u8(img, 320, 240, form=ore.RESIZE_FORM_LDS)


def test_resize_unaligned_views_and_streams(ore):
    """A source that starts at an odd address (the 16-byte staging loads must not read outside it) and an odd-width output whose rows
    start at every alignment; on a side stream."""
    h, w, nh, nw = 211, 317, 157, 203
    img = random_image(h, w)
    buf = torch.full((h * w * 3 + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    want = pil_resize(img, nh, nw).transpose(2, 0, 1)
    for off in (1, 7, 16, 33):
        src = buf[off:off + h * w * 3].view(h, w, 3)
        src.copy_(torch.from_numpy(img))
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        got = ore.resize_bilinear_u8(src, nh, nw, stream=s)
        s.synchronize()
        assert np.array_equal(got.cpu().numpy(), want), off


# ------------------------------------------------------------------------------------------ the raw-image request form
RAW_SIZES = [(480, 640), (300, 500)]                      # -> 320x427 and 320x533 under MIN_SIZE_TEST 320 / MAX_SIZE_TEST 640


def _cfg(extra=()):
    from fewx.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(PKG, "configs", "fsod", "finetune_vovnet.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", "cuda", "INPUT.MAX_SIZE_TEST", 640, "MODEL.WEIGHTS", ""] + list(extra))
    return cfg


def _roi_state():
    sd = R.synth_state_dict(0)
    sd2 = R.synth_roi_state(sd)
    sd2["roi_heads.box_head.0.fc1.weight"] = sd2["roi_heads.box_head.0.fc1.weight"] * 0.01
    return sd, sd2


def _support_dict(ids=(0,)):
    d = {k: {} for k in ("p3", "p4", "p5", "rcnn_8", "rcnn_4")}
    for j, c in enumerate(ids):
        for k, v in R.synth_support(j * 10).items():
            d[k][c] = v
        d["rcnn_8"][c] = torch.randn(24, 128, 8, 8, generator=torch.Generator().manual_seed(9 + j)) * 0.1
        d["rcnn_4"][c] = torch.zeros(24, 128, 4, 4)
    return d


def _load(m):
    sd, sd2 = _roi_state()
    m.load_state_dict(sd, strict=False)
    m.load_state_dict({k: v for k, v in sd2.items() if k.startswith("roi_heads.")}, strict=False)
    m.set_support_dict(_support_dict())
    return m.eval()


@pytest.fixture(scope="module")
def model(ore):
    """The synthetic detector of tests/test_hip_parity.py's inference_many test."""
    from detectron2.modeling import build_model
    cfg = _cfg()
    cfg.freeze()
    return _load(build_model(cfg))


def raw_image(seed, h, w):
    """[h, w, 3] uint8, the synthetic image generator's content."""
    return np.ascontiguousarray(R.synth_image(seed, h, w).numpy().transpose(1, 2, 0))


def pil_request(raw, model, swap=False):
    """The request the CPU mapper would build: Pillow's resize to the model's test size, planar uint8, the raw size as output size."""
    h, w = raw.shape[:2]
    import orehip
    nh, nw = orehip.resize_shortest_edge_shape(h, w, *model._test_size)
    img = pil_resize(raw, nh, nw).transpose(2, 0, 1)
    return {"image": torch.from_numpy(np.ascontiguousarray(img[::-1] if swap else img)), "height": h, "width": w}


def fields(out):
    i = out["instances"]
    return i.image_size, i.pred_boxes.tensor, i.scores, i.pred_classes


def assert_same(got, want, need=1):
    g, w = fields(got), fields(want)
    assert g[0] == w[0] and len(w[2]) >= need, (g[0], w[0], len(w[2]))
    for a, b, name in zip(g[1:], w[1:], ("boxes", "scores", "classes")):
        if not torch.equal(a, b):
            rows = (a != b).reshape(len(a), -1).any(1).nonzero().flatten().tolist() if a.shape == b.shape else "shapes %s / %s" % (a.shape, b.shape)
            raise AssertionError(f"{name} differ in rows {rows}")


@pytest.mark.parametrize("hw", RAW_SIZES, ids=lambda v: "%dx%d" % v)
def test_model_raw_request_equals_pillow_request(model, hw):
    """model([{"image_raw": raw}]) == model([{"image": Pillow-resized, "height", "width"}]): the same engine, the same one-image
    path, the same input bytes -- torch.equal on boxes, scores and classes, for a numpy array, a CPU tensor and a device tensor."""
    raw = raw_image(31 + hw[0], *hw)
    want = model([pil_request(raw, model)])[0]
    assert fields(want)[0] == hw
    for form in (raw, torch.from_numpy(raw), torch.from_numpy(raw).cuda()):
        assert_same(model([{"image_raw": form}])[0], want)
    with pytest.raises(ValueError, match="not both"):
        model([{"image_raw": raw, **pil_request(raw, model)}])
    # an explicit output size is kept
    got = model([{"image_raw": raw, "height": 200, "width": 300}])[0]
    assert_same(got, model([{**pil_request(raw, model), "height": 200, "width": 300}])[0])


def test_model_raw_request_on_the_checked_path(ore, model):
    """The first call of a fresh engine (no cached engine: _inference_checked) takes the raw form too."""
    raw = raw_image(77, *RAW_SIZES[0])
    want = model([pil_request(raw, model)])[0]
    model.set_support_dict(_support_dict())                       # drops the engine key: the next call goes through the checked path
    assert_same(model([{"image_raw": raw}])[0], want)


@pytest.mark.parametrize("fmt", ["BGR", "RGB"])
def test_default_predictor(model, fmt):
    """DefaultPredictor(cfg)(bgr) == the model fed Pillow's resize of the image (BGR) or of its channel-reversed form (RGB)."""
    from detectron2.engine.defaults import DefaultPredictor
    cfg = _cfg(["INPUT.FORMAT", fmt])
    pred = DefaultPredictor(cfg)
    assert pred.input_format == fmt and pred.metadata.name == "coco_2017_val_stone" and not pred.model.training
    _load(pred.model)
    for hw in RAW_SIZES:
        bgr = raw_image(50 + hw[1], *hw)
        want = pred.model([pil_request(bgr, pred.model, swap=(fmt == "RGB"))])[0]
        got = pred(bgr)
        assert_same(got, want)
        if fmt == "BGR":
            assert_same(got, model([{"image_raw": bgr}])[0])
    with pytest.raises(ValueError):
        pred(np.zeros((32, 32), dtype=np.uint8))


def test_inference_many_raw_requests(model):
    """inference_many on raw requests of two sizes (two fold groups) == inference_many on their Pillow-resized forms with the same
    max_fold, request by request; a list that mixes both forms comes back in request order."""
    raws = [raw_image(60 + i, *RAW_SIZES[i % 2]) for i in range(5)]
    want = model.inference_many([pil_request(r, model) for r in raws], max_fold=3)
    got = model.inference_many([{"image_raw": r} for r in raws], max_fold=3)
    assert len(got) == len(want) == 5
    for g, w in zip(got, want):
        assert_same(g, w)
    mixed = model.inference_many([{"image_raw": r} if i % 2 else pil_request(r, model) for i, r in enumerate(raws)], max_fold=3)
    for g, w in zip(mixed, want):
        assert_same(g, w)


def test_nway_raw_request(model):
    """N-way (support_classes = "all", two classes) with image_raw == N-way with the Pillow-resized image."""
    raw = raw_image(91, *RAW_SIZES[1])
    model.set_support_dict(_support_dict((3, 8)))
    model.support_classes = "all"
    try:
        want = model([pil_request(raw, model)])[0]
        got = model([{"image_raw": raw}])[0]
        many = model.inference_many([{"image_raw": raw}])[0]
    finally:
        model.support_classes = None
        model.set_support_dict(_support_dict())
    assert_same(got, want)
    assert_same(many, want)
    assert set(fields(want)[3].tolist()) <= {3, 8}


def test_mapper_device_resize_feeds_the_model(model):
    """DatasetMapperWithSupport(device_resize=True) -> model == the default mapper -> model."""
    from fewx.data.dataset_mapper import DatasetMapperWithSupport
    raw = raw_image(13, 360, 500)
    read = lambda path, format="BGR": raw
    rec = {"file_name": "x.png", "image_id": 1, "height": 360, "width": 500}
    cfg = _cfg()
    a = DatasetMapperWithSupport(cfg, is_train=False, read_image=read)(rec)
    b = DatasetMapperWithSupport(cfg, is_train=False, read_image=read, device_resize=True)(rec)
    assert_same(model([b])[0], model([a])[0])
