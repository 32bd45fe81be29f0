"""GPU: the detection overlay kernel (csrc/ore_overlay.hip) against tests/overlay_ref.py, byte for byte, and what is built on it:
Visualizer on device Instances, VisualizationDemo, AsyncPredictor.  The reference of a frame size is computed once and shared."""
import functools

import numpy as np
import pytest
import torch

import overlay_ref as OR
from test_hip_resize import RAW_SIZES, _cfg, _load, assert_same, fields, raw_image
from test_overlay_host import NAMES, frame

pytestmark = pytest.mark.gpu

BAND = 4096                                                   # guard bytes on either side of a drawn frame (a multiple of 4)
SIZES = [(75, 100), (480, 640), (1080, 1920), (1, 1)]
STYLE = {(75, 100): (1, 1), (480, 640): (3, 2), (1080, 1920): (4, 3), (1, 1): (1, 1)}      # (line width, text scale)


@pytest.fixture(scope="module")
def ore():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import orehip
    orehip.lib()
    return orehip


@functools.lru_cache(maxsize=None)
def case(h, w):
    """(frame, boxes, scores, classes, keyword arguments, reference picture) of one frame size."""
    import orehip
    L, S = STYLE[(h, w)]
    img = frame(h, w, 11)
    b, s, c = OR.cases(h, w, seed=h + w, rows=20)
    kw = dict(score_thresh=0.01, line_width=L, text_scale=S, names=NAMES, palette=orehip.OVERLAY_PALETTE, color_by="class")
    want = OR.overlay_ref(img, b, s, c, atlas=orehip.overlay_atlas(), **kw)
    for a in (img, b, s, c, want):
        a.setflags(write=False)
    return img, b, s, c, kw, want


def guarded_draw(ore_, img, b, s, c, n_dev=None, inplace=False, **kw):
    """overlay_draw into (or inside) the middle of a buffer of 0xA5 bytes; returns the picture and checks both guard bands."""
    n = img.size
    buf = torch.full((n + 2 * BAND,), 0xA5, dtype=torch.uint8, device="cuda")
    out = buf[BAND:BAND + n].view(img.shape)
    src = torch.from_numpy(np.array(img)).cuda()
    dev = lambda a: None if a is None else torch.from_numpy(np.array(a)).cuda()
    if inplace:
        out.copy_(src)
        src = out
    got = ore_.overlay_draw(src, dev(b), dev(s), dev(c), n_dev, out=out, **kw)
    assert got.data_ptr() == out.data_ptr()
    host = buf.cpu().numpy()
    assert (host[:BAND] == 0xA5).all() and (host[BAND + n:] == 0xA5).all(), "bytes outside the frame were written"
    if not inplace:
        assert np.array_equal(src.cpu().numpy(), img), "the source frame of an out-of-place draw changed"
    return host[BAND:BAND + n].reshape(img.shape)


@pytest.mark.parametrize("hw", SIZES, ids=lambda v: "%dx%d" % v)
def test_draw_equals_ref(ore, hw):
    """Out of place, in place, with the row count on the device, and on a non-default stream: the reference's bytes every time."""
    img, b, s, c, kw, want = case(*hw)
    for inplace in (False, True):
        got = guarded_draw(ore, img, b, s, c, inplace=inplace, **kw)
        print(f"{hw[0]}x{hw[1]} inplace={inplace}: {int((got != want).sum())} differing bytes, {int((want != img).any(2).sum())} pixels drawn")
        assert np.array_equal(got, want)
    n_dev = torch.tensor([len(s)], dtype=torch.int32, device="cuda")
    assert np.array_equal(guarded_draw(ore, img, b, s, c, n_dev, **kw), want)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        got = guarded_draw(ore, img, b, s, c, n_dev, inplace=True, **kw)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("hw", [(40, 3), (33, 2), (50, 1), (3, 1030), (2, 2049)], ids=lambda v: "%dx%d" % v)
def test_narrow_and_wide_frames(ore, hw):
    """Frames narrower than a thread's 4 pixels (a span then covers several rows) and wider than a block's 1024 (a run is part of one
    row): the paths of the cull that the common sizes do not take."""
    h, w = hw
    img = frame(h, w, 13)
    b, s, c = OR.cases(h, w, seed=h * w, rows=20)
    b[16:] = [[0.2, 1.5, w - 0.5, h - 0.7], [1.0, 0.0, 2.0, h], [w * 0.5, h * 0.25, w * 0.75, h * 0.9], [0.0, h * 0.5, w, h * 0.5 + 1.0]]
    kw = dict(line_width=1, text_scale=1, names=NAMES, palette=ore.OVERLAY_PALETTE)
    want = OR.overlay_ref(img, b, s, c, atlas=ore.overlay_atlas(), **kw)
    assert (want != img).any()
    for inplace in (False, True):
        assert np.array_equal(guarded_draw(ore, img, b, s, c, inplace=inplace, **kw), want)


def test_device_count_cuts_the_rows(ore):
    """n_dev below, at and above the rows given (the kernel caps it), and 0: the reference of that many rows."""
    h, w = 75, 100
    img, b, s, c, kw, _ = case(h, w)
    for n in (0, 7, len(s), len(s) + 50, -3):
        n_dev = torch.tensor([n], dtype=torch.int32, device="cuda")
        want = OR.overlay_ref(img, b, s, c, min(max(n, 0), len(s)), atlas=ore.overlay_atlas(), **kw)
        assert np.array_equal(guarded_draw(ore, img, b, s, c, n_dev, **kw), want), n
        assert np.array_equal(guarded_draw(ore, img, b, s, c, n_dev, inplace=True, **kw), want), n


def test_320_rows_and_instance_colours(ore):
    """The record's 320 rows, all drawn, coloured by instance (the palette index wraps), labels on; then only the first 200."""
    h, w = 120, 161
    assert int(ore.lib().ore_det_record_rows()) == 320
    rng = np.random.default_rng(3)
    x0, y0 = rng.uniform(-10, w - 5, 320), rng.uniform(-10, h - 5, 320)
    b = np.stack([x0, y0, x0 + rng.uniform(2, 60, 320), y0 + rng.uniform(2, 50, 320)], 1).astype(np.float32)
    s = rng.uniform(0, 1, 320).astype(np.float32)
    c = rng.integers(-1, 7, 320).astype(np.int64)
    img = frame(h, w, 5)
    kw = dict(line_width=2, text_scale=1, names=NAMES, palette=ore.OVERLAY_PALETTE, color_by="instance")
    want = OR.overlay_ref(img, b, s, c, atlas=ore.overlay_atlas(), **kw)
    assert np.array_equal(guarded_draw(ore, img, b, s, c, **kw), want)
    n_dev = torch.tensor([200], dtype=torch.int32, device="cuda")
    assert np.array_equal(guarded_draw(ore, img, b, s, c, n_dev, inplace=True, **kw), OR.overlay_ref(img, b, s, c, 200, atlas=ore.overlay_atlas(), **kw))
    # no classes, no names, no labels, a one-colour palette
    kw = dict(line_width=16, text_scale=0, edge_alpha=255, palette=np.array([[1, 2, 3]], np.uint8))
    assert np.array_equal(guarded_draw(ore, img, b, s, None, **kw), OR.overlay_ref(img, b, s, None, atlas=ore.overlay_atlas(), **kw))
    kw = dict(line_width=1, text_scale=8, label_alpha=0, palette=ore.OVERLAY_PALETTE)
    assert np.array_equal(guarded_draw(ore, img, b[:9], s[:9], None, **kw), OR.overlay_ref(img, b[:9], s[:9], None, atlas=ore.overlay_atlas(), **kw))


def test_two_runs_are_bit_equal(ore):
    img, b, s, c, kw, want = case(480, 640)
    a = guarded_draw(ore, img, b, s, c, **kw)
    assert np.array_equal(a, guarded_draw(ore, img, b, s, c, **kw)) and np.array_equal(a, want)


def test_33_palettes_evict_the_oldest_tables(ore):
    """The table cache holds 32: 33 distinct two-colour palettes (beside the atlas and the names) push the oldest tables out, the atlas
    and the first palette among them, and a draw with the first palette afterwards uploads them again -- overlay_host's bytes every time."""
    h, w = 32, 48
    img = frame(h, w, 17)
    b, s, c = OR.cases(h, w, seed=h + w, rows=6)
    pals = [np.array([[7 * i + 1, 255 - 5 * i, 90], [3 * i, 40 + i, 200 - 2 * i]], np.uint8) for i in range(33)]
    assert len({p.tobytes() for p in pals}) == 33
    ore._OVERLAY_TABLES.clear()
    for pal in pals + pals[:1]:
        kw = dict(line_width=1, text_scale=1, names=NAMES, palette=pal, color_by="class")
        want = ore.overlay_host(img, b, s, c, **kw)
        assert (want != img).any()
        assert np.array_equal(guarded_draw(ore, img, b, s, c, **kw), want)
        assert len(ore._OVERLAY_TABLES) <= ore._OVERLAY_TABLES_MAX == 32
    assert len(ore._OVERLAY_TABLES) == 32


def test_limits_are_errors(ore):
    img = torch.zeros(16, 16, 3, dtype=torch.uint8, device="cuda")
    b = torch.tensor([[1.0, 1.0, 9.0, 9.0]], device="cuda")
    s = torch.tensor([0.5], device="cuda")
    ok = dict(line_width=1, text_scale=1)
    ore.overlay_draw(img, b, s, **ok)
    for kw in (dict(line_width=0, text_scale=1), dict(line_width=17, text_scale=1), dict(line_width=1, text_scale=9),
               dict(line_width=1, text_scale=-1), dict(ok, edge_alpha=256), dict(ok, label_alpha=-1),
               dict(ok, palette=np.zeros((257, 3), np.uint8)), dict(ok, color_by="area")):
        with pytest.raises(ore.OreError):
            ore.overlay_draw(img, b, s, **kw)
    with pytest.raises(ore.OreError, match="max_rows"):
        ore.overlay_draw(img, torch.zeros(321, 4, device="cuda"), torch.zeros(321, device="cuda"), **ok)
    for shape in ((1, 8193, 3), (8193, 1, 3)):
        with pytest.raises(ore.OreError, match="sides"):
            ore.overlay_draw(torch.zeros(shape, dtype=torch.uint8, device="cuda"), b, s, **ok)
    buf = torch.zeros(16 * 16 * 3 + 8, dtype=torch.uint8, device="cuda")
    with pytest.raises(ore.OreError, match="aligned"):
        ore.overlay_draw(buf[1:1 + 768].view(16, 16, 3), b, s, **ok)
    with pytest.raises(ore.OreError, match="overlap"):
        ore.overlay_draw(buf[0:768].view(16, 16, 3), b, s, out=buf[4:772].view(16, 16, 3), **ok)
    for bad in (torch.tensor([1], dtype=torch.int64, device="cuda"), torch.tensor([1.0], device="cuda"), torch.tensor([1], dtype=torch.int32), 1):
        with pytest.raises(ore.OreError, match="n_dev"):      # the count is an int32 word on the frame's device
            ore.overlay_draw(img, b, s, None, bad, **ok)
    assert int(ore.lib().ore_overlay_workspace_bytes(321)) == 0 and int(ore.lib().ore_overlay_workspace_bytes(320)) > 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ the detectron2 names
def test_visualizer_device_equals_host(ore):
    """Visualizer.draw_instance_predictions on device Instances (the kernel) == on .to("cpu") Instances (overlay_host) == the
    reference, in both colour modes; VideoVisualizer likewise."""
    from detectron2.data import Metadata
    from detectron2.structures import Boxes, Instances
    from detectron2.utils.video_visualizer import VideoVisualizer
    from detectron2.utils.visualizer import ColorMode, Visualizer, default_overlay_params
    h, w = 300, 500
    img = frame(h, w, 2)
    b, s, c = OR.cases(h, w, seed=8, rows=20)
    keep = np.isfinite(b).all(1) & np.isfinite(s)
    inst = Instances((h, w))
    inst.pred_boxes = Boxes(torch.from_numpy(b[keep]).cuda())
    inst.scores = torch.from_numpy(s[keep]).cuda()
    inst.pred_classes = torch.from_numpy(c[keep]).cuda()
    meta = Metadata(name="t", thing_classes=NAMES)
    for mode, color_by in ((ColorMode.IMAGE, "instance"), (ColorMode.SEGMENTATION, "class")):
        dev = Visualizer(img, meta, instance_mode=mode).draw_instance_predictions(inst)
        assert torch.is_tensor(dev.img) and dev.img.is_cuda
        host = Visualizer(img, meta, instance_mode=mode).draw_instance_predictions(inst.to("cpu"))
        want = OR.overlay_ref(img, b[keep], s[keep], c[keep], atlas=ore.overlay_atlas(), palette=ore.OVERLAY_PALETTE, names=NAMES,
                              color_by=color_by, **default_overlay_params(h, w))
        assert np.array_equal(dev.get_image(), want) and np.array_equal(host.get_image(), want)
    dev = VideoVisualizer(meta).draw_instance_predictions(torch.from_numpy(img).cuda(), inst)
    assert np.array_equal(dev.get_image(), VideoVisualizer(meta).draw_instance_predictions(img, inst.to("cpu")).get_image())


@pytest.fixture(scope="module")
def pred(ore):
    """DefaultPredictor over the synthetic detector of tests/test_hip_resize.py: the one-image reference of everything below."""
    from detectron2.engine.defaults import DefaultPredictor
    p = DefaultPredictor(_cfg())
    _load(p.model)
    return p


def ref_picture(ore, bgr, out, color_by, names=None):
    """overlay_ref of a result's rows on the BGR frame, with the defaults of the demo."""
    from detectron2.utils.visualizer import default_overlay_params
    _, boxes, scores, classes = fields(out)
    return OR.overlay_ref(bgr, boxes.cpu().numpy(), scores.cpu().numpy(), classes.cpu().numpy(), atlas=ore.overlay_atlas(),
                          palette=ore.OVERLAY_PALETTE[:, ::-1], color_by=color_by, names=names, **default_overlay_params(*bgr.shape[:2]))


def test_visualization_demo_run_on_image(ore, pred):
    from detectron2.utils.visualizer import ColorMode
    from predictor import VisualizationDemo
    demo = VisualizationDemo(_cfg(), instance_mode=ColorMode.SEGMENTATION)
    _load(demo.predictor.model)
    saved = demo.metadata.get("thing_classes")
    demo.metadata.set(thing_classes=["stone"])
    try:
        for hw in RAW_SIZES:
            bgr = raw_image(40 + hw[0], *hw)
            want = pred(bgr)
            got, vis = demo.run_on_image(bgr)
            assert_same(got, want)
            picture = ref_picture(ore, bgr, want, "class", ["stone"])
            assert (picture != bgr).any() and np.array_equal(vis.get_image(), picture[:, :, ::-1])
    finally:
        demo.metadata.pop("thing_classes", None)
        if saved is not None:
            demo.metadata.set(thing_classes=saved)


@pytest.fixture(scope="module")
def apred(ore):
    from predictor import AsyncPredictor
    ap = AsyncPredictor(_cfg(), inflight=4)
    _load(ap.model)
    yield ap
    ap.shutdown()


def test_async_predictor_order_results_and_pictures(ore, pred, apred):
    """12 frames of two sizes with up to 4 pending: every result torch.equal to DefaultPredictor's, in put order, and every vis_image
    the reference picture of those rows; the input frames are left as they were."""
    from detectron2.utils.visualizer import thing_classes
    names = thing_classes(apred.metadata)
    frames = [raw_image(70 + i, *RAW_SIZES[i % 2]) for i in range(12)]
    frames[5] = torch.from_numpy(frames[5])                                   # a CPU tensor
    frames[6] = torch.from_numpy(frames[6]).cuda()                             # a device tensor: drawn out of place
    as_np = lambda f: f.cpu().numpy() if torch.is_tensor(f) else f
    before = [as_np(f).copy() for f in frames]
    want = [pred(as_np(f)) for f in frames]
    assert apred.default_buffer_size == 4 and len(apred) == 0
    got = []
    for i, f in enumerate(frames):
        if len(apred) == apred.default_buffer_size:
            got.append(apred.get())
        apred.put(f, draw=(i % 3 != 2))                                        # every third frame without a picture
        assert len(apred) <= 4
    assert len(apred) == 4
    while len(apred):
        got.append(apred.get())
    with pytest.raises(IndexError):
        apred.get()
    assert len(got) == 12
    for i, (g, w_, f0) in enumerate(zip(got, want, before)):
        assert_same(g, w_)
        assert np.array_equal(as_np(frames[i]), f0)
        if i % 3 != 2:
            vis = g["vis_image"]
            assert vis.is_cuda and np.array_equal(vis.cpu().numpy(), ref_picture(ore, f0, w_, "instance", names)), i
        else:
            assert "vis_image" not in g
    assert_same(apred(before[0]), want[0])                                     # __call__ = put + get


def test_async_predictor_cold_tables_on_several_streams(ore, pred):
    """A fresh AsyncPredictor with every cached device table dropped (resize tables, atlas, palette, names), frames of alternating
    sizes, drawn: slot 0's stream uploads a table behind its own work and slot 1's stream uses it at once.  The use waits for the
    upload's event, so results and pictures are the reference's from the first frame on.  A long frame goes first, so that the
    uploading stream is the busy one."""
    from detectron2.utils.visualizer import thing_classes
    from predictor import AsyncPredictor
    ap = AsyncPredictor(_cfg(), inflight=4)
    _load(ap.model)
    names = ["stone"]
    big, small = (1080, 1920), RAW_SIZES[1]
    frames = [raw_image(200 + i, *(big if i % 4 == 0 else small)) for i in range(8)]
    want = [pred(f) for f in frames]
    try:
        ap.put(frames[0])                                     # engines and graphs exist; nothing was drawn, nothing of `small` resized
        ap.get()
        torch.cuda.synchronize()
        ore._RESIZE_TABLES.clear()
        ore._OVERLAY_TABLES.clear()
        got = []
        for f in frames:
            if len(ap) == ap.default_buffer_size:
                got.append(ap.get())
            ap.put(f, draw={"names": names})
        while len(ap):
            got.append(ap.get())
    finally:
        ap.shutdown()
    for i, (g, w_, f) in enumerate(zip(got, want, frames)):
        assert_same(g, w_)
        assert np.array_equal(g["vis_image"].cpu().numpy(), ref_picture(ore, f, w_, "instance", names)), i


def test_async_predictor_refuses_bad_draw_arguments_with_the_engine_idle(ore, pred, apred):
    """Bad overlay arguments are refused before the frame's pass begins, and a draw that fails after it began ends the pass: the
    same slot takes the next frame either way."""
    bgr = raw_image(34, *RAW_SIZES[0])
    want = pred(bgr)
    for draw in ({"colour": "red"}, {"line_width": 0}, {"text_scale": 9}, {"color_by": "area"}, {"palette": np.zeros((0, 3), np.uint8)}, "yes"):
        with pytest.raises(ValueError):
            apred.put(bgr, draw=draw)
        assert len(apred) == 0
    assert_same(apred(bgr), want)
    slot = apred._slots[apred._next]
    with pytest.raises(TypeError):                             # passes the host checks, fails inside overlay_draw, after detect_begin
        apred.put(bgr, draw={"names": 5})
    assert len(apred) == 0 and apred._slots[apred._next] is slot
    apred.put(bgr, draw=True)                                  # the same slot's engine is free again
    assert_same(apred.get(), want)


def test_async_predictor_sees_a_weight_edit(apred):
    """A weight edit between two puts: the pass already pending finishes on the old engines, the next one runs on rebuilt engines and
    equals the one-image predictor over the same (edited) model."""
    bgr = raw_image(33, *RAW_SIZES[0])
    one = apred.predictor
    before = one(bgr)
    w = apred.model.conv3.weight
    saved = w.detach().clone()
    apred.put(bgr)
    engines = [s.engine for s in apred._slots]
    try:
        with torch.no_grad():
            w.mul_(0.5)
        apred.put(bgr)
        assert len(apred) == 2 and all(a is not b for a, b in zip(engines, [s.engine for s in apred._slots]))
        first, second = apred.get(), apred.get()
        edited = one(bgr)
    finally:
        with torch.no_grad():
            w.copy_(saved)
    assert_same(first, before)
    assert_same(second, edited, need=0)
    assert not (fields(edited)[2].shape == fields(before)[2].shape and torch.equal(fields(edited)[2], fields(before)[2]))
    assert_same(apred(bgr), before)


def test_async_predictor_drawn_path_issues_no_sync(ore, pred, apred):
    """put(..., draw=True) enqueues upload, resize, pass and overlay without a host synchronisation torch knows of (sync debug mode
    "error"); the wait is get's."""
    frames = [raw_image(90 + i, *RAW_SIZES[0]) for i in range(4)]
    want = [pred(f) for f in frames]
    for f in frames:                                          # engines, graphs, tables, staging buffers: built outside the measured calls
        apred.put(f, draw=True)
    while len(apred):
        apred.get()
    dev_frame = torch.from_numpy(frames[3]).cuda()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):                      # the mode is live: a read-back raises
            torch.ones(1, device="cuda").item()
        for f in frames[:3] + [dev_frame]:
            apred.put(f, draw=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for f, w_ in zip(frames, want):
        g = apred.get()
        assert_same(g, w_)
        assert np.array_equal(g["vis_image"].cpu().numpy(), ref_picture(ore, f, w_, "instance", getattr(apred.metadata, "thing_classes", None)))


def test_run_on_video_parallel_equals_serial(ore, pred):
    """run_on_video over a list of frames and over a capture-like object, parallel and not: the same annotated BGR frames, in order,
    equal to the reference picture of DefaultPredictor's rows (coloured by class)."""
    from detectron2.utils.visualizer import thing_classes
    from predictor import VisualizationDemo

    class Capture:
        def __init__(self, frames):
            self.frames = list(frames)

        def isOpened(self):
            return True

        def read(self):
            return (True, self.frames.pop(0)) if self.frames else (False, None)

    frames = [raw_image(120 + i, *RAW_SIZES[i % 2]) for i in range(6)]
    serial = VisualizationDemo(_cfg(), parallel=False)
    _load(serial.predictor.model)
    par = VisualizationDemo(_cfg(), parallel=True)
    _load(par.predictor.model)
    names = thing_classes(serial.metadata)
    try:
        a = list(serial.run_on_video(frames))
        b = list(par.run_on_video(iter(frames)))
        c = list(par.run_on_video(Capture(frames)))
        got, vis = par.run_on_image(frames[1])                                  # the parallel demo draws one image through put / get
    finally:
        par.predictor.shutdown()
    assert_same(got, pred(frames[1]))
    assert np.array_equal(vis.get_image(), ref_picture(ore, frames[1], got, "instance", names)[:, :, ::-1])
    assert len(a) == len(b) == len(c) == 6
    for i, f in enumerate(frames):
        want = ref_picture(ore, f, pred(f), "class", names)
        assert isinstance(a[i], np.ndarray) and a[i].shape == f.shape
        assert np.array_equal(a[i], want) and np.array_equal(b[i], want) and np.array_equal(c[i], want), i
