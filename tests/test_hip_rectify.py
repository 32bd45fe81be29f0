"""GPU: k_rectify_u8 (csrc/ore_rectify.hip) against orehip.rectify_host, byte for byte, on the case table of tests/rectify_ref.py --
outputs whose rows start at every misalignment, more than one workgroup in both directions, a 1 x 1 source, a horizon, an output that
lies wholly outside the source -- with guard bands, out=, a side stream and the refusals; then rectify= of DefaultPredictor,
AsyncPredictor, VisualizationDemo, TiledPredictor and demo.py on the synthetic detector of tests/test_hip_resize.py."""
import ctypes

import numpy as np
import pytest
import torch

import rectify_ref as RR
from test_hip_resize import _cfg, _load, raw_image

pytestmark = pytest.mark.gpu

BAND = 4096
FRAME_HW, OUT_HW = (300, 500), (288, 416)
FRAME_QUAD = [(60, 20), (460, 30), (490, 280), (10, 270)]


@pytest.fixture(scope="module")
def ore():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import orehip
    orehip.lib()
    return orehip


def guarded(ore_, src, M, out_hw, fill=(0, 0, 0), lead=0, src_lead=0):
    """rectify_u8 into the middle of a buffer of 0xA5 bytes, `lead` bytes off a 4-byte boundary, from a source `src_lead` bytes off
    one; returns the output and checks both guard bands."""
    ho, wo = out_hw
    n = ho * wo * 3
    buf = torch.full((n + 2 * BAND + 4,), 0xA5, dtype=torch.uint8, device="cuda")
    out = buf[BAND + lead:BAND + lead + n].view(ho, wo, 3)
    sbuf = torch.empty(src.size + 4, dtype=torch.uint8, device="cuda")
    dsrc = sbuf[src_lead:src_lead + src.size].view(src.shape)
    dsrc.copy_(torch.from_numpy(src))
    got = ore_.rectify_u8(dsrc, M, out_hw, fill, out=out)
    assert got.data_ptr() == out.data_ptr()
    host = buf.cpu().numpy()
    assert (host[:BAND + lead] == 0xA5).all() and (host[BAND + lead + n:] == 0xA5).all(), "bytes outside the output were written"
    return host[BAND + lead:BAND + lead + n].reshape(ho, wo, 3)


@pytest.mark.parametrize("case", RR.CASE_IDS)
def test_device_equals_host(ore, case):
    _, hw, out_hw, M, fill = RR.CASES[RR.CASE_IDS.index(case)]
    src = RR.source(*hw)
    want = ore.rectify_host(src, M, out_hw, fill)
    got = ore.rectify_u8(torch.from_numpy(src).cuda(), M, out_hw, fill)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (*out_hw, 3) and got.is_contiguous()
    assert torch.equal(got.cpu(), torch.from_numpy(want)), np.argwhere((got.cpu().numpy() != want).any(2))[:5]
    assert np.array_equal(guarded(ore, src, M, out_hw, fill), want)


@pytest.mark.parametrize("lead", [1, 2, 3])
def test_every_alignment_of_output_and_source(ore, lead):
    """The output starts 1, 2 and 3 bytes off a 4-byte boundary (so do all its rows' heads and tails), the source likewise: the 8-byte
    tap loads and the word stores hold at any address."""
    for (hs, ws), (ho, wo) in (((33, 65), (64, 67)), ((96, 300), (70, 260)), ((5, 7), (3, 5))):
        src = RR.source(hs, ws)
        for M in (RR.matrices(hs, ws, ho, wo)["perspective"], RR.matrices(hs, ws, ho, wo)["shift"]):
            want = ore.rectify_host(src, M, (ho, wo), (7, 8, 9))
            assert np.array_equal(guarded(ore, src, M, (ho, wo), (7, 8, 9), lead=lead, src_lead=4 - lead), want)


def test_identity_shift_and_the_largest_sides(ore):
    src = RR.source(33, 65)
    dev = torch.from_numpy(src).cuda()
    assert torch.equal(ore.rectify_u8(dev, np.eye(3), (33, 65)), dev)
    for hw in ((1, 16384), (16384, 1)):                          # the contract's largest extent, one pixel wide: 256 and 1024 workgroups
        line = RR.source(*hw)
        d = torch.from_numpy(line).cuda()
        assert torch.equal(ore.rectify_u8(d, np.eye(3), hw), d)
        M = [[1, 0, 0.5], [0, 1, 0.5], [0, 0, 1]]
        assert torch.equal(ore.rectify_u8(d, M, hw).cpu(), torch.from_numpy(ore.rectify_host(line, M, hw)))


def test_side_stream_and_rectifier(ore):
    (hs, ws), (ho, wo) = (96, 300), (70, 260)
    src = RR.source(hs, ws)
    R = ore.Rectifier(RR.matrices(hs, ws, ho, wo)["perspective"], out_hw=(ho, wo), fill=(3, 2, 1))
    want = torch.from_numpy(R(src))
    dev = torch.from_numpy(src).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = R(dev)
        out = torch.empty(ho, wo, 3, dtype=torch.uint8, device="cuda")
        assert R(dev, out=out) is out
    s.synchronize()
    assert torch.equal(got.cpu(), want) and torch.equal(out.cpu(), want)


def test_launch_can_be_captured(ore):
    """No table and no upload: the launch replays from a graph on new source bytes."""
    (hs, ws), (ho, wo) = (33, 65), (64, 67)
    M = RR.matrices(hs, ws, ho, wo)["perspective"]
    a, b = RR.source(hs, ws), RR.source(ws, hs).reshape(hs, ws, 3)
    dev = torch.from_numpy(a).cuda()
    out = torch.zeros(ho, wo, 3, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ore.rectify_u8(dev, M, (ho, wo), out=out)                # warm: nothing is allocated during the capture
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            ore.rectify_u8(dev, M, (ho, wo), out=out)
    torch.cuda.synchronize()
    dev.copy_(torch.from_numpy(b))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), torch.from_numpy(ore.rectify_host(b, M, (ho, wo))))


def test_refusals(ore):
    src = torch.from_numpy(RR.source(5, 7)).cuda()
    eye = np.eye(3)
    for bad in (src.float(), src[:, :, :2], src[0], src.permute(1, 0, 2), src.cpu()):
        with pytest.raises(ValueError, match="rectify_u8"):
            ore.rectify_u8(bad, eye, (5, 7))
    for M in (np.eye(2), [[1, 0, 0], [0, 1, 0], [0, float("nan"), 1]]):
        with pytest.raises(ValueError, match="M "):
            ore.rectify_u8(src, M, (5, 7))
    for hw in ((0, 7), (5, 16385)):
        with pytest.raises(ValueError, match="out_hw"):
            ore.rectify_u8(src, eye, hw)
    with pytest.raises(ValueError, match="fill"):
        ore.rectify_u8(src, eye, (5, 7), (0, 0, 300))
    good = torch.empty(5, 7, 3, dtype=torch.uint8, device="cuda")
    for out in (good.cpu(), good.float(), torch.empty(5, 8, 3, dtype=torch.uint8, device="cuda"), good.permute(1, 0, 2), src):
        with pytest.raises(ValueError, match="out"):
            ore.rectify_u8(src, eye, (5, 7), out=out)
    both = torch.empty(5 * 7 * 3 + 6, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="overlaps"):
        ore.rectify_u8(both[:105].view(5, 7, 3), eye, (5, 7), out=both[6:].view(5, 7, 3))
    # the C entry, on real buffers: ORE_EINVAL, and the output is left as it was
    L = ore.lib()
    dst = torch.full((3, 5, 3), 0xA5, dtype=torch.uint8, device="cuda")
    m9 = lambda *v: (ctypes.c_float * 9)(*(v or (1, 0, 0, 0, 1, 0, 0, 0, 1)))
    ok = dict(src=src.data_ptr(), hs=5, ws=7, m=m9(), dst=dst.data_ptr(), ho=3, wo=5, fill=0)
    for bad in (dict(src=None), dict(dst=None), dict(m=None), dict(hs=0), dict(ws=16385), dict(ho=0), dict(wo=16385),
                dict(m=m9(1, 0, 0, 0, 1, 0, 0, 0, float("nan"))), dict(m=m9(float("-inf"), 0, 0, 0, 1, 0, 0, 0, 1)), dict(fill=1 << 24),
                dict(dst=src.data_ptr()), dict(dst=src.data_ptr() + 104)):
        a = dict(ok, **bad)
        rc = L.ore_rectify_u8_fwd(a["src"], a["hs"], a["ws"], a["m"], a["dst"], a["ho"], a["wo"], a["fill"], None)
        assert rc == -22 and L.ore_last_error().startswith(b"ore_rectify_u8_fwd"), (bad, rc)
    torch.cuda.synchronize()
    assert (dst == 0xA5).all() and torch.equal(src.cpu(), torch.from_numpy(RR.source(5, 7)))


# ------------------------------------------------------------------------------------------ the wrappers
def fields(out):
    i = out["instances"]
    return i.image_size, i.pred_boxes.tensor, i.scores, i.pred_classes


def assert_same(got, want, need=1):
    g, w = fields(got), fields(want)
    assert g[0] == w[0] and len(w[2]) >= need, (g[0], w[0], len(w[2]))
    for a, b, name in zip(g[1:], w[1:], ("boxes", "scores", "classes")):
        assert torch.equal(a, b), name


@pytest.fixture(scope="module")
def rect(ore):
    return ore.Rectifier(quad=FRAME_QUAD, out_hw=OUT_HW, fill=(104, 116, 124))


@pytest.fixture(scope="module")
def plain(ore):
    """DefaultPredictor without rectification: what every rectified wrapper is compared with, fed rectify_host's frame."""
    from detectron2.engine.defaults import DefaultPredictor
    pred = DefaultPredictor(_cfg())
    assert pred.rectify is None
    _load(pred.model)
    return pred


@pytest.fixture(scope="module")
def rectified(ore, rect):
    from detectron2.engine.defaults import DefaultPredictor
    pred = DefaultPredictor(_cfg(), rectify=rect)
    _load(pred.model)
    return pred


def flat(rect, frame):
    return np.ascontiguousarray(rect(frame))


def test_default_predictor_host_frame(ore, rect, plain, rectified):
    for seed in (41, 42):
        frame = raw_image(seed, *FRAME_HW)
        want = plain(flat(rect, frame))
        got = rectified(frame)
        assert fields(got)[0] == OUT_HW
        assert_same(got, want)
        assert_same(rectified(torch.from_numpy(frame)), want)
    with pytest.raises(ValueError):
        rectified(np.zeros((32, 32), dtype=np.uint8))
    from detectron2.engine.defaults import DefaultPredictor
    with pytest.raises(ValueError, match="rectify"):
        DefaultPredictor(_cfg(), rectify="quad")


def test_default_predictor_device_frame(ore, rect, plain, rectified):
    frame = raw_image(43, *FRAME_HW)
    dev = torch.from_numpy(frame).cuda()
    assert_same(rectified(dev), plain(flat(rect, frame)))
    assert torch.equal(dev.cpu(), torch.from_numpy(frame))       # the caller's frame is left as it was


def test_async_predictor_alternating(ore, rect, plain):
    """Six frames through four slots, every other one rectified: the instances are DefaultPredictor's on rectify_host's frame (or on
    the frame itself), "vis_image" is overlay_host drawn on that frame, and put does not synchronise."""
    from detectron2.utils.visualizer import default_overlay_params, thing_classes
    from predictor import AsyncPredictor
    ap = AsyncPredictor(_cfg(), inflight=4)
    _load(ap.model)
    names = thing_classes(ap.metadata)
    frames = [raw_image(80 + i, *FRAME_HW) for i in range(6)]
    frames[3] = torch.from_numpy(frames[3]).cuda()                 # a device frame, rectified: drawn on the slot's own tensor
    seen = [flat(rect, f.cpu().numpy() if torch.is_tensor(f) else f) if i % 2 else np.asarray(f) for i, f in enumerate(frames)]
    want = [plain(s) for s in seen]
    got = []
    try:
        ap.put(frames[0], draw=True, rectify=rect)                # engines, graphs and tables exist
        ap.put(frames[0], draw=True)
        ap.get(), ap.get()
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            for i, f in enumerate(frames[:4]):
                ap.put(f, draw=True, rectify=rect if i % 2 else None)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        got.append(ap.get())
        for i, f in enumerate(frames[4:], 4):
            ap.put(f, draw=True, rectify=rect if i % 2 else None)
        while len(ap):
            got.append(ap.get())
        with pytest.raises(ValueError, match="rectify"):
            ap.put(frames[0], rectify=np.eye(3))
    finally:
        ap.shutdown()
    assert len(got) == 6
    for i, (g, w, s) in enumerate(zip(got, want, seen)):
        assert fields(g)[0] == (OUT_HW if i % 2 else FRAME_HW)
        assert_same(g, w)
        _, b, sc, c = fields(w)
        picture = ore.overlay_host(s, b.cpu().numpy(), sc.cpu().numpy(), c.cpu().numpy(), palette=np.ascontiguousarray(ore.OVERLAY_PALETTE[:, ::-1]),
                                   color_by="instance", names=names, **default_overlay_params(*s.shape[:2]))
        assert (picture != s).any() and torch.equal(g["vis_image"].cpu(), torch.from_numpy(picture)), i
    assert torch.equal(frames[3].cpu(), torch.from_numpy(raw_image(83, *FRAME_HW)))


def test_visualization_demo_belt_frame_is_out_hw(ore, rect):
    from predictor import VisualizationDemo
    cfg = _cfg(["MODEL.ROI_HEADS.SCORE_THRESH_TEST", 0.0])
    raw = raw_image(300, *FRAME_HW)
    frames = [np.ascontiguousarray(np.roll(raw, f * 16, 1)) for f in range(3)]
    demos = [VisualizationDemo(cfg, rectify=rect, track="belt", parallel=par) for par in (False, True)]
    try:
        outs = []
        for d in demos:
            _load(d.predictor.model)
            outs.append(list(d.run_on_video(iter(frames))))
            p = d.tracker.belt_params
            assert type(d.tracker) is ore.BeltTracker and (p["frame_h"], p["frame_w"]) == OUT_HW and d.track_stats()["frames"] == 3
        assert all(o.shape == (*OUT_HW, 3) for out in outs for o in out) and len(outs[0]) == len(outs[1]) == 3
        assert all(np.array_equal(a, b) for a, b in zip(*outs))
        predictions, vis = demos[0].run_on_image(frames[0])
        assert predictions["instances"].image_size == OUT_HW and tuple(vis.get_image().shape) == (*OUT_HW, 3)
    finally:
        demos[1].predictor.shutdown()
    with pytest.raises(ValueError, match="rectify"):
        VisualizationDemo(cfg, rectify=np.eye(3))


def test_tiled_predictor(ore):
    """A 96 x 300 frame rectified (magnified) to 700 x 900 in front of the tile gather, against the same predictor fed rectify_host's
    frame."""
    from predictor import TiledPredictor
    R = ore.Rectifier(quad=[(5, 3), (290, 8), (297, 90), (2, 93)], out_hw=(700, 900))
    pred = TiledPredictor(_cfg(), rectify=R, tile=320, overlap=96)
    same = TiledPredictor(_cfg(), tile=320, overlap=96)
    _load(pred.model), _load(same.model)
    assert len(pred.tiled.plan(700, 900)[0]["origins"]) > 4
    frame = raw_image(55, 96, 300)
    want = same(flat(R, frame))
    assert fields(want)[0] == (700, 900)
    assert_same(pred(frame), want)
    assert_same(pred(torch.from_numpy(frame).cuda()), want)


def test_demo_writes_the_rectified_size(ore, tmp_path, monkeypatch):
    from PIL import Image
    import demo
    import predictor

    class Demo(predictor.VisualizationDemo):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            _load(self.predictor.model)

    monkeypatch.setattr(predictor, "VisualizationDemo", Demo)
    src, dst = str(tmp_path / "in.png"), str(tmp_path / "out.png")
    Image.fromarray(raw_image(61, *FRAME_HW)[:, :, ::-1].copy()).save(src)
    quad = [str(v) for p in FRAME_QUAD for v in p]
    demo.main(["--input", src, "--output", dst, "--rectify-quad", *quad, "--rectify-size", str(OUT_HW[1]), str(OUT_HW[0]), "--confidence-threshold",
               "0.0", "--opts", "MODEL.DEVICE", "cuda", "MODEL.WEIGHTS", "", "INPUT.MAX_SIZE_TEST", "640"])
    with Image.open(dst) as im:
        assert im.size == (OUT_HW[1], OUT_HW[0])
