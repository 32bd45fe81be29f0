"""GPU: the heat-map kernels (csrc/ore_heatmap.hip) against tests/heatmap_ref.py, byte for byte, and what is built on them:
Engine.heat_source, VisualizationDemo(heatmap=...), AsyncPredictor.put(heatmap=...).  A reference is computed once and shared."""
import numpy as np
import pytest
import torch

import heatmap_ref as HR
import overlay_ref as OR
from test_hip_resize import RAW_SIZES, _cfg, _load, _support_dict, assert_same, raw_image

pytestmark = pytest.mark.gpu

BAND = 4096                                                   # guard bytes on either side of a drawn frame (a multiple of 4)


@pytest.fixture(scope="module")
def ore():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import orehip
    orehip.lib()
    return orehip


def dev_pairs(maps, strides):
    return [(torch.from_numpy(np.array(m)).cuda(), s) for m, s in zip(maps, strides)]


def guarded_draw(ore_, img, maps, strides, in_hw, inplace=False, **style):
    """heatmap_draw into (or inside) the middle of a buffer of 0xA5 bytes; returns the picture and checks both guard bands."""
    n = img.size
    buf = torch.full((n + 2 * BAND,), 0xA5, dtype=torch.uint8, device="cuda")
    out = buf[BAND:BAND + n].view(img.shape)
    src = torch.from_numpy(np.array(img)).cuda()
    if inplace:
        out.copy_(src)
        src = out
    got = ore_.heatmap_draw(src, dev_pairs(maps, strides), in_hw, out=out, **style)
    assert got.data_ptr() == out.data_ptr()
    host = buf.cpu().numpy()
    assert (host[:BAND] == 0xA5).all() and (host[BAND + n:] == 0xA5).all(), "bytes outside the frame were written"
    if not inplace:
        assert np.array_equal(src.cpu().numpy(), img), "the source frame of an out-of-place draw changed"
    return host[BAND:BAND + n].reshape(img.shape)


# ------------------------------------------------------------------------------------------ render (stages C + D)
@pytest.mark.parametrize("hw", HR.FRAMES, ids=lambda v: "%dx%d" % v)
def test_render_equals_ref(ore, hw):
    """Three levels 5x7 / 3x4 / 2x2 at in_hw (40, 56): out of place, in place and on a non-default stream; on the small frames also
    every style (alpha 0 / 128 / 178 / 255, both alpha modes, gray / jet / a random table), one level only, and an input size that is
    no multiple of the strides."""
    img, maps, strides, in_hw, style, want = HR.render_case(hw)
    for inplace in (False, True):
        got = guarded_draw(ore, img, maps, strides, in_hw, inplace=inplace, **style)
        print(f"{hw[0]}x{hw[1]} inplace={inplace}: {int((got != want).sum())} differing bytes")
        assert np.array_equal(got, want)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        got = guarded_draw(ore, img, maps, strides, in_hw, inplace=True, **style)
    assert np.array_equal(got, want)
    if hw[0] * hw[1] > 10000:
        return
    for si in range(1, len(HR.STYLES)):
        img, maps, strides, in_hw, style, want = HR.render_case(hw, si)
        for inplace in (False, True):
            assert np.array_equal(guarded_draw(ore, img, maps, strides, in_hw, inplace=inplace, **style), want), (si, inplace)
    for n_levels, in_hw in ((1, HR.IN_HW), (3, (43, 61)), (2, (43, 61))):
        img, maps, strides, in_hw, style, want = HR.render_case(hw, 0, n_levels, in_hw)
        assert np.array_equal(guarded_draw(ore, img, maps, strides, in_hw, **style), want), (n_levels, in_hw)


def test_render_large_geometry(ore):
    """Where the tap numerator (2x + 1) * in_w * 256 passes 2^32: an 8192-wide input drawn onto a 3 x 8190 frame at stride 128."""
    rng = np.random.default_rng(8)
    maps, strides, in_hw = [rng.integers(0, 256, (3, 64), dtype=np.uint8)], (128,), (300, 8192)
    img = HR.frame(3, 8190, 1)
    assert (2 * 8189 + 1) * 8192 * 256 > 2 ** 32
    want = HR.heatmap_ref(img, maps, strides, in_hw, lut="jet", alpha=200)
    assert np.array_equal(guarded_draw(ore, img, maps, strides, in_hw, lut="jet", alpha=200), want)


@pytest.mark.parametrize("case", ["narrow-frame-large-map", "downscale-of-large-maps", "wide-map-2048", "wide-map-2049"])
def test_render_large_maps(ore, case):
    """Maps far larger than the 5x7 / 3x4 / 2x2 ones above: a 3-pixel-wide frame whose blocks span hundreds of frame rows over a
    512 x 512 map, a downscale of two large maps (neighbouring pixels' taps are rows apart), and rows wider than a block's run of
    pixels, of a width that is and is not a multiple of 4."""
    rng = np.random.default_rng(12)
    if case == "narrow-frame-large-map":
        maps, strides, in_hw, hw = [rng.integers(0, 256, (512, 512), dtype=np.uint8)], (8,), (4096, 4096), (600, 3)
    elif case == "downscale-of-large-maps":
        maps, strides, in_hw, hw = [rng.integers(0, 256, s, dtype=np.uint8) for s in ((300, 400), (150, 200))], (8, 16), (2400, 3200), (45, 60)
    else:
        mw = int(case[-4:])
        maps, strides, in_hw, hw = [rng.integers(0, 256, (80, mw), dtype=np.uint8)], (1,), (80, mw), (20, 2048)
    img = HR.frame(*hw, seed=3)
    want = HR.heatmap_ref(img, maps, strides, in_hw, lut="jet", alpha=150, alpha_mode="value")
    for inplace in (False, True):
        assert np.array_equal(guarded_draw(ore, img, maps, strides, in_hw, inplace=inplace, lut="jet", alpha=150, alpha_mode="value"), want)


def test_render_device_equals_host_and_bgr(ore):
    img, maps, strides, in_hw, style, want = HR.render_case((75, 100), 3)
    bgr = np.ascontiguousarray(img[:, :, ::-1])
    got = guarded_draw(ore, bgr, maps, strides, in_hw, channel_order="BGR", **style)
    assert np.array_equal(got[:, :, ::-1], want)
    assert np.array_equal(got, ore.heatmap_host(bgr, list(zip(maps, strides)), in_hw, channel_order="BGR", **style))
    fresh = ore.heatmap_draw(torch.from_numpy(np.array(img)).cuda(), dev_pairs(maps, strides), in_hw, **style)    # out=None: a new frame
    assert np.array_equal(fresh.cpu().numpy(), want)


def test_render_limits_are_errors(ore):
    img = torch.zeros(16, 16, 3, dtype=torch.uint8, device="cuda")
    m = torch.zeros(2, 2, dtype=torch.uint8, device="cuda")
    ore.heatmap_draw(img, [(m, 8)], (16, 16))
    for kw in (dict(alpha=256), dict(alpha=-1), dict(alpha_mode="x"), dict(lut="hot"), dict(lut=np.zeros((4, 3), np.uint8))):
        with pytest.raises(ore.OreError):
            ore.heatmap_draw(img, [(m, 8)], (16, 16), **kw)
    for levels, in_hw in (([], (16, 16)), ([(m, 8)] * 4, (16, 16)), ([(m, 0)], (16, 16)), ([(m, 129)], (16, 16)), ([(m, 8)], None),
                          ([(m, 8)], (0, 16)), ([(m, 8)], (16, 8193)), ([(m.cpu(), 8)], (16, 16)), ([(m.float(), 8)], (16, 16)),
                          ([(torch.zeros(2, 4, dtype=torch.uint8, device="cuda")[:, ::2], 8)], (16, 16))):
        with pytest.raises(ore.OreError):
            ore.heatmap_draw(img, levels, in_hw)
    for shape in ((1, 8193, 3), (8193, 1, 3)):
        with pytest.raises(ore.OreError, match="sides"):
            ore.heatmap_draw(torch.zeros(shape, dtype=torch.uint8, device="cuda"), [(m, 8)], (16, 16))
    buf = torch.zeros(16 * 16 * 3 + 8, dtype=torch.uint8, device="cuda")
    with pytest.raises(ore.OreError, match="aligned"):
        ore.heatmap_draw(buf[1:1 + 768].view(16, 16, 3), [(m, 8)], (16, 16))
    with pytest.raises(ore.OreError, match="overlap"):
        ore.heatmap_draw(buf[0:768].view(16, 16, 3), [(m, 8)], (16, 16), out=buf[4:772].view(16, 16, 3))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ quantise (stages A + B)
def device_source(ore_, vals, *, ld, coff, batch=1, slot=0, bf16=False, seed=0, **what):
    """A HeatSource over fresh device buffers [batch * h * w, ld] filled with noise, whose slot `slot` holds vals[l] at columns
    coff .. coff + ch; levels at strides 8 / 16 / 32."""
    rng = np.random.default_rng(seed)
    bufs, levels = [], []
    ch = vals[0].shape[2]
    for l, v in enumerate(vals):
        h, w = v.shape[:2]
        full = rng.normal(0, 3, (batch, h * w, ld)).astype(np.float32)
        full[slot, :, coff:coff + ch] = v.reshape(h * w, ch)
        t = torch.from_numpy(full.reshape(batch * h * w, ld)).cuda()
        bufs.append(t.to(torch.bfloat16) if bf16 else t)
        levels.append((h, w, 8 << l))
    return ore_.HeatSource(bufs, levels, ch=ch, coff=coff, batch=batch, slot=slot, in_hw=(40, 56), **what)


def check_levels(ore_, vals, ref=None, **kw):
    what = {k: kw[k] for k in ("channel", "transform", "norm") if k in kw}
    src = device_source(ore_, vals, **kw)
    got = ore_.heatmap_levels(src)
    want = (ref or HR.levels_ref)(vals, what.get("channel", "mean"), what.get("transform"), what.get("norm", "max"))
    assert len(got) == len(want) and got.strides == [8 << l for l in range(len(vals))] and got.in_hw == (40, 56)
    for l, (g, w_) in enumerate(zip(got, want)):
        g = g.cpu().numpy()
        assert g.dtype == np.uint8 and g.shape == w_.shape
        assert np.array_equal(g, w_), (l, int((g != w_).sum()))
    return want


def test_quantise_mean_in_the_p_layout(ore):
    """C = 128 mean, ld = 2F and coff = F (the p{l} layout), batch slot 1 of 2, norm "max": 0, 1, > 1, negatives, NaN, +-inf among
    the values (an infinite maximum: everything quantises to 0), then the same without the infinities."""
    vals = [HR.quantise_values(l + 1, hw, 128) for l, hw in enumerate(HR.LEVEL_HW)]
    check_levels(ore, vals, ld=256, coff=128, batch=2, slot=1, channel="mean", norm="max")
    vals = [np.nan_to_num(v, nan=np.nan, posinf=2.0, neginf=-2.0) for v in vals]
    want = check_levels(ore, vals, ld=256, coff=128, batch=2, slot=1, channel="mean", norm="max")
    assert max(int(w_.max()) for w_ in want) == 255
    check_levels(ore, vals, ld=256, coff=128, batch=2, slot=0, channel="mean", norm="unit", transform="sigmoid")


def test_quantise_channel_in_the_head_layout(ore):
    """One channel of rows [l, t, r, b, hm] at ld 8, through the sigmoid, norm "unit" (objectness) and raw with both norms; the
    special values sit in every channel."""
    vals = [HR.quantise_values(l + 11, hw, 5) * 6 for l, hw in enumerate(HR.LEVEL_HW)]
    check_levels(ore, vals, ld=8, coff=0, channel=4, transform="sigmoid", norm="unit")
    vals = [HR.quantise_values(l + 11, hw, 5) for l, hw in enumerate(HR.LEVEL_HW)]
    check_levels(ore, vals, ld=8, coff=0, channel=4, norm="unit")
    check_levels(ore, vals, ld=8, coff=0, batch=2, slot=1, channel=2, norm="max")
    check_levels(ore, vals[:1], ld=8, coff=3, channel=0, norm="max")


def test_quantise_bf16(ore):
    vals = [HR.bf16_round(HR.quantise_values(l + 21, hw, 128)) for l, hw in enumerate(HR.LEVEL_HW)]
    check_levels(ore, vals, ld=256, coff=128, bf16=True, channel="mean", norm="unit")
    vals = [np.nan_to_num(v, nan=np.nan, posinf=2.0, neginf=-2.0) for v in vals]
    check_levels(ore, vals, ld=256, coff=0, batch=2, slot=1, bf16=True, channel="mean", norm="max")
    check_levels(ore, vals, ld=128, coff=0, bf16=True, channel=17, norm="max")


def test_quantise_all_cold(ore):
    """norm "max" with every value <= 0 (or NaN): m == 0, every q is 0."""
    vals = [-np.abs(HR.quantise_values(l + 31, hw, 8, special=False)) for l, hw in enumerate(HR.LEVEL_HW)]
    vals[0][0, 0], vals[1][0, 0], vals[2][0, 0] = 0.0, -0.0, np.nan
    want = check_levels(ore, vals, ld=8, coff=0, channel="mean", norm="max")
    assert not any(w_.any() for w_ in want)
    check_levels(ore, vals, ld=8, coff=0, channel=3, norm="max")


def test_quantise_many_blocks(ore):
    """More than one block (the maximum crosses blocks), and more than the 256 blocks the first kernel is capped at (its grid-stride
    loop).  The large case's reference is heatmap_levels_host, which test_heatmap_host pins to the per-location reference."""
    vals = [HR.quantise_values(41 + l, hw, 32, special=False) for l, hw in enumerate(((40, 54), (20, 27), (10, 14)))]
    vals[2][9, 13] = 3.5                                       # the maximum sits in the last block
    want = check_levels(ore, vals, ld=32, coff=0, channel="mean", norm="max")
    assert want[2][9, 13] == 255
    host = lambda v, c, t, n: ore.heatmap_levels_host(v, channel=c, transform=t, norm=n)
    big = [HR.quantise_values(51, (260, 261), 4, special=False)]
    assert 260 * 261 > 256 * 256
    big[0][259, 260, 1] = 4.25
    want = check_levels(ore, big, ref=host, ld=4, coff=0, channel=1, norm="max")
    assert want[0][259, 260] == 255 and 0 < want[0].mean() < 255
    check_levels(ore, big, ref=host, ld=4, coff=0, channel="mean", transform="sigmoid", norm="unit")


def test_sigmoid_straddles(ore):
    """For k = 1 .. 255 the fp32 logit of k / 255 and its +-1, +-2 ulp neighbours: the device q is the reference q."""
    x = HR.straddle_logits()
    vals = [np.zeros((1, len(x), 5), np.float32)]
    vals[0][0, :, 4] = x
    got = ore.heatmap_levels(device_source(ore, vals, ld=8, coff=0, channel=4, transform="sigmoid", norm="unit"))[0].cpu().numpy().reshape(-1)
    want = np.array([HR.quantise(s) for s in ore.sigmoid_host(x)], dtype=np.uint8)
    bad = np.nonzero(got != want)[0]
    print(f"{len(x)} logits, {len(bad)} differ", [(float(x[i]), int(got[i]), int(want[i])) for i in bad[:5]])
    assert np.array_equal(got, want)


def test_quantise_refusals(ore):
    vals = [np.zeros((2, 2, 6), np.float32)]
    with pytest.raises(ore.OreError, match="multiple"):        # a channel count that is no multiple of 4 has no mean
        device_source(ore, vals, ld=8, coff=0, channel="mean")
    t = torch.zeros(4, 8, device="cuda")
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    L = ore.lib()
    args = lambda **k: [k.get(a, d) for a, d in (("n", 1), ("s0", t.data_ptr()), ("s1", None), ("s2", None), ("hw", ore._i32s([2, 2])),
                                                   ("ld", ore._i32s([8])), ("coff", ore._i32s([0])), ("ch", 6), ("bf16", 0), ("batch", 1),
                                                   ("slot", 0), ("channel", 0), ("transform", 0), ("norm", 0), ("ws", ws.data_ptr()),
                                                   ("ws_bytes", ws.numel()), ("stream", None))]
    assert L.ore_heatmap_levels_fwd(*args()) == 0
    for bad in (dict(channel=-1), dict(channel=6), dict(slot=1), dict(batch=0), dict(transform=2), dict(norm=2), dict(n=0), dict(n=4),
                dict(s0=None), dict(ch=9), dict(hw=ore._i32s([2, 4097])), dict(channel=-1, ch=8, ld=ore._i32s([10])), dict(ws_bytes=16)):
        assert L.ore_heatmap_levels_fwd(*args(**bad)) != 0, bad
    for kw in (dict(channel=5), dict(channel=-1), dict(transform="tanh"), dict(norm="minmax")):
        with pytest.raises(ore.OreError):
            device_source(ore, [np.zeros((2, 2, 5), np.float32)], **{"ld": 8, "coff": 0, **kw})
    with pytest.raises(ore.OreError, match="slot"):
        ore.HeatSource([t], [(2, 2, 8)], ch=5, channel=0, in_hw=(16, 16), slot=1)
    with pytest.raises(ore.OreError, match="do not fit"):
        ore.HeatSource([t], [(2, 2, 8)], ch=5, coff=4, channel=0, in_hw=(16, 16))
    for bad in ([t[:, :4]], [t.double()], [t.cpu()], [t[:3]], [t, t]):
        with pytest.raises(ore.OreError):
            ore.HeatSource(bad, [(2, 2, 8)], ch=4, channel=0, in_hw=(16, 16))
    with pytest.raises(ore.OreError):
        ore.heatmap_levels([(torch.zeros(2, 2, dtype=torch.uint8, device="cuda"), 8)])
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ end to end
def host_heat(ore_, engine, kind, bgr, slot=0, **style):
    """The host composition of a heat map: the kind's buffers copied out of the engine after the pass, then heatmap_ref's stages."""
    what = ore_.heat_kind(kind)
    geo = engine.last_geometry()
    vals, strides = [], []
    for name in what["buffers"]:
        h, w, s = geo["levels"][int(name[-1]) - 3]
        t = engine.buffer(name).float().cpu().numpy()
        vals.append(np.ascontiguousarray(t.reshape(geo["B"], h, w, -1)[slot]))
        strides.append(s)
    maps = HR.levels_ref(vals, what["channel"], what["transform"], what["norm"])
    assert max(int(m.max()) for m in maps) > 0, "an empty heat map checks nothing"
    return HR.heatmap_ref(bgr, maps, strides, (geo["H"], geo["W"]), channel_order="BGR", **style)


def boxes_on(ore_, picture, out, color_by, names):
    from detectron2.utils.visualizer import default_overlay_params
    i = out["instances"]
    return OR.overlay_ref(picture, i.pred_boxes.tensor.cpu().numpy(), i.scores.cpu().numpy(), i.pred_classes.cpu().numpy(),
                          atlas=ore_.overlay_atlas(), palette=ore_.OVERLAY_PALETTE[:, ::-1], color_by=color_by, names=names,
                          **default_overlay_params(*picture.shape[:2]))


@pytest.fixture(scope="module")
def pred(ore):
    from detectron2.engine.defaults import DefaultPredictor
    p = DefaultPredictor(_cfg())
    _load(p.model)
    return p


@pytest.mark.parametrize("heatmap", ["objectness", "attention", "p4:3", {"kind": "pos3", "lut": "gray", "alpha": 178, "alpha_mode": "value"}],
                         ids=["objectness", "attention", "p4:3", "pos3-gray-value"])
def test_visualization_demo_heatmap(ore, pred, heatmap):
    """VisualizationDemo(cfg, heatmap=kind).run_on_image == the host composition: the buffers copied out after the same pass ->
    heatmap_ref -> overlay_ref; the predictions are DefaultPredictor's."""
    from detectron2.utils.visualizer import thing_classes
    from predictor import VisualizationDemo
    demo = VisualizationDemo(_cfg(), heatmap=heatmap)
    _load(demo.predictor.model)
    kind = heatmap if isinstance(heatmap, str) else heatmap["kind"]
    style = {} if isinstance(heatmap, str) else {k: v for k, v in heatmap.items() if k != "kind"}
    bgr = raw_image(47, *RAW_SIZES[1])
    got, vis = demo.run_on_image(bgr)
    assert_same(got, pred(bgr))
    heat = host_heat(ore, demo.predictor.model._engine, kind, bgr, **style)
    want = boxes_on(ore, heat, got, "instance", thing_classes(demo.metadata))
    print(f"{kind}: {int((heat != bgr).any(2).sum())} pixels changed by the heat map, {int((want != heat).any(2).sum())} by the boxes")
    assert (heat != bgr).any() and (want != heat).any()
    assert np.array_equal(vis.get_image(), want[:, :, ::-1])


def test_heatmap_none_draws_todays_picture(ore, pred):
    from detectron2.utils.visualizer import thing_classes
    from predictor import VisualizationDemo
    demo = VisualizationDemo(_cfg(), heatmap=None)
    _load(demo.predictor.model)
    bgr = raw_image(48, *RAW_SIZES[0])
    got, vis = demo.run_on_image(bgr)
    assert_same(got, pred(bgr))
    assert np.array_equal(vis.get_image(), boxes_on(ore, bgr, got, "instance", thing_classes(demo.metadata))[:, :, ::-1])


def test_parallel_demo_draws_the_same_bytes(ore, pred):
    """6 frames of two sizes through run_on_video, serial and with 4 passes in flight: the same annotated frames, each the host
    composition's heat map under the boxes; put(heatmap=...) alone gives the heat map without boxes and leaves a device frame alone."""
    from detectron2.utils.visualizer import thing_classes
    from predictor import VisualizationDemo
    frames = [raw_image(130 + i, *RAW_SIZES[i % 2]) for i in range(6)]
    serial = VisualizationDemo(_cfg(), parallel=False, heatmap="objectness")
    _load(serial.predictor.model)
    par = VisualizationDemo(_cfg(), parallel=True, heatmap="objectness")
    _load(par.predictor.model)
    names = thing_classes(serial.metadata)
    try:
        assert par.predictor.inflight == 4
        a = list(serial.run_on_video(frames))
        b = list(par.run_on_video(iter(frames)))
        got, vis = par.run_on_image(frames[1])
        dev = torch.from_numpy(frames[0]).cuda()
        par.predictor.put(dev, heatmap={"kind": "attention", "alpha": 200})
        only = par.predictor.get()
        heat_only = host_heat(ore, par.predictor._slots[(par.predictor._next - 1) % 4].engine, "attention", frames[0], alpha=200)
    finally:
        par.predictor.shutdown()
    assert len(a) == len(b) == 6
    for i, f in enumerate(frames):
        assert np.array_equal(a[i], b[i]), i
    # the serial demo's last pass is frame 5's: its engine still holds that pass
    heat = host_heat(ore, serial.predictor.model._engine, "objectness", frames[5])
    assert np.array_equal(a[5], boxes_on(ore, heat, pred(frames[5]), "class", names))
    assert_same(got, pred(frames[1]))
    _, picture = serial.run_on_image(frames[1])
    assert np.array_equal(vis.get_image(), picture.get_image())
    assert np.array_equal(only["vis_image"].cpu().numpy(), heat_only) and np.array_equal(dev.cpu().numpy(), frames[0])
    assert_same(only, pred(frames[0]))


def test_async_heatmap_path_issues_no_sync_and_refuses_early(ore, pred):
    """put(..., draw=True, heatmap=...) enqueues without a host synchronisation torch knows of; bad heat-map arguments are refused
    with the engine idle."""
    from predictor import AsyncPredictor
    ap = AsyncPredictor(_cfg(), inflight=2)
    _load(ap.model)
    frames = [raw_image(140 + i, *RAW_SIZES[0]) for i in range(2)]
    try:
        for bad in ("heat", {"kind": "p4:128"}, {"kind": "head3:5"}, {"kind": "p4", "slot": 1}, {"kind": "p4", "alpha": 300}, {"alpha": 3}):
            with pytest.raises(ValueError):
                ap.put(frames[0], heatmap=bad)
            assert len(ap) == 0
        for f in frames:                                       # engines, graphs, tables, workspaces: built outside the measured calls
            ap.put(f, draw=True, heatmap="attention")
        warm = [ap.get() for _ in frames]
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            for f in frames:
                ap.put(f, draw=True, heatmap="attention")
        finally:
            torch.cuda.set_sync_debug_mode("default")
        for f, w_ in zip(frames, warm):
            g = ap.get()
            assert_same(g, pred(f))
            assert torch.equal(g["vis_image"], w_["vis_image"])
    finally:
        ap.shutdown()


def test_stale_source_raises(ore, pred):
    bgr = raw_image(49, *RAW_SIZES[1])
    frame = torch.from_numpy(bgr).cuda()
    pred(bgr)
    e = pred.model._engine
    src = e.heat_source("objectness")
    levels = ore.heatmap_levels(src)
    first = ore.heatmap_draw(frame, levels)
    assert np.array_equal(first.cpu().numpy(), ore.heatmap_draw(frame, src).cpu().numpy())
    pred(bgr)                                                  # a newer pass of the same engine
    assert pred.model._engine is e and e.last_geometry()["serial"] == src.serial + 1
    for stale in (src, levels):
        with pytest.raises(ore.OreError, match="stale"):
            ore.heatmap_draw(frame, stale)
    with pytest.raises(ore.OreError, match="stale"):
        ore.heatmap_levels(src)
    again = ore.heatmap_draw(frame, e.heat_source("objectness"))
    assert np.array_equal(again.cpu().numpy(), first.cpu().numpy())
    for bad in ("objectness:1", "p6", "stem1"):
        with pytest.raises(ore.OreError):
            e.heat_source(bad)
    with pytest.raises(ore.OreError, match="slot"):
        e.heat_source("objectness", slot=1)
    with pytest.raises(ore.OreError, match="channel"):
        e.heat_source("p4:128")


def test_nway_slot_draws_that_class(ore):
    """An N-way pass over two classes: slot k draws class k's map -- the host composition of block k of the level buffers -- through
    the demo (objectness) and through heat_source (attention).  The synthetic head's logits differ by 1e-4 between the two classes,
    less than a quantisation step, so it is the attention pictures -- the correlation with each class's own prototypes -- that are
    required to differ."""
    from predictor import VisualizationDemo
    bgr = raw_image(52, *RAW_SIZES[1])
    frame = torch.from_numpy(bgr).cuda()
    pictures = []
    for slot in (0, 1):
        demo = VisualizationDemo(_cfg(), heatmap={"kind": "objectness", "slot": slot})
        m = _load(demo.predictor.model)
        m.set_support_dict(_support_dict((3, 8)))
        m.support_classes = "all"
        got, vis = demo.run_on_image(bgr)
        e = m.engine()
        assert e.last_geometry()["B"] == 2 and set(got["instances"].pred_classes.tolist()) <= {3, 8}
        heat = host_heat(ore, e, "objectness", bgr, slot=slot)
        assert np.array_equal(vis.get_image(), boxes_on(ore, heat, got, "instance", getattr(demo.metadata, "thing_classes", None))[:, :, ::-1])
        attn = ore.heatmap_draw(frame, e.heat_source("attention", slot=slot), channel_order="BGR").cpu().numpy()
        assert np.array_equal(attn, host_heat(ore, e, "attention", bgr, slot=slot))
        pictures.append(attn)
        with pytest.raises(ore.OreError, match="slot"):
            e.heat_source("objectness", slot=2)
    assert (pictures[0] != pictures[1]).any()


def test_nway_every_buffer_kind_is_per_slot(ore):
    """After an N-way pass every admitted level buffer -- p, attn, pos, tower, head -- is a batch of K class slots: slot 1's picture is
    the host composition of block 1, and its quantised map is, to one step, the map of a one-class engine built with class 1's
    supports alone (the N-way pass pins those buffers to 1e-5 of the one-class pass: tests/test_hip_nway.py; 1e-5 of the maximum is
    far below a 1 / 255 step, so only a value on a step's edge may move, by one).  A buffer in another layout would give neither."""
    from detectron2.engine.defaults import DefaultPredictor
    bgr = raw_image(53, *RAW_SIZES[1])
    frame = torch.from_numpy(bgr).cuda()
    both, one = DefaultPredictor(_cfg()), DefaultPredictor(_cfg())
    two = _support_dict((3, 8))
    _load(both.model).set_support_dict(two)
    both.model.support_classes = "all"
    _load(one.model).set_support_dict({k: {8: v[8]} for k, v in two.items()})
    both(bgr)
    one(bgr)
    eK, e1 = both.model.engine(), one.model.engine()
    assert eK.last_geometry()["B"] == 2 and e1.last_geometry()["B"] == 1
    for kind in ("p4", "attn4", "pos4", "tower4", "head4:0", "p3:5", "attn5", "pos3", "tower5:0"):
        got = ore.heatmap_draw(frame, eK.heat_source(kind, slot=1), channel_order="BGR").cpu().numpy()
        assert np.array_equal(got, host_heat(ore, eK, kind, bgr, slot=1)), kind
        qK = ore.heatmap_levels(eK.heat_source(kind, slot=1))[0].cpu().numpy().astype(np.int32)
        q1 = ore.heatmap_levels(e1.heat_source(kind))[0].cpu().numpy().astype(np.int32)
        print(f"{kind}: {int((qK != q1).sum())} of {qK.size} locations differ from the one-class pass, by at most {int(np.abs(qK - q1).max())}")
        assert qK.shape == q1.shape and int(np.abs(qK - q1).max()) <= 1 and qK.max() == 255, kind
    for bad in ("lat3", "lat4:1"):
        with pytest.raises(ore.OreError):
            eK.heat_source(bad)


def test_visualizer_draws_device_sources(ore, pred):
    """Visualizer.draw_heatmap with a HeatSource, a HeatLevels and device maps, then draw_instance_predictions: the host composition's
    heat map with the boxes on top; VideoVisualizer.draw_heatmap likewise."""
    from detectron2.utils.video_visualizer import VideoVisualizer
    from detectron2.utils.visualizer import Visualizer
    bgr = raw_image(54, *RAW_SIZES[0])
    out = pred(bgr)
    e = pred.model.engine()
    heat = host_heat(ore, e, "attention", bgr, alpha=100)
    want = boxes_on(ore, heat, out, "instance", None)
    src = e.heat_source("attention")
    levels = ore.heatmap_levels(src)
    pairs = [(m.clone(), s) for m, s in zip(levels.maps, levels.strides)]
    for source, kw in ((src, {}), (levels, {}), (pairs, {"in_hw": levels.in_hw})):
        vis = Visualizer(bgr, None, channel_order="BGR")
        drawn = vis.draw_heatmap(source, alpha=100, **kw)
        assert torch.is_tensor(drawn.img) and drawn.img.is_cuda and np.array_equal(drawn.img.cpu().numpy(), heat)
        boxed = vis.draw_instance_predictions(out["instances"])
        assert np.array_equal(boxed.img.cpu().numpy(), want) and (want != heat).any()
    got = VideoVisualizer(None, channel_order="BGR").draw_heatmap(torch.from_numpy(bgr).cuda(), src, alpha=100)
    assert np.array_equal(got.img.cpu().numpy(), heat) and np.array_equal(got.get_image(), heat[:, :, ::-1])


def test_demo_without_a_pass_is_refused(ore):
    """VisualizationDemo's heat map needs the pass it draws: an engine that has not run one is a ValueError, not a picture."""
    from predictor import VisualizationDemo
    demo = VisualizationDemo(_cfg(), heatmap="objectness")
    _load(demo.predictor.model)
    with pytest.raises(ValueError, match="pass"):
        demo._heat(torch.zeros(32, 32, 3, dtype=torch.uint8, device="cuda"))
