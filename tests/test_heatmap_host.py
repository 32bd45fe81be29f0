"""CPU: the heat-map render contract ("heatmap v1", include/ore_hip.h) as orehip.heatmap_host / heatmap_levels_host state it, against
the independent restatement tests/heatmap_ref.py on the cases the device test draws; the sigmoid's host twin against the oracle; the
colour tables; the argument refusals of the package and of the demo names built on it."""
import numpy as np
import pytest
import torch

import heatmap_ref as HR


@pytest.fixture(scope="module")
def ore():
    import orehip
    return orehip


def pairs(maps, strides):
    return list(zip(maps, strides))


@pytest.mark.parametrize("hw", HR.FRAMES, ids=lambda v: "%dx%d" % v)
def test_host_equals_ref(ore, hw):
    """Three levels onto every frame size of the device test, default style; the small ones in every style, with one level only and
    with an input size that is no multiple of the strides."""
    img, maps, strides, in_hw, style, want = HR.render_case(hw)
    got = ore.heatmap_host(img, pairs(maps, strides), in_hw, **style)
    assert got.dtype == np.uint8 and got.shape == img.shape
    assert np.array_equal(got, want), int((got != want).sum())
    if hw != (1, 1):
        assert (got != img).any()
    if hw[0] * hw[1] > 10000:
        return
    for si in range(1, len(HR.STYLES)):
        img, maps, strides, in_hw, style, want = HR.render_case(hw, si)
        assert np.array_equal(ore.heatmap_host(img, pairs(maps, strides), in_hw, **style), want), si
    for n_levels, in_hw in ((1, HR.IN_HW), (3, (43, 61)), (2, (43, 61))):
        img, maps, strides, in_hw, style, want = HR.render_case(hw, 0, n_levels, in_hw)
        assert np.array_equal(ore.heatmap_host(img, pairs(maps, strides), in_hw, **style), want), (n_levels, in_hw)


def test_host_in_place_and_bgr(ore):
    img, maps, strides, in_hw, style, want = HR.render_case((37, 53), 3)
    buf = np.array(img)
    assert ore.heatmap_host(buf, pairs(maps, strides), in_hw, out=buf, **style) is buf and np.array_equal(buf, want)
    out = np.zeros_like(img)
    assert ore.heatmap_host(img, pairs(maps, strides), in_hw, out=out, **style) is out and np.array_equal(out, want)
    # a BGR frame with the table reversed is the RGB picture with its channels reversed
    bgr = np.ascontiguousarray(img[:, :, ::-1])
    got = ore.heatmap_host(bgr, pairs(maps, strides), in_hw, channel_order="BGR", **style)
    assert np.array_equal(got[:, :, ::-1], want)
    assert np.array_equal(got, HR.heatmap_ref(bgr, maps, strides, in_hw, channel_order="BGR", **style))
    # CPU tensors are taken too
    got = ore.heatmap_host(torch.from_numpy(np.array(img)), [(torch.from_numpy(np.array(m)), s) for m, s in zip(maps, strides)], in_hw, **style)
    assert np.array_equal(got, want)


def test_sigmoid_host_equals_the_oracle(ore):
    """ore_sigmoid_host == oracle.decode.sigmoid bit for bit: random logits, the straddle set, the ends of the range."""
    from oracle import decode as odec
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.normal(0, 6, 200000), rng.uniform(-100, 100, 50000)]).astype(np.float32)
    x = np.concatenate([x, HR.straddle_logits(), np.array([0.0, -0.0, 88.0, 88.5, -87.0, -87.5, 1e-30, -1e-30, np.inf, -np.inf], np.float32)])
    got, want = ore.sigmoid_host(x), odec.sigmoid(x)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert ore.sigmoid_host(np.zeros((2, 3), np.float32)).shape == (2, 3)
    assert np.isnan(ore.sigmoid_host(np.array([np.nan, -np.nan], np.float32))).all()            # a NaN returns early: no conversion of it


def test_straddles_cross_quantisation_steps(ore):
    """The straddle set does what it is for: around every k the quantised sigmoid takes the values on both sides of a step."""
    x = HR.straddle_logits()
    q = ore.heatmap_levels_host([x.reshape(1, -1, 1)], channel=0, transform="sigmoid", norm="unit")[0].reshape(-1)
    want = np.array([HR.quantise(s) for s in ore.sigmoid_host(x)], dtype=np.uint8)
    assert np.array_equal(q, want)
    steps = sum(len(set(q[5 * i:5 * i + 5].tolist())) > 1 for i in range(254))
    print(f"{steps} of 254 five-point neighbourhoods straddle a step; q spans {q.min()} .. {q.max()}")
    # sigmoid(logit(k / 255)) is k / 255 to a few ulp, so a neighbourhood quantises to k - 1 or k, and some take both
    assert all(set(q[5 * i:5 * i + 5].tolist()) <= {i, i + 1} for i in range(254)) and steps >= 1 and q.max() == 255


@pytest.mark.parametrize("channel,transform,norm", [("mean", None, "max"), (4, "sigmoid", "unit"), (3, None, "max"), ("mean", "sigmoid", "unit"),
                                                    (0, None, "unit"), ("mean", "sigmoid", "max")])
def test_levels_host_equals_ref(ore, channel, transform, norm):
    """Stages A + B: 0, 1, > 1, negatives, NaN, both infinities among the values; 128 channels for the mean, 8 otherwise."""
    ch = 128 if channel == "mean" else 8
    vals = [HR.quantise_values(l + 1, hw, ch) for l, hw in enumerate(HR.LEVEL_HW)]
    got = ore.heatmap_levels_host(vals, channel=channel, transform=transform, norm=norm)
    want = HR.levels_ref(vals, channel, transform, norm)
    for g, w_ in zip(got, want):
        assert g.dtype == np.uint8 and np.array_equal(g, w_), (g, w_)
    # without the infinities the maximum is finite and the maps are not empty
    vals = [np.nan_to_num(v, nan=np.nan, posinf=2.0, neginf=-2.0) for v in vals]
    got = ore.heatmap_levels_host(vals, channel=channel, transform=transform, norm=norm)
    want = HR.levels_ref(vals, channel, transform, norm)
    assert all(np.array_equal(g, w_) for g, w_ in zip(got, want)) and max(int(g.max()) for g in got) > 0


def test_levels_host_special_values(ore):
    v = np.array([0.0, 1.0, 1.5, -0.25, np.nan, np.inf, -np.inf, -0.0, 0.5, 0.999999], np.float32).reshape(1, -1, 1)
    assert ore.heatmap_levels_host([v], channel=0, norm="unit")[0].reshape(-1).tolist() == [0, 255, 255, 0, 0, 255, 0, 0, 127, 254]
    # an infinite maximum empties everything finite; inf / inf is NaN -> 0
    assert not ore.heatmap_levels_host([v], channel=0, norm="max")[0].any()
    # all values <= 0 (or NaN): m == 0, every q is 0
    neg = np.array([-1.0, -0.0, 0.0, np.nan, -np.inf], np.float32).reshape(1, -1, 1)
    assert not ore.heatmap_levels_host([neg], channel=0, norm="max")[0].any()
    assert [int(q.max()) for q in HR.levels_ref([neg], 0, None, "max")] == [0]
    fin = np.array([0.5, 2.0, 1.0, -3.0], np.float32).reshape(2, 2, 1)
    assert ore.heatmap_levels_host([fin], channel=0, norm="max")[0].tolist() == [[63, 255], [127, 0]]


def test_constant_map_blends_one_colour(ore):
    """A constant map of value q gives every pixel blend(LUT[q]); alpha 0 returns the frame; alpha 255 "constant" returns LUT[v]."""
    img = HR.frame(23, 31, 4)
    for q in (0, 1, 77, 254, 255):
        maps = [np.full(hw, q, np.uint8) for hw in HR.LEVEL_HW]
        for lut in ("jet", "gray", HR.RANDOM_LUT):
            tab = ore.heatmap_lut(lut).astype(np.int64)
            got = ore.heatmap_host(img, pairs(maps, HR.STRIDES), HR.IN_HW, lut=lut, alpha=100)
            assert np.array_equal(got, (img.astype(np.int64) * 155 + tab[q] * 100 + 127) // 255)
            got = ore.heatmap_host(img, pairs(maps, HR.STRIDES), HR.IN_HW, lut=lut, alpha=100, alpha_mode="value")
            A = (100 * q + 127) // 255
            assert np.array_equal(got, (img.astype(np.int64) * (255 - A) + tab[q] * A + 127) // 255)
    img, maps, strides, in_hw, _, _ = HR.render_case((37, 53))
    for mode in ("constant", "value"):
        assert np.array_equal(ore.heatmap_host(img, pairs(maps, strides), in_hw, alpha=0, alpha_mode=mode), img)
    got = ore.heatmap_host(img, pairs(maps, strides), in_hw, alpha=255, lut=HR.RANDOM_LUT)
    assert np.array_equal(got, HR.RANDOM_LUT[HR.merged_ref(37, 53, maps, strides, in_hw)])
    # "value": where the merged map is 0 the frame is untouched
    cold = [np.zeros(hw, np.uint8) for hw in HR.LEVEL_HW]
    assert np.array_equal(ore.heatmap_host(img, pairs(cold, strides), in_hw, alpha=255, alpha_mode="value"), img)


def test_cells_sit_at_the_centernet_locations(ore):
    """Cell (i, j) sits at input coordinate (j s + s / 2, i s + s / 2), the boundary between pixels j s + s / 2 - 1 and j s + s / 2 of
    a frame of the input's size: a single hot cell draws a profile that is symmetric about that boundary and highest on either side."""
    for j in range(1, 6):
        row = np.zeros((1, 7), np.uint8)
        row[0, j] = 255
        v = HR.merged_ref(8, 56, [row], (8,), (8, 56))
        assert (v == v[0]).all()                               # one map row: every frame row alike
        v = v[0]
        c = 8 * j + 4
        assert np.array_equal(v[c - 12:c], v[c:c + 12][::-1]) and v[c] == v.max() == (255 * 240 * 256 + 32768) >> 16
        got = ore.heatmap_host(np.zeros((8, 56, 3), np.uint8), [(row, 8)], (8, 56), lut="gray", alpha=255)
        assert np.array_equal(got[0, :, 0], v)


def test_lut_anchors(ore):
    jet, gray = ore.heatmap_lut("jet"), ore.heatmap_lut("gray")
    assert jet.shape == (256, 3) and jet.dtype == np.uint8
    assert tuple(jet[0]) == (0, 0, 128) and tuple(jet[255]) == (128, 0, 0)
    assert np.array_equal(jet, HR.jet_table()) and np.array_equal(gray, HR.gray_table())
    assert tuple(gray[0]) == (0, 0, 0) and tuple(gray[200]) == (200, 200, 200)
    for lut in ("jet", "gray", HR.RANDOM_LUT):
        assert np.array_equal(ore.heatmap_lut(lut, "BGR"), ore.heatmap_lut(lut)[:, ::-1])
    assert np.array_equal(ore.heatmap_lut(HR.RANDOM_LUT), HR.RANDOM_LUT)
    assert np.array_equal(ore.heatmap_lut(torch.from_numpy(np.array(HR.RANDOM_LUT))), HR.RANDOM_LUT)
    assert ore.heatmap_lut() is not None and np.array_equal(ore.heatmap_lut(), jet)                 # the default is jet


def test_heat_kinds(ore):
    assert ore.heat_kind("objectness") == {"buffers": ("head3", "head4", "head5"), "channel": 4, "transform": "sigmoid", "norm": "unit"}
    assert ore.heat_kind("attention") == {"buffers": ("attn3", "attn4", "attn5"), "channel": "mean", "transform": None, "norm": "max"}
    assert ore.heat_kind("p4") == {"buffers": ("p4",), "channel": "mean", "transform": None, "norm": "max"}
    assert ore.heat_kind("pos3:17") == {"buffers": ("pos3",), "channel": 17, "transform": None, "norm": "max"}
    for bad in ("p6", "p4:", "p4:-1", "stem1", "lat4", "lat3:1", "head3", "attention:3", "", "P4", None, 4):
        with pytest.raises(ore.OreError):
            ore.heat_kind(bad)


def test_refusals(ore):
    img, maps, strides, in_hw, _, _ = HR.render_case((37, 53))
    ok = pairs(maps, strides)
    for kw in (dict(alpha=256), dict(alpha=-1), dict(alpha=0.5), dict(alpha=True), dict(alpha_mode="linear"), dict(lut="hot"),
               dict(lut=np.zeros((255, 3), np.uint8)), dict(lut=np.zeros((256, 3), np.int32)), dict(channel_order="GBR")):
        with pytest.raises(ore.OreError):
            ore.heatmap_host(img, ok, in_hw, **kw)
    for levels, hw_in in (([], in_hw), (ok + ok[:1], in_hw), ([(maps[0], 0)], in_hw), ([(maps[0], 129)], in_hw), (ok, None), (ok, (0, 56)),
                          (ok, (40, 8193)), ([maps[0]], in_hw), ([(maps[0].reshape(-1), 8)], in_hw), ([(np.zeros((4097, 1), np.uint8), 8)], in_hw)):
        with pytest.raises(ore.OreError):
            ore.heatmap_host(img, levels, hw_in)
    with pytest.raises(ore.OreError):
        ore.heatmap_host(img, [(maps[0].astype(np.int32), 8)], in_hw)
    with pytest.raises(ore.OreError):
        ore.heatmap_host(img[:, :, :2], ok, in_hw)
    with pytest.raises(ore.OreError, match="multiple of 4"):
        ore.heatmap_levels_host([np.zeros((2, 2, 6), np.float32)], channel="mean")
    for kw in (dict(channel=8), dict(channel=-1), dict(channel="sum"), dict(transform="tanh"), dict(norm="minmax")):
        with pytest.raises(ore.OreError):
            ore.heatmap_levels_host([np.zeros((2, 2, 8), np.float32)], **kw)
    # the library's own checks, reached without a device: no workspace for sizes out of range
    assert int(ore.lib().ore_heatmap_workspace_bytes(1, ore._i32s([4097, 1]))) == 0
    assert int(ore.lib().ore_heatmap_workspace_bytes(4, ore._i32s([1] * 8))) == 0
    assert int(ore.lib().ore_heatmap_workspace_bytes(3, ore._i32s([5, 7, 3, 4, 2, 2]))) >= 35 + 12 + 4
    with pytest.raises(ore.OreError):
        ore.heatmap_draw(torch.zeros(4, 4, 3, dtype=torch.uint8), ok, in_hw)                       # a host frame is not drawn on the device


def test_demo_names_refuse_bad_heatmaps():
    """heatmap= of VisualizationDemo / AsyncPredictor.put and demo.py's flags: checked on the host, before any engine exists."""
    import demo
    from predictor import heatmap_args
    assert heatmap_args(None) is None
    assert heatmap_args("objectness") == {"kind": "objectness", "slot": 0, "lut": "jet", "alpha": 128, "alpha_mode": "constant"}
    kw = heatmap_args({"kind": "pos3:17", "alpha": 178, "lut": "gray", "alpha_mode": "value", "slot": 1})
    assert (kw["kind"], kw["alpha"], kw["lut"], kw["alpha_mode"], kw["slot"]) == ("pos3:17", 178, "gray", "value", 1)
    assert np.array_equal(heatmap_args({"kind": "p4", "lut": HR.RANDOM_LUT})["lut"], HR.RANDOM_LUT)
    for bad in ("heat", "head4", {"alpha": 3}, {"kind": "p4", "colour": 1}, {"kind": "p4", "alpha": 256}, {"kind": "p4", "alpha_mode": "x"},
                {"kind": "p4", "lut": "hot"}, {"kind": "p4", "lut": np.zeros((3, 3), np.uint8)}, {"kind": "p4", "slot": -1},
                {"kind": "p4", "slot": 0.5}, 5, True):
        with pytest.raises(ValueError):
            heatmap_args(bad)
    args = demo.get_parser().parse_args(["--input", "a.jpg", "--output", "o", "--heatmap", "attention", "--heatmap-alpha", "99",
                                         "--heatmap-colormap", "gray"])
    assert (args.heatmap, args.heatmap_alpha, args.heatmap_colormap) == ("attention", 99, "gray")
    none = demo.get_parser().parse_args(["--input", "a.jpg", "--output", "o"])
    assert none.heatmap is None and none.heatmap_alpha == 128 and none.heatmap_colormap == "jet"
    with pytest.raises(SystemExit):
        demo.get_parser().parse_args(["--heatmap-colormap", "hot"])


def test_visualizer_draws_host_maps(ore):
    """Visualizer.draw_heatmap / VideoVisualizer.draw_heatmap on host maps: heatmap_host's bytes; the Visualizer then draws boxes on
    top of the heat map."""
    from detectron2.structures import Boxes, Instances
    from detectron2.utils.video_visualizer import VideoVisualizer
    from detectron2.utils.visualizer import Visualizer, default_overlay_params
    img, maps, strides, in_hw, style, want = HR.render_case((75, 100), 1)
    vis = Visualizer(img)
    out = vis.draw_heatmap(pairs(maps, strides), in_hw=in_hw, **style)
    assert np.array_equal(out.get_image(), want) and np.array_equal(vis.get_output().img, want)
    inst = Instances((75, 100))
    inst.pred_boxes = Boxes(torch.tensor([[10.0, 12.0, 60.0, 50.0]]))
    inst.scores = torch.tensor([0.5])
    boxed = vis.draw_instance_predictions(inst).get_image()
    direct = ore.overlay_host(want, inst.pred_boxes.tensor, inst.scores, None, palette=ore.OVERLAY_PALETTE, **default_overlay_params(75, 100))
    assert np.array_equal(boxed, direct) and (boxed != want).any()
    bgr = np.ascontiguousarray(img[:, :, ::-1])
    got = VideoVisualizer(None, channel_order="BGR").draw_heatmap(bgr, pairs(maps, strides), in_hw=in_hw, **style)
    assert np.array_equal(got.img[:, :, ::-1], want) and np.array_equal(got.get_image(), want)
    with pytest.raises(ValueError):
        vis.draw_heatmap(pairs(maps, strides), in_hw=in_hw, colour="red")
