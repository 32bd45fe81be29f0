"""CPU: the detection overlay's render contract ("overlay v1", include/ore_hip.h) as orehip.overlay_host states it, against the
independent restatement tests/overlay_ref.py and a hand-derived fixture; the detectron2 demo names built on it."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import PKG
import overlay_ref as OR

NAMES = ["stone", "a-rather-long-class-name-of-32-b", "cat", "x", "dog"]


@pytest.fixture(scope="module")
def ore():
    import orehip
    return orehip


def frame(h, w, seed=0):
    return np.random.default_rng(seed * 7919 + h * 10007 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)


def both(ore, img, b, s, c, n=None, **kw):
    kw.setdefault("palette", ore.OVERLAY_PALETTE)
    got = ore.overlay_host(img, b, s, c, n, **kw)
    want = OR.overlay_ref(img, b, s, c, n, atlas=ore.overlay_atlas(), **kw)
    return got, want


@pytest.mark.parametrize("S", [0, 1, 3])
@pytest.mark.parametrize("L", [1, 4])
@pytest.mark.parametrize("hw", [(75, 100), (120, 161)], ids=lambda v: "%dx%d" % v)
def test_host_equals_ref(ore, hw, L, S):
    """Overlapping boxes, boxes partly and wholly outside, degenerate and non-finite rows, equal areas, x.5 % scores, class ids outside
    the names table, labels clamped at the right and bottom edges (overlay_ref.cases), both colour rules."""
    h, w = hw
    img = frame(h, w)
    b, s, c = OR.cases(h, w, seed=L * 10 + S, rows=28)
    for color_by in ("instance", "class"):
        got, want = both(ore, img, b, s, c, score_thresh=0.01, line_width=L, text_scale=S, color_by=color_by, names=NAMES)
        assert got.shape == img.shape and got.dtype == np.uint8
        assert np.array_equal(got, want), int((got != want).sum())
        assert (got != img).any()
    # the count cuts the rows; no classes and no names: percentages only
    got, want = both(ore, img, b, s, None, 9, line_width=L, text_scale=S, edge_alpha=77, label_alpha=255)
    assert np.array_equal(got, want)


def test_cases_cover_what_they_claim(ore):
    """The shared case set really holds the situations the contract separates."""
    h, w = 75, 100
    b, s, c = OR.cases(h, w, rows=28)
    tab = ore.overlay_instance_table(b, s, c, None, h, w, 0.01, 1, ore.OVERLAY_PALETTE, 0, ore.overlay_names_table(NAMES))
    rows = [q["row"] for q in tab]
    assert 0 in rows and 1 in rows and 13 in rows and 14 in rows and 15 in rows
    assert not {2, 3, 5, 6, 7, 8, 9} & set(rows)                               # outside, reversed, non-finite, below the threshold
    assert rows[0] == 13                                                         # the overflowing area is the largest: drawn first
    assert rows.index(10) < rows.index(11)                                       # equal areas: the lower row first
    text = {q["row"]: q["text"] for q in tab}
    assert text[0].endswith(b" 12%") and text[1].endswith(b" 38%")               # 12.5 -> 12, 37.5 -> 38: half to even
    assert text[10] == b"62%" and text[11] == b"100%"                            # ids -2 and 5 have no name; 99.5 -> 100
    lab = {q["row"]: q["label"] for q in tab}
    assert lab[12][0] + lab[12][2] == w and lab[12][1] + lab[12][3] == h         # pushed back into the frame at both edges


def test_literal_fixture(ore):
    """A 12 x 16 frame, one box, no label, derived by hand.  Box (2.5, 3.2, 10.1, 8.9): X0 = floor(2.5) = 2, Y0 = floor(3.2) = 3,
    X1 = ceil(10.1) - 1 = 10, Y1 = ceil(8.9) - 1 = 8; line width 1: the rectangle's border.  Background (10, 100, 200), colour
    (255, 0, 60), alpha 128: (10 * 127 + 255 * 128 + 127) / 255 = 34037 / 255 = 133, (100 * 127 + 0 + 127) / 255 = 12827 / 255 = 50,
    (200 * 127 + 60 * 128 + 127) / 255 = 33207 / 255 = 130."""
    picture = ["................",
               "................",
               "................",
               "..#########.....",
               "..#.......#.....",
               "..#.......#.....",
               "..#.......#.....",
               "..#.......#.....",
               "..#########.....",
               "................",
               "................",
               "................"]
    img = np.empty((12, 16, 3), np.uint8)
    img[:] = (10, 100, 200)
    want = img.copy()
    for y, line in enumerate(picture):
        for x, ch in enumerate(line):
            if ch == "#":
                want[y, x] = (133, 50, 130)
    kw = dict(line_width=1, text_scale=0, edge_alpha=128, palette=np.array([[255, 0, 60]], np.uint8))
    box, score = np.array([[2.5, 3.2, 10.1, 8.9]], np.float32), np.array([0.5], np.float32)
    assert np.array_equal(ore.overlay_host(img, box, score, **kw), want)
    assert np.array_equal(OR.overlay_ref(img, box, score, atlas=ore.overlay_atlas(), **kw), want)
    # line width 2 thickens inwards: row 4 and column 3 join the border, the centre stays
    got = ore.overlay_host(img, box, score, **{**kw, "line_width": 2})
    assert (got[4, 2:11] == (133, 50, 130)).all() and (got[5, 3] == (133, 50, 130)).all() and (got[5, 4] == (10, 100, 200)).all()


def test_properties(ore):
    h, w = 60, 90
    img = frame(h, w, 3)
    b, s, c = OR.cases(h, w, seed=5, rows=20)
    kw = dict(line_width=2, text_scale=1, names=NAMES)
    # n = 0: the frame unchanged, a new array
    got = ore.overlay_host(img, b, s, c, 0, **kw)
    assert np.array_equal(got, img) and got is not img
    assert np.array_equal(ore.overlay_host(img, b[:0], s[:0], c[:0], **kw), img)
    # pixels outside every rectangle and label are unchanged
    small = [0, 4, 14, 15, 16, 17]                                                # without the whole-frame box
    got = ore.overlay_host(img, b[small], s[small], c[small], **kw)
    tab = ore.overlay_instance_table(b[small], s[small], c[small], None, h, w, 0.0, 1, ore.OVERLAY_PALETTE, 0, ore.overlay_names_table(NAMES))
    touched = np.zeros((h, w), bool)
    for q in tab:
        X0, Y0, X1, Y1 = q["rect"]
        touched[Y0:Y1 + 1, X0:X1 + 1] = True
        lx, ly, lw, lh = q["label"]
        touched[ly:ly + lh, lx:lx + lw] = True
    assert len(tab) >= 3 and not touched.all() and np.array_equal(got[~touched], img[~touched]) and (got != img).any()
    # edge_alpha = 255: the pure colour
    pal = np.array([[9, 200, 77]], np.uint8)
    got = ore.overlay_host(img, np.array([[10, 10, 50, 40]], np.float32), np.array([1.0], np.float32), line_width=3, text_scale=0,
                           edge_alpha=255, palette=pal)
    assert (got[10:13, 10:50] == pal[0]).all() and (got[10:40, 47:50] == pal[0]).all() and np.array_equal(got[13:37, 13:47], img[13:37, 13:47])
    # in place: out = the frame
    buf = img.copy()
    assert ore.overlay_host(buf, b, s, c, out=buf, **kw) is buf and np.array_equal(buf, ore.overlay_host(img, b, s, c, **kw))


def test_row_order_does_not_matter_with_class_colours(ore):
    """Rows of distinct areas, coloured by class: any permutation of the rows gives the same picture (the draw order is by area)."""
    h, w = 80, 110
    img = frame(h, w, 9)
    rng = np.random.default_rng(4)
    n = 12
    x0, y0 = rng.uniform(0, w * 0.6, n), rng.uniform(0, h * 0.6, n)
    side = 5.0 + 3.0 * np.arange(n)                                              # distinct areas
    b = np.stack([x0, y0, x0 + side, y0 + side * 0.75], 1).astype(np.float32)
    s = rng.uniform(0.1, 1.0, n).astype(np.float32)
    c = rng.integers(0, 5, n).astype(np.int64)
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    assert len(np.unique(area)) == n
    kw = dict(line_width=2, text_scale=1, names=NAMES, color_by="class")
    want = ore.overlay_host(img, b, s, c, **kw)
    for seed in range(3):
        p = np.random.default_rng(seed).permutation(n)
        assert np.array_equal(ore.overlay_host(img, b[p], s[p], c[p], **kw), want)
        assert np.array_equal(OR.overlay_ref(img, b[p], s[p], c[p], atlas=ore.overlay_atlas(), palette=ore.OVERLAY_PALETTE, **kw), want)


def test_atlas_and_palette(ore):
    a = ore.overlay_atlas()
    assert a.shape == (95, 11, 6) and a.dtype == np.uint8 and set(np.unique(a)) == {0, 1}
    assert not a[0].any() and a[ord("%") - 32].any() and all(a[ord(ch) - 32].any() for ch in "0123456789")
    assert ore.OVERLAY_PALETTE.shape[0] >= 16 and ore.OVERLAY_PALETTE.dtype == np.uint8
    assert len({tuple(c) for c in ore.OVERLAY_PALETTE.tolist()}) == len(ore.OVERLAY_PALETTE)


def test_host_limits(ore):
    img = frame(20, 20)
    b, s = np.array([[1, 1, 9, 9]], np.float32), np.array([0.5], np.float32)
    for kw in (dict(line_width=0, text_scale=1), dict(line_width=17, text_scale=1), dict(line_width=1, text_scale=9),
               dict(line_width=1, text_scale=-1), dict(line_width=1, text_scale=1, edge_alpha=256)):
        with pytest.raises(ore.OreError):
            ore.overlay_host(img, b, s, **kw)
    with pytest.raises(ore.OreError):
        ore.overlay_host(img, np.zeros((321, 4), np.float32), np.zeros(321, np.float32), line_width=1, text_scale=0)
    with pytest.raises(ore.OreError):
        ore.overlay_host(img, b, s, line_width=1, text_scale=0, color_by="area")


def test_read_image_round_trip(tmp_path):
    from PIL import Image
    from detectron2.data.detection_utils import read_image
    from fewx.data.dataset_mapper import _pil_read_image
    rgb = frame(13, 17, 1)
    path = str(tmp_path / "a.png")
    Image.fromarray(rgb).save(path)
    assert np.array_equal(read_image(path, "RGB"), rgb) and np.array_equal(read_image(path), rgb)
    bgr = read_image(path, format="BGR")
    assert np.array_equal(bgr, rgb[:, :, ::-1]) and bgr.flags["C_CONTIGUOUS"]
    grey = read_image(path, "L")
    assert grey.shape == (13, 17, 1) and np.array_equal(grey[:, :, 0], np.asarray(Image.fromarray(rgb).convert("L")))
    assert np.array_equal(_pil_read_image(path), bgr) and np.array_equal(_pil_read_image(path, "RGB"), rgb)
    gpath = str(tmp_path / "g.png")
    Image.fromarray(rgb[:, :, 0]).save(gpath)
    assert read_image(gpath).shape == (13, 17) and read_image(gpath, "BGR").shape == (13, 17, 3)
    with pytest.raises(ValueError):
        read_image(path, "YUV")


def test_read_image_applies_exif_orientation(tmp_path):
    """A file tagged "rotate 90 clockwise to view" (EXIF orientation 6) comes out upright, as upstream's read_image gives it."""
    from PIL import Image
    from detectron2.data.detection_utils import read_image
    rgb = frame(10, 20, 4)
    exif = Image.Exif()
    exif[0x0112] = 6
    path = str(tmp_path / "turned.png")
    Image.fromarray(rgb).save(path, exif=exif)
    want = np.rot90(rgb, -1)
    assert np.array_equal(read_image(path, "RGB"), want) and np.array_equal(read_image(path, "BGR"), want[:, :, ::-1])


def test_demo_helpers(tmp_path):
    """demo.py's own pieces, without a device: the default config resolves next to the script from any directory, the threshold lands
    where the detector reads it, a lone --input is a glob pattern, several inputs need a directory."""
    import demo
    args = demo.get_parser().parse_args(["--input", "x.png", "--output", "o", "--confidence-threshold", "0.25", "--opts", "MODEL.DEVICE", "cpu"])
    assert os.path.isfile(args.config_file) and os.path.isabs(args.config_file)
    cfg = demo.setup_cfg(args)
    assert cfg.MODEL.ROI_HEADS.SCORE_THRESH_TEST == 0.25 and cfg.MODEL.DEVICE == "cpu"
    for name in ("b.png", "a.png", "c.txt"):
        (tmp_path / name).write_bytes(b"")
    assert demo.input_paths([str(tmp_path / "*.png")]) == [str(tmp_path / "a.png"), str(tmp_path / "b.png")]
    assert demo.input_paths(["p", "q"]) == ["p", "q"]
    with pytest.raises(SystemExit, match="no file matches"):
        demo.input_paths([str(tmp_path / "*.jpg")])
    assert demo.output_path(str(tmp_path), "dir/a.png", 2) == str(tmp_path / "a.png")
    assert demo.output_path(str(tmp_path / "one.png"), "dir/a.png", 1) == str(tmp_path / "one.png")
    with pytest.raises(SystemExit, match="need a directory"):
        demo.output_path(str(tmp_path / "one.png"), "dir/a.png", 2)
    for argv in ([], ["--input", "x.png"], ["--webcam", "--input", "x.png"]):
        with pytest.raises(SystemExit):
            demo.main(argv)


def test_demo_names_import():
    from detectron2.utils.video_visualizer import VideoVisualizer
    from detectron2.utils.visualizer import ColorMode, VisImage, Visualizer
    from predictor import AsyncPredictor, VisualizationDemo
    assert {m.name for m in ColorMode} == {"IMAGE", "SEGMENTATION", "IMAGE_BW"}
    for name in ("put", "get", "__len__", "__call__", "shutdown", "default_buffer_size"):
        assert hasattr(AsyncPredictor, name), name
    for name in ("run_on_image", "run_on_video"):
        assert hasattr(VisualizationDemo, name), name
    assert callable(Visualizer.draw_instance_predictions) and callable(VideoVisualizer.draw_instance_predictions) and callable(VisImage.save)


def test_demo_help_lists_the_flags():
    out = subprocess.run([sys.executable, os.path.join(PKG, "demo.py"), "--help"], capture_output=True, text=True, env={**os.environ, "PYTHONPATH": PKG})
    assert out.returncode == 0, out.stderr
    for flag in ("--config-file", "--input", "--output", "--confidence-threshold", "--opts", "--video-input", "--webcam"):
        assert flag in out.stdout, flag


def test_visualizer_on_host_instances(ore, tmp_path):
    """Host Instances go through overlay_host: the picture equals the reference with the defaults of detectron2's proportions; IMAGE
    colours by instance, SEGMENTATION by class; VideoVisualizer by class; VisImage.save writes the picture."""
    from PIL import Image
    from detectron2.data import Metadata
    from detectron2.structures import Boxes, Instances
    from detectron2.utils.video_visualizer import VideoVisualizer
    from detectron2.utils.visualizer import ColorMode, Visualizer, default_overlay_params
    h, w = 90, 140
    assert default_overlay_params(h, w) == {"line_width": 2, "text_scale": 1}
    assert default_overlay_params(1080, 1920) == {"line_width": 4, "text_scale": 1}
    assert default_overlay_params(2160, 3840) == {"line_width": 8, "text_scale": 3}
    assert default_overlay_params(8192, 8192) == {"line_width": 16, "text_scale": 8}
    img = frame(h, w, 2)
    b, s, c = OR.cases(h, w, seed=8, rows=16)
    keep = np.isfinite(b).all(1) & np.isfinite(s)
    inst = Instances((h, w))
    inst.pred_boxes = Boxes(torch.from_numpy(b[keep]))
    inst.scores = torch.from_numpy(s[keep])
    inst.pred_classes = torch.from_numpy(c[keep])
    meta = Metadata(name="t", thing_classes=NAMES)
    ref = lambda color_by: OR.overlay_ref(img, b[keep], s[keep], c[keep], atlas=ore.overlay_atlas(), palette=ore.OVERLAY_PALETTE,
                                          line_width=2, text_scale=1, color_by=color_by, names=NAMES)
    vis = Visualizer(img, meta).draw_instance_predictions(inst)
    assert np.array_equal(vis.get_image(), ref("instance")) and (vis.height, vis.width) == (h, w)
    assert np.array_equal(Visualizer(img, meta, instance_mode=ColorMode.SEGMENTATION).draw_instance_predictions(inst).get_image(), ref("class"))
    assert np.array_equal(VideoVisualizer(meta).draw_instance_predictions(img, inst).get_image(), ref("class"))
    # a BGR frame drawn as BGR comes back as the same RGB picture
    bgr = np.ascontiguousarray(img[:, :, ::-1])
    assert np.array_equal(Visualizer(bgr, meta, channel_order="BGR").draw_instance_predictions(inst).get_image(), ref("instance"))
    path = str(tmp_path / "v.png")
    vis.save(path)
    assert np.array_equal(np.asarray(Image.open(path)), ref("instance"))


def test_visualizer_refusals():
    from detectron2.utils.video_visualizer import VideoVisualizer
    from detectron2.utils.visualizer import ColorMode, Visualizer
    img = np.zeros((8, 8, 3), np.uint8)
    with pytest.raises(ValueError, match="scale"):
        Visualizer(img, scale=1.2)
    with pytest.raises(NotImplementedError, match="masks"):
        Visualizer(img, instance_mode=ColorMode.IMAGE_BW)
    with pytest.raises(NotImplementedError, match="masks"):
        VideoVisualizer(None, ColorMode.IMAGE_BW)
    v = Visualizer(img)
    for method in (v.draw_panoptic_seg_predictions, v.draw_sem_seg, v.draw_dataset_dict):
        with pytest.raises(NotImplementedError, match="boxes only"):
            method(None)


def test_async_predictor_rejects_before_touching_a_device():
    """inflight outside 1 .. 4 and num_gpus != 1 are refused before a model is built (cfg is not even looked at)."""
    from predictor import AsyncPredictor
    for kw in ({"inflight": 0}, {"inflight": 5}, {"num_gpus": 2}, {"num_gpus": 0}):
        with pytest.raises(ValueError):
            AsyncPredictor(None, **kw)
