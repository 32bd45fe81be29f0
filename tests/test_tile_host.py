"""CPU: the host side of tiled inference -- orehip.tile_plan's properties, orehip.tile_gather_host / tile_collect_host against the second
statement in tests/tile_ref.py, and the limits TiledInference refuses before any GPU work."""
import os

import numpy as np
import pytest
import torch

import tile_ref
from conftest import PKG


def _cfg(extra=()):
    from fewx.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(PKG, "configs", "fsod", "finetune_vovnet.yaml"))
    cfg.merge_from_list(["MODEL.WEIGHTS", "", "MODEL.DEVICE", "cpu"] + list(extra))
    return cfg


# ------------------------------------------------------------------------------------------ the plan
def test_plan_properties_over_a_sweep():
    """Per axis, for every (L, t, o) of the sweep: every pixel is covered, the last tile is flush with the far edge, consecutive tiles
    overlap by at least o, all extents are equal (by construction: one extent per axis) and fit the axis, L <= t gives one tile; the
    2-D plan is the row-major product of its axes and equals tests/tile_ref.py's."""
    import orehip
    n = 0
    for t in (1, 2, 7, 64, 100, 640):
        for o in sorted({0, 1, t // 3, t // 2, t - 1}):
            if not 0 <= o < t:
                continue
            for L in sorted({1, 2, t - 1, t, t + 1, 2 * t - o - 1, 2 * t - o, 2 * t - o + 1, 3 * t, 5 * t + 3, 1080, 3840}):
                if L < 1 or (t - o == 1 and L > 50 * t):
                    continue
                p = orehip.tile_plan(L, L + 5, (t, t), (o, o))
                e, s, ny = p["th"], p["stride_y"], p["ny"]
                ys = [y for y, x in p["origins"][::p["nx"]]]
                assert len(ys) == ny and len(p["origins"]) == ny * p["nx"]
                assert e == min(t, L) and s == t - o
                assert ys[0] == 0 and ys[-1] + e == L, (L, t, o, ys)
                assert all(0 <= y and y + e <= L for y in ys)
                covered = np.zeros(L, bool)
                for y in ys:
                    covered[y:y + e] = True
                assert covered.all(), (L, t, o)
                assert all(b > a and a + e - b >= o for a, b in zip(ys, ys[1:])), (L, t, o, ys)
                if L <= t:
                    assert ny == 1
                else:
                    assert ny == -(-(L - t) // s) + 1
                    assert ys == [min(k * s, L - e) for k in range(ny)]
                want = tile_ref.plan(L, L + 5, (t, t), (o, o))
                assert p == want, (L, t, o)
                n += 1
    assert n > 150
    assert orehip.tile_plan(67, 101, (64, 64), (16, 16))["origins"] == [(0, 0), (0, 37), (3, 0), (3, 37)]
    p = orehip.tile_plan(2160, 3840, (640, 640), (128, 128))
    assert (p["ny"], p["nx"], p["th"], p["tw"], p["origins"][-1]) == (4, 8, 640, 640, (1520, 3200))
    for bad in ((64, 64), (64, 70), (64, -1)):
        with pytest.raises(ValueError):
            orehip.tile_plan(100, 100, (64, 64), (bad[1], 0))
    with pytest.raises(ValueError):
        orehip.tile_plan(0, 100, (64, 64), (0, 0))


def test_gather_host_equals_slicing():
    import orehip
    rng = np.random.default_rng(5)
    for (h, w), t, o in (((67, 101), (64, 64), 16), ((50, 300), (64, 128), 32), ((64, 64), (64, 64), 0)):
        frame = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        p = orehip.tile_plan(h, w, t, (o, o))
        for swap in (False, True):
            got = orehip.tile_gather_host(frame, p, swap)
            assert got.dtype == np.uint8 and got.flags.c_contiguous and np.array_equal(got, tile_ref.gather(frame, p, swap))
        for i in range(len(p["origins"])):
            assert orehip.tile_edges(p, i, h, w) == tile_ref.edges_of(p, i, h, w)


# ------------------------------------------------------------------------------------------ the seam rule and the transform
@pytest.mark.parametrize("edges", range(16))
def test_collect_host_equals_reference(edges):
    """Hand-made rows exactly at margin, one ulp either side, at src_w - margin / src_h - margin, NaN and inf rows: the kept rows, their
    order and every bit of the transformed coordinates."""
    import orehip
    for src_hw, margin, (sx, sy, ox, oy) in (((256, 320), 2.0, (1.0, 1.0, 192.0, 37.0)), ((300, 333), 2.7, (1.0, 1.0, 3200.0, 1520.0)),
                                             ((320, 427), 0.0, (640 / 427, 480 / 320, 0.0, 0.0)), ((97, 64), 1.0, (1.7, 0.3, 5.5, 7.25))):
        boxes, scores, classes = tile_ref.hand_rows(120, src_hw, margin, seed=edges * 7 + src_hw[0])
        wb, ws, wc, widx, wdrop = tile_ref.collect(boxes, scores, classes, sx, sy, ox, oy, src_hw, edges, margin)
        gb, gs, gc, kept = orehip.tile_collect_host(boxes, scores, classes, sx=sx, sy=sy, ox=ox, oy=oy, src_hw=src_hw, edges=edges, margin=margin)
        assert gb.dtype == np.float32 and gs.dtype == np.float32 and gc.dtype == np.int64
        assert np.array_equal(np.nonzero(kept)[0], widx) and int((~kept).sum()) == wdrop
        assert gb.tobytes() == wb.tobytes() and np.array_equal(gs, ws) and np.array_equal(gc, wc)
        if edges == 0:
            assert wdrop == 0
        if edges == 15:
            assert 0 < wdrop < len(boxes) and np.isnan(boxes[widx]).any(), "NaN rows pass the seam rule"
    # classes=None: every class 0
    assert (orehip.tile_collect_host(boxes, scores, None, sx=1, sy=1, ox=0, oy=0, src_hw=src_hw, edges=3, margin=1.0)[2] == 0).all()


def test_seam_rule_at_the_margin():
    """The comparisons are strict: a coordinate exactly at the margin (or exactly at size - margin) is kept, one ulp outside is not."""
    import orehip
    f = np.float32
    m, sw, sh = f(2.0), 320, 256
    below, above = np.nextafter(m, f(-1)), np.nextafter(f(sw) - m, f(1e9))
    rows = np.array([[m, m, f(sw) - m, f(sh) - m], [below, 50, 100, 100], [50, below, 100, 100], [50, 50, above, 100],
                     [50, 50, 100, np.nextafter(f(sh) - m, f(1e9))], [np.nan, 0, 400, 400], [0, 0, np.inf, 100]], dtype=np.float32)
    kw = dict(sx=1.0, sy=1.0, ox=0.0, oy=0.0, src_hw=(sh, sw), margin=2.0)
    kept = lambda e: orehip.tile_collect_host(rows, np.ones(len(rows), np.float32), None, edges=e, **kw)[3].tolist()
    assert kept(0) == [True] * 7
    assert kept(15) == [True, False, False, False, False, False, False]
    assert kept(1) == [True, False, True, True, True, True, False]        # NaN x0 passes the left test; x0 = 0 of the inf row does not
    assert kept(4) == [True, True, True, False, True, False, False]
    assert kept(10) == [True, True, False, True, False, False, False]


# ------------------------------------------------------------------------------------------ limits and types
class _Wrapped(torch.nn.Module):
    def __init__(self, module):
        super().__init__()
        self.module = module


def _cpu_model(cfg):
    from detectron2.modeling import build_model
    m = build_model(cfg).eval()
    m.set_support_dict({k: {0: torch.zeros(1, 128, s, s)} for k, s in (("p3", 32), ("p4", 16), ("p5", 8))})
    return m


def test_limits_and_types_without_gpu():
    """Every limit is a ValueError that names the numbers, raised before any GPU work (the model is on the CPU here); a model that is
    not the detector is a TypeError."""
    from fewx.modeling import TiledInference
    from fewx.modeling import tiled_inference as TI
    cfg = _cfg()
    with pytest.raises(TypeError, match="CenterNet2Detector"):
        TiledInference(cfg, torch.nn.Linear(2, 2))
    model = _cpu_model(cfg)
    t = TiledInference(cfg, _Wrapped(model))
    assert t.model is model and (t.tile, t.overlap, t.margin, t.full_frame, t.fold) == ((640, 640), (128, 128), 2.0, True, 1)
    assert (t.topk, t.nms_thresh) == (int(cfg.TEST.DETECTIONS_PER_IMAGE), float(cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST))
    with pytest.raises(ValueError, match="overlap 640x640"):
        TiledInference(cfg, model, tile=640, overlap=640)
    with pytest.raises(ValueError, match="overlap 700x700"):
        TiledInference(cfg, model, tile=(640, 640), overlap=700)
    with pytest.raises(ValueError, match="at least 64"):
        TiledInference(cfg, model, tile=(640, 48), overlap=8)
    for bad in (0, 8193, -3):
        with pytest.raises(ValueError, match=r"max_detections %d outside 1 \.\. 8192" % bad):
            TiledInference(cfg, model, max_detections=bad)
    assert TiledInference(cfg, model, max_detections=8192).topk == 8192
    # more than 128 tiles: 64-pixel tiles of a 1080p frame
    frame = np.zeros((1080, 1920, 3), dtype=np.uint8)
    with pytest.raises(ValueError, match=r"17x30 = 510 tiles.*128"):
        TiledInference(cfg, model, tile=64, overlap=0, full_frame=False)([{"image_raw": frame}])
    # the merge pool: sources x rows
    rows = t._rows()
    assert rows == min(int(cfg.TEST.DETECTIONS_PER_IMAGE), 320)
    side = 160
    plan = __import__("orehip").tile_plan(1080, 1920, (side, side), (0, 0))
    n = plan["ny"] * plan["nx"]
    assert n <= 128 and (n + 1) * rows > 8192
    with pytest.raises(ValueError, match=r"%d sources x %d detection rows = %d candidates.*8192" % (n + 1, rows, (n + 1) * rows)):
        TiledInference(cfg, model, tile=side, overlap=0)([{"image_raw": frame}])
    # a tile beyond the detection tail's level: 1600x1600 -> 200 * 200 locations
    big = np.zeros((1700, 1700, 3), dtype=np.uint8)
    with pytest.raises(ValueError, match=r"1600x1600 tile has 40000 stride-8 locations.*30720"):
        TiledInference(cfg, model, tile=1600, overlap=100, full_frame=False)([{"image_raw": big}])
    # the resized frame beyond it: 1080p at MIN_SIZE_TEST 1200 -> 1200x2133, padded 1216x2144 -> 152 * 268 locations
    with pytest.raises(ValueError, match=r"full-frame pass at 1200x2133 has 40736 stride-8 locations.*30720"):
        TiledInference(_cfg(["INPUT.MIN_SIZE_TEST", 1200, "INPUT.MAX_SIZE_TEST", 4000]), model)([{"image_raw": frame}])
    with pytest.raises(ValueError, match="8192"):
        TiledInference(cfg, model)([{"image_raw": np.zeros((8, 8200, 3), dtype=np.uint8)}])
    # requests
    with pytest.raises(ValueError, match="not both"):
        t([{"image": torch.zeros(3, 64, 64, dtype=torch.uint8), "image_raw": frame}])
    with pytest.raises(ValueError, match="uint8"):
        t([{"image": torch.zeros(3, 64, 64)}])
    with pytest.raises(ValueError, match=r"720x1280 differ from the frame's 1080x1920"):
        t([{"image_raw": frame, "height": 720, "width": 1280}])
    # what the defaults take: 1080p and 2160p at tile 640 / overlap 128 pass every check
    for hw, tiles in (((1080, 1920), 8), ((2160, 3840), 32)):
        plan, full_hw = t.plan(*hw)
        assert plan["ny"] * plan["nx"] == tiles and full_hw is not None
        TI.check_tiling_limits(hw, plan, full_hw, rows)
