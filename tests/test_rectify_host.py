"""CPU: the host statement of the contract "rectify v1" (orehip.rectify_host) against the independent per-pixel reference of
tests/rectify_ref.py and against cases whose bytes can be written down; homography_from_quad and Rectifier; the refusals, those of the C
entry included (ORE_EINVAL comes before any launch, so the addresses are never read); and the reason the feature exists, as a test."""
import ctypes

import numpy as np
import pytest
import torch

import belt_ref as BR
import rectify_ref as RR

QUAD = [(560, 300), (1360, 300), (1900, 1000), (20, 1000)]       # a mild oblique view of a 720 x 1280 belt plane in a 1080 x 1920 frame


@pytest.fixture(scope="module")
def ore():
    import orehip
    return orehip


@pytest.mark.parametrize("case", RR.CASE_IDS)
def test_host_equals_reference(ore, case):
    _, hw, out_hw, M, fill = RR.CASES[RR.CASE_IDS.index(case)]
    got = ore.rectify_host(RR.source(*hw), M, out_hw, fill)
    want = RR.reference(case)
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert np.array_equal(got, want), np.argwhere((got != want).any(2))[:5]


def test_exact_cases(ore):
    """Identity: the source; an integer shift: shifted bytes and fill exactly where the source ends; a half-pixel shift: the rounded
    means (a + b + c + d + 2) >> 2 of the four taps, clamped at the far edges."""
    hs, ws = 33, 65
    src = RR.source(hs, ws)
    assert np.array_equal(ore.rectify_host(src, np.eye(3), (hs, ws)), src)
    assert np.array_equal(ore.rectify_host(torch.from_numpy(src), np.eye(3).reshape(9).tolist(), (hs, ws)), src)
    fill = (200, 100, 50)
    got = ore.rectify_host(src, [[1, 0, 3], [0, 1, -2], [0, 0, 1]], (hs, ws), fill)       # out[i][j] = src[i - 2][j + 3]
    want = np.empty_like(src)
    want[:] = np.array(fill, np.uint8)
    want[2:, :ws - 3] = src[:hs - 2, 3:]
    assert np.array_equal(got, want)
    got = ore.rectify_host(src, [[1, 0, 0.5], [0, 1, 0.5], [0, 0, 1]], (hs, ws))
    p = np.pad(src.astype(np.int64), ((0, 1), (0, 1), (0, 0)), mode="edge")
    want = (p[:-1, :-1] + p[:-1, 1:] + p[1:, :-1] + p[1:, 1:] + 2) >> 2
    assert np.array_equal(got, want.astype(np.uint8))
    # a larger output than the source: the source in the corner, fill around it
    got = ore.rectify_host(src, np.eye(3), (hs + 4, ws + 5), fill)
    assert np.array_equal(got[:hs, :ws], src) and (got[hs:] == fill).all() and (got[:, ws:] == fill).all()


@pytest.mark.parametrize("name", ["min2", "perspective"])
def test_positions_agree_with_float64(ore, name):
    """The contract's fixed-point positions lie within 1/256 px of the float64 evaluation of the same fp32 matrix, and the bytes are the
    integer blend at the contract's own positions."""
    (hs, ws), (ho, wo) = (33, 65), (24, 40)
    src = RR.source(hs, ws)
    M = np.asarray(RR.matrices(hs, ws, ho, wo)[name], dtype=np.float64).astype(np.float32)
    got = ore.rectify_host(src, M, (ho, wo))
    m, m64 = [float(v) for v in M.reshape(9)], M.astype(np.float64)
    worst, inside_n = 0.0, 0
    for i in range(ho):
        for j in range(wo):
            X, Y, Z = m64 @ np.array([j + 0.5, i + 0.5, 1.0])
            inside, U, V = RR.positions(m, i, j, hs, ws)
            if not inside:
                assert tuple(got[i, j]) == (0, 0, 0)
                continue
            inside_n += 1
            worst = max(worst, abs(U / 256.0 - (X / Z - 0.5)), abs(V / 256.0 - (Y / Z - 0.5)))
            assert list(got[i, j]) == RR.blend(src, U, V), (i, j)
    print(f"{name}: {inside_n} of {ho * wo} pixels inside, worst position error {worst * 256:.4f} / 256 px")
    assert inside_n > ho * wo // 4 and worst <= 1.0 / 256.0


def test_horizon(ore):
    """Z changes sign inside the output: every pixel with Z <= 0 is fill, and the pixels in front of the horizon are the reference's."""
    hs, ws, ho, wo, fill = 33, 65, 64, 67, (9, 8, 7)
    got = ore.rectify_host(RR.source(hs, ws), RR.horizon(ho), (ho, wo), fill)
    behind = (1.0 - 2.0 * (np.arange(ho) + 0.5) / ho) <= 0
    assert behind.sum() == ho // 2 and (got[behind] == np.array(fill, np.uint8)).all()
    assert np.array_equal(got, RR.reference("33x65-64x67-horizon")) and (got[~behind][:, :8] != np.array(fill, np.uint8)).any()


def test_homography_from_quad(ore):
    for out_hw, quad in (((720, 1280), QUAD), ((100, 50), [(3.5, 2), (40, 7.25), (47, 90), (-4, 80)]), ((64, 64), [(0, 0), (64, 0), (64, 64), (0, 64)])):
        M = ore.homography_from_quad(quad, out_hw)
        assert M.dtype == np.float64 and M.shape == (3, 3) and M[2, 2] == 1.0
        ho, wo = out_hw
        c = np.array([[0, 0, 1], [wo, 0, 1], [wo, ho, 1], [0, ho, 1]], dtype=np.float64) @ M.T
        assert (c[:, 2] > 0).all()
        assert np.abs(c[:, :2] / c[:, 2:] - np.asarray(quad, np.float64)).max() < 1e-6
    assert np.allclose(ore.homography_from_quad([(0, 0), (64, 0), (64, 64), (0, 64)], (64, 64)), np.eye(3), atol=1e-12)
    for bad in ([(0, 0), (10, 0), (20, 0), (0, 10)],                  # three points on a line
                [(0, 0), (0, 0), (10, 10), (0, 10)],                  # a repeated point
                [(0, 0), (10, 10), (10, 0), (0, 10)],                 # a bow tie: the points do not run round the quad
                [(0, 0), (10, 0), (2, 2), (0, 10)],                   # not convex: a corner falls behind the camera
                [(0, 0), (10, 0), (10, 10)], [(0, 0), (10, 0), (10, float("nan")), (0, 10)]):
        with pytest.raises(ValueError, match="homography_from_quad"):
            ore.homography_from_quad(bad, (32, 32))
    with pytest.raises(ValueError):
        ore.homography_from_quad(QUAD, (0, 32))


def test_rectifier_round_trip_and_boxes(ore):
    R = ore.Rectifier(quad=QUAD, out_hw=(720, 1280), fill=(1, 2, 3))
    assert R.M.dtype == np.float32 and R.M.shape == (3, 3) and R.out_hw == (720, 1280) and R.fill == (1, 2, 3)
    assert np.array_equal(R.M, ore.homography_from_quad(QUAD, (720, 1280)).astype(np.float32))
    rng = np.random.default_rng(5)
    p = rng.uniform(0, 1, (200, 2)) * np.array([1280.0, 720.0])
    s = R.to_source(p)
    assert s.dtype == np.float64 and s.shape == (200, 2)
    assert np.abs(R.to_rectified(s) - p).max() < 1e-9
    assert np.abs(R.to_source([(0, 0), (1280, 0), (1280, 720), (0, 720)]) - np.array(QUAD, np.float64)).max() < 1e-3   # .M is fp32
    lo = rng.uniform(0, 1, (50, 2)) * np.array([1200.0, 650.0])
    boxes = np.concatenate([lo, lo + rng.uniform(20, 70, (50, 2))], 1)
    cam = R.boxes_to_source(boxes)
    assert cam.shape == (50, 4) and (cam[:, 2:] > cam[:, :2]).all()
    corners = R.to_source(boxes[:, [0, 1, 2, 1, 2, 3, 0, 3]].reshape(-1, 2)).reshape(50, 4, 2)
    assert np.array_equal(cam, np.concatenate([corners.min(1), corners.max(1)], 1))
    back = R.boxes_to_rectified(cam)                                 # the bounds of the bounds: they contain the box they came from
    assert (back[:, :2] <= boxes[:, :2] + 1e-9).all() and (back[:, 2:] >= boxes[:, 2:] - 1e-9).all()
    same = ore.Rectifier(R.M, out_hw=(720, 1280))
    assert np.array_equal(same.M, R.M)
    # a host frame goes through rectify_host, as an array or as a tensor
    small = ore.Rectifier([[1, 0, 3], [0, 1, -2], [0, 0, 1]], out_hw=(9, 11), fill=(4, 5, 6))
    src = RR.source(5, 7)
    want = ore.rectify_host(src, small.M, (9, 11), (4, 5, 6))
    assert np.array_equal(small(src), want) and torch.equal(small(torch.from_numpy(src)), torch.from_numpy(want))


def test_refusals(ore):
    src, eye = RR.source(5, 7), np.eye(3)
    for bad in (np.eye(2), list(range(8)), "matrix", [[1, 0, 0], [0, 1, 0], [0, float("inf"), 1]], [[1, 0, 0], [0, float("nan"), 0], [0, 0, 1]],
                np.eye(3) * 1e39):
        with pytest.raises(ValueError, match="M "):
            ore.rectify_host(src, bad, (5, 7))
    for bad in ((0, 7), (5, 16385), (5,), (5.0, 7), None):
        with pytest.raises(ValueError, match="out_hw"):
            ore.rectify_host(src, eye, bad)
    for bad in ((0, 0), (0, 0, 256), (0, -1, 0), 7, (0.5, 0, 0)):
        with pytest.raises(ValueError, match="fill"):
            ore.rectify_host(src, eye, (5, 7), bad)
    for bad in (src.astype(np.float32), src[:, :, :2], src[0], np.zeros((0, 7, 3), np.uint8)):
        with pytest.raises(ValueError):
            ore.rectify_host(bad, eye, (5, 7))
    with pytest.raises(ValueError, match="device tensor"):
        ore.rectify_u8(torch.from_numpy(src), eye, (5, 7))
    with pytest.raises(ValueError, match="device tensor"):
        ore.rectify_u8(src, eye, (5, 7))
    for kw in ({}, {"M": eye, "quad": QUAD}):
        with pytest.raises(ValueError, match="exactly one"):
            ore.Rectifier(out_hw=(5, 7), **kw)
    with pytest.raises(ValueError, match="singular"):
        ore.Rectifier(np.zeros((3, 3)), out_hw=(5, 7))
    with pytest.raises(ValueError):
        ore.Rectifier(eye, out_hw=(5, 0))


def test_c_entry_refusals(ore):
    """ore_rectify_u8_fwd answers ORE_EINVAL with a message naming it before any launch; the addresses are never read."""
    L = ore.lib()
    m9 = lambda *v: (ctypes.c_float * 9)(*(v or (1, 0, 0, 0, 1, 0, 0, 0, 1)))
    ok = dict(src=0x10000, hs=5, ws=7, m=m9(), dst=0x20000, ho=3, wo=5, fill=0)
    nan9, inf9 = [1, 0, 0, 0, 1, 0, 0, 0, float("nan")], [float("inf"), 0, 0, 0, 1, 0, 0, 0, 1]
    for bad in (dict(src=None), dict(dst=None), dict(m=None), dict(hs=0), dict(ws=16385), dict(ho=-1), dict(wo=0), dict(wo=16385),
                dict(m=m9(*nan9)), dict(m=m9(*inf9)), dict(fill=-1), dict(fill=1 << 24), dict(dst=0x10000), dict(dst=0x10000 + 5 * 7 * 3 - 1),
                dict(src=0x20000 + 3 * 5 * 3 - 1)):
        a = dict(ok, **bad)
        rc = L.ore_rectify_u8_fwd(a["src"], a["hs"], a["ws"], a["m"], a["dst"], a["ho"], a["wo"], a["fill"], None)
        assert rc == -22 and L.ore_last_error().startswith(b"ore_rectify_u8_fwd"), (bad, rc, L.ore_last_error())
    assert ore.RECTIFY_MAX_SIDE == 16384 and "ore_rectify_u8_fwd" in ore.SYMBOLS


def test_demo_flags_and_wiring_surfaces(ore, tmp_path):
    """demo.py's --rectify-quad / --rectify-size without a device: the rectifier they make, the input frame's size as the default,
    the refusals; and rectify=None as the default of every wrapper."""
    import inspect
    from PIL import Image
    import demo
    from detectron2.engine.defaults import DefaultPredictor
    from predictor import AsyncPredictor, TiledPredictor, VisualizationDemo
    path = str(tmp_path / "frame.png")
    Image.fromarray(np.zeros((108, 192, 3), np.uint8)).save(path)
    quad = [56, 30, 136, 30, 190, 100, 2, 100]
    flags = ["--rectify-quad"] + [str(v) for v in quad]
    args = demo.get_parser().parse_args(["--input", path, "--output", "o"] + flags)
    R = demo.make_rectifier(args)
    assert isinstance(R, ore.Rectifier) and R.out_hw == (108, 192)
    assert np.abs(R.to_source([(0, 0), (192, 0), (192, 108), (0, 108)]).reshape(-1) - np.array(quad, np.float64)).max() < 1e-3
    args = demo.get_parser().parse_args(["--input", path, "--output", "o", "--rectify-size", "128", "72"] + flags)
    assert demo.make_rectifier(args).out_hw == (72, 128)
    assert demo.make_rectifier(demo.get_parser().parse_args(["--input", path, "--output", "o"])) is None
    for argv in (["--rectify-size", "128", "72"], ["--rectify-quad", "0", "0", "10", "0", "20", "0", "0", "10"],
                 flags + ["--rectify-size", "0", "72"]):
        with pytest.raises(SystemExit) as e:
            demo.main(["--input", path, "--output", "o"] + argv)
        assert "demo.py: --rectify" in str(e.value), argv
    for fn in (DefaultPredictor.__init__, AsyncPredictor.put, AsyncPredictor.__call__, VisualizationDemo.__init__, TiledPredictor.__init__):
        assert inspect.signature(fn).parameters["rectify"].default is None, fn


# ------------------------------------------------------------------------------------------ the reason
def _planted_plane():
    """40 boxes of 20 .. 70 px moving (37, 2) px per frame in a 720 x 1280 belt plane, 8 frames, +-1 px of jitter; a box is seen while
    it lies wholly inside the plane."""
    out = []
    for b, s, c, n, o in BR.belt_sequence(40, shift=(37, 2), frames=8, seed=0, frame=(720, 1280), miss=0.0):
        keep = (b[:, 0] >= 0) & (b[:, 1] >= 0) & (b[:, 2] <= 1280) & (b[:, 3] <= 720)
        out.append((b[keep], s[keep], c[keep], int(keep.sum()), o[keep]))
    return out


def _tracked(ore, frames, frame):
    tr = ore.WideBeltTracker("cpu", frame=frame)
    ids = [tr.update(b, s, c, n).numpy() for b, s, c, n, _ in frames]
    return tr.stats(), BR.kept_ids(frames, ids)


def test_oblique_view_loses_tracks_and_rectified_boxes_keep_them(ore):
    """The planted belt seen through the oblique view (boxes_to_source) splits the belt's vote: more tracks are started than there are
    objects and continuations are lost.  The same boxes brought back (boxes_to_rectified) start exactly one track per object and keep
    every continuation, as the boxes of the plane themselves do."""
    R = ore.Rectifier(quad=QUAD, out_hw=(720, 1280))
    plane = _planted_plane()
    objects = len({int(o) for f in plane for o in f[4]})
    cam = [(R.boxes_to_source(b).astype(np.float32), s, c, n, o) for b, s, c, n, o in plane]
    back = [(R.boxes_to_rectified(b).astype(np.float32), s, c, n, o) for b, s, c, n, o in cam]
    assert all((b[:, 0] >= 0).all() and (b[:, 2] <= 1920).all() and (b[:, 1] >= 0).all() and (b[:, 3] <= 1080).all() for b, *_ in cam)
    st_plane, (kept_plane, total) = _tracked(ore, plane, (720, 1280))
    st_cam, (kept_cam, total_cam) = _tracked(ore, cam, (1080, 1920))
    st_back, (kept_back, total_back) = _tracked(ore, back, (720, 1280))
    print(f"{objects} objects, {total} continuations: plane {st_plane['started']} tracks, {kept_plane} kept; camera view "
          f"{st_cam['started']} tracks, {kept_cam} kept, peak {st_cam['votes']} votes; rectified {st_back['started']} tracks, {kept_back} kept")
    assert objects > 30 and total == total_cam == total_back and total > 5 * objects
    assert st_plane["started"] == objects and kept_plane == total
    assert st_cam["started"] > objects and kept_cam < total
    assert st_back["started"] == objects and kept_back == total
