"""CPU: the association contract "track v1" (include/ore_hip.h) as orehip.track_host states it, against the independent restatement
tests/track_ref.py and a hand-written scenario; "overlay v1, track colouring" as overlay_host states it against
tests/overlay_track_ref.py; the surfaces built on both (BoxTracker on host tensors, VideoVisualizer(track=True), the demo's flag)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT
import overlay_ref as OR
import overlay_track_ref as OTR
import track_ref as TR

NAMES = ["stone", "a-rather-long-class-name-of-32-b", "cat", "x", "dog"]
SHAPES = [(0, 1), (1, 1), (5, 8), (64, 64), (65, 130), (320, 1024)]


@pytest.fixture(scope="module")
def ore():
    import orehip
    return orehip


def run_both(ore, frames, **kw):
    """Every frame through track_host and the reference; ids and the whole state must agree after each.  Returns the per-frame ids and
    the reference states."""
    host, ref, out = None, TR.empty_state(), []
    for f, (b, s, c, n) in enumerate(frames):
        ids, host = ore.track_host(host, b, s, c, n, **kw)
        want, ref = TR.update_ref(ref, b, s, c, n, **kw)
        assert ids.dtype == np.int64 and np.array_equal(ids, want), (f, ids, want)
        assert TR.same_state(host, ref), f
        out.append((ids, ref))
    return out


@pytest.mark.parametrize("rows,capacity", SHAPES, ids=lambda v: str(v))
def test_host_equals_ref_on_sequences(ore, rows, capacity):
    frames = TR.sequence(rows, seed=rows)
    res = run_both(ore, frames, capacity=capacity, score_thresh=0.05)
    run_both(ore, [(b, s, None, n) for b, s, _, n in frames], capacity=capacity, score_thresh=0.05, class_aware=False, ttl=3)
    if rows >= 5:                                            # the sequences do what they claim: ids persist, new ones appear, rows die
        first, last = res[0][1], res[-1][1]
        assert last["next_id"] > first["next_id"] > 0
        assert any((ids == -1).any() for ids, _ in res)
        seen0 = set(res[0][0][res[0][0] >= 0])
        assert seen0 & set(res[1][0][res[1][0] >= 0])
    if (rows, capacity) == (64, 64):
        assert res[-1][1]["dropped"] > 0                     # the overflow path


def test_host_equals_ref_on_ties_and_chain(ore):
    res = run_both(ore, TR.ties_case())
    assert res[1][1]["n_pairs"] >= 20
    res = run_both(ore, TR.chain_case(40), iou_thresh=TR.CHAIN_IOU_THRESH)
    assert np.array_equal(res[1][0], np.arange(40))          # row i continues track i: the greedy order walks the chain from the left
    t, r = TR.chain_case(40)[0][0], TR.chain_case(40)[1][0]
    assert TR.mutual_best_rounds(t, r, TR.CHAIN_IOU_THRESH) >= 10


def test_literal_three_frames(ore):
    """Hand-derived.  Frame 0: A = (0,0,10,10), B = (20,0,30,10) -> ids 0, 1.  Frame 1 lists a box near B first, then a new box C, then a
    dead row: B' = (21,0,31,10) has IoU 90 / 110 = 0.818 with B -> id 1; C = (50,50,60,60) -> id 2; the NaN row -> -1.  A was missed:
    it stays behind the rows with ttl 7.  Frame 2: A' = (1,0,11,10), IoU 0.818 with A -> id 0 again, ttl back to 8; B and C are missed
    -> ttl 7 each, in their previous order."""
    kw = dict(capacity=8, iou_thresh=0.6, ttl=8)
    f0 = np.array([[0, 0, 10, 10], [20, 0, 30, 10]], np.float32)
    f1 = np.array([[21, 0, 31, 10], [50, 50, 60, 60], [np.nan, 0, 5, 5]], np.float32)
    f2 = np.array([[1, 0, 11, 10]], np.float32)
    ids, st = ore.track_host(None, f0, np.ones(2, np.float32), **kw)
    assert ids.tolist() == [0, 1] and st["ttl"].tolist() == [8, 8] and st["next_id"] == 2 and st["m"] == 2
    ids, st = ore.track_host(st, f1, np.ones(3, np.float32), **kw)
    assert ids.tolist() == [1, 2, -1]
    assert st["ids"].tolist() == [1, 2, 0] and st["ttl"].tolist() == [8, 8, 7] and st["next_id"] == 3
    assert st["boxes"].tolist() == [[21, 0, 31, 10], [50, 50, 60, 60], [0, 0, 10, 10]]
    ids, st = ore.track_host(st, f2, np.ones(1, np.float32), **kw)
    assert ids.tolist() == [0]
    assert st["ids"].tolist() == [0, 1, 2] and st["ttl"].tolist() == [8, 7, 7] and st["next_id"] == 3
    assert (st["frames"], st["dropped"], st["m"]) == (3, 0, 3)
    # the reference reads the scenario the same way
    ref = TR.empty_state()
    for f in (f0, f1, f2):
        _, ref = TR.update_ref(ref, f, np.ones(len(f), np.float32), **kw)
    assert TR.same_state(st, ref)


def test_properties(ore):
    """Live rows get distinct ids; an id never comes back once its track has expired; class_aware=False matches across classes; the
    thresholds are strict (IoU) and inclusive (score)."""
    frames = TR.sequence(40, frames=20, seed=3)
    st, alive_before, expired = None, set(), set()
    for b, s, c, n in frames:
        ids, st = ore.track_host(st, b, s, c, n, ttl=2, score_thresh=0.05)
        live = ids[ids >= 0]
        assert len(set(live.tolist())) == len(live)
        now = set(st["ids"].tolist())
        assert len(now) == st["m"]
        expired |= alive_before - now
        assert not expired & set(live.tolist())
        alive_before = now
    assert expired
    box = np.array([[0, 0, 10, 10]], np.float32)
    one = np.ones(1, np.float32)
    _, st = ore.track_host(None, box, one, np.array([3]))
    assert ore.track_host(st, box, one, np.array([4]))[0].tolist() == [1]
    assert ore.track_host(st, box, one, np.array([4]), class_aware=False)[0].tolist() == [0]
    # inter 3 over union 5: the quotient rounds to fp32(0.6), the threshold itself -> not a candidate (the comparison is strict)
    a, b3, b4 = np.array([[0, 0, 4, 1]], np.float32), np.array([[1, 0, 5, 1]], np.float32), np.array([[0.5, 0, 4.5, 1]], np.float32)
    assert TR.iou_ref(a[0], b3[0]) == np.float32(0.6)
    _, st = ore.track_host(None, a, one)
    assert ore.track_host(st, b3, one, iou_thresh=np.float32(0.6))[0].tolist() == [1]
    assert ore.track_host(st, b4, one, iou_thresh=np.float32(0.6))[0].tolist() == [0]      # 3.5 / 4.5
    assert ore.track_host(None, a, np.array([0.25], np.float32), score_thresh=0.25)[0].tolist() == [0]
    assert ore.track_host(None, a, np.array([0.2499], np.float32), score_thresh=0.25)[0].tolist() == [-1]
    for bad in (dict(capacity=0), dict(capacity=1025), dict(ttl=0), dict(ttl=(1 << 20) + 1), dict(iou_thresh=-0.1), dict(iou_thresh=float("nan")),
                dict(iou_thresh=float("inf"))):
        with pytest.raises(ore.OreError):
            ore.track_host(None, a, one, **bad)


def test_box_tracker_on_host_tensors(ore):
    """BoxTracker("cpu") is track_host with the state kept: ids per frame, Instances in and track_ids out, stats, reset."""
    from detectron2.structures import Boxes, Instances
    frames = TR.sequence(12, frames=6, seed=5)
    tr = ore.BoxTracker("cpu", capacity=16, score_thresh=0.05)
    ref = TR.empty_state()
    for b, s, c, n in frames:
        ids = tr.update(torch.from_numpy(b), torch.from_numpy(s), torch.from_numpy(c), n)
        want, ref = TR.update_ref(ref, b, s, c, n, capacity=16, score_thresh=0.05)
        assert ids.dtype == torch.int64 and np.array_equal(ids.numpy(), want)
    assert tr.stats() == {"tracks": len(ref["tracks"]), "started": ref["next_id"], "frames": 6, "dropped": ref["dropped"]}
    assert TR.same_state(tr.state_host(), ref)
    assert set(tr.state()) == {"boxes", "classes", "ids", "ttl", "m", "next_id", "frames", "dropped"}
    tr.reset()
    assert tr.stats() == {"tracks": 0, "started": 0, "frames": 0, "dropped": 0}
    b, s, c, _ = frames[0]
    keep = np.isfinite(b).all(1)
    inst = Instances((400, 400))
    inst.pred_boxes, inst.scores, inst.pred_classes = Boxes(torch.from_numpy(b[keep])), torch.from_numpy(s[keep]), torch.from_numpy(c[keep])
    ids = tr.update(inst)
    assert inst.has("track_ids") and inst.track_ids is ids and len(ids) == int(keep.sum())


@pytest.mark.parametrize("S", [0, 1, 2])
@pytest.mark.parametrize("hw", [(75, 100), (120, 161)], ids=lambda v: "%dx%d" % v)
def test_overlay_host_track_colouring(ore, hw, S):
    h, w = hw
    img = np.random.default_rng(h).integers(0, 256, (h, w, 3), dtype=np.uint8)
    b, s, c = OR.cases(h, w, seed=S, rows=28)
    c[1] = 1                                                     # the 32-byte name behind a 19-digit id: the text is cut at 40
    ids = OTR.track_ids_for(28, seed=S)
    kw = dict(score_thresh=0.01, line_width=2, text_scale=S, names=NAMES, palette=ore.OVERLAY_PALETTE)
    got = ore.overlay_host(img, b, s, c, ids=ids, color_by="track", **kw)
    want = OTR.overlay_track_ref(img, b, s, c, ids, atlas=ore.overlay_atlas(), **kw)
    assert np.array_equal(got, want), int((got != want).sum())
    assert (got != img).any()
    # the count cuts the rows; no classes, no names
    got = ore.overlay_host(img, b, s, None, 12, ids=ids, color_by="track", **dict(kw, names=None))
    assert np.array_equal(got, OTR.overlay_track_ref(img, b, s, None, ids, 12, atlas=ore.overlay_atlas(), **dict(kw, names=None)))
    # ids given but another colour rule: the bytes of today's overlay; "track" without ids is refused
    for by in ("instance", "class"):
        assert np.array_equal(ore.overlay_host(img, b, s, c, ids=ids, color_by=by, **kw), ore.overlay_host(img, b, s, c, color_by=by, **kw))
    with pytest.raises(ore.OreError, match="ids"):
        ore.overlay_host(img, b, s, c, color_by="track", **kw)
    if S:
        tab = ore.overlay_instance_table(b, s, c, None, h, w, 0.01, S, ore.OVERLAY_PALETTE, 2, ore.overlay_names_table(NAMES), ids=ids)
        texts = {q["row"]: q["text"] for q in tab}
        assert texts[1] == b"#9223372036854775807 a-rather-long-class" and len(texts[1]) == 40
        assert texts[0].startswith(b"#7 ") and 12 not in texts


def test_surfaces_exist(ore):
    import inspect
    import demo
    from detectron2.utils.video_visualizer import VideoVisualizer
    from detectron2.utils.visualizer import draw_boxes
    from predictor import AsyncPredictor, VisualizationDemo
    for name in ("ore_track_state_bytes", "ore_track_reset", "ore_track_workspace_bytes", "ore_track_update_fwd", "ore_overlay_draw_ids_fwd"):
        assert name in ore.SYMBOLS and hasattr(ore.lib(), name), name
    L = ore.lib()
    assert L.ore_track_state_bytes(0) == 0 and L.ore_track_state_bytes(1025) == 0
    assert L.ore_track_state_bytes(1) == 80 and L.ore_track_state_bytes(1024) == 32 + 36 * 1024
    assert L.ore_track_workspace_bytes(1024, 320) == 0
    for bad in ((None, 0, None), (None, 1025, None)):
        assert L.ore_track_reset(*bad) != 0 and b"capacity" in L.ore_last_error()
    # ORE_EINVAL comes before any launch, so the refusals can be seen without a device: the addresses are never read
    st, rows, ids = 0x10000, 0x20000, 0x30000
    ok = dict(state=st, capacity=16, n_host=8, max_rows=8, score=0.0, iou=0.6, ttl=8, ids=ids)
    for bad in (dict(capacity=0), dict(capacity=1025), dict(max_rows=321), dict(max_rows=-1), dict(n_host=-1), dict(ttl=0), dict(ttl=(1 << 20) + 1),
                dict(iou=-0.1), dict(iou=float("nan")), dict(iou=float("inf")), dict(score=float("nan")), dict(state=0), dict(state=st + 8),
                dict(ids=0), dict(ids=st + 64), dict(ids=rows), dict(state=rows + 16)):
        a = dict(ok, **bad)
        rc = L.ore_track_update_fwd(a["state"], a["capacity"], rows, rows + 0x1000, rows + 0x2000, None, a["n_host"], a["max_rows"], a["score"],
                                    a["iou"], a["ttl"], 1, a["ids"], None, 0, None)
        assert rc == -22 and L.ore_last_error().startswith(b"ore_track_update_fwd"), (bad, rc)
    assert L.ore_overlay_draw_ids_fwd(st, st, 8, 8, rows, rows + 0x1000, None, None, None, 4, 4, 0.0, 1, 0, 128, 204, ids, 20, 2, None, 0, None,
                                      0x40000, 1 << 20, None) == -22 and b"needs ids" in L.ore_last_error()
    sig = inspect.signature(ore.BoxTracker.__init__).parameters
    assert {k: sig[k].default for k in ore.TRACK_DEFAULTS} == ore.TRACK_DEFAULTS == {"capacity": 1024, "iou_thresh": 0.6, "ttl": 8, "class_aware": True,
                                                                                      "score_thresh": 0.0}
    for name in ("update", "reset", "state", "stats"):
        assert callable(getattr(ore.BoxTracker, name))
    assert inspect.signature(VideoVisualizer.__init__).parameters["track"].default is False
    assert inspect.signature(AsyncPredictor.put).parameters["track"].default is None
    assert inspect.signature(VisualizationDemo.__init__).parameters["track"].default is False
    assert callable(VisualizationDemo.track_stats) and "ids" in inspect.signature(draw_boxes).parameters
    assert "ids" in inspect.signature(ore.overlay_draw).parameters and "ids" in inspect.signature(ore.overlay_host).parameters
    args = demo.get_parser().parse_args(["--track", "--input", "a.png", "b.png", "--output", "o"])
    assert args.track and not demo.get_parser().parse_args(["--input", "a.png"]).track
    with pytest.raises(SystemExit, match="sequence"):
        demo.main(["--track", "--input", "a.png", "--output", "o"])
    out = subprocess.run([sys.executable, os.path.join(PKG, "demo.py"), "--help"], capture_output=True, text=True, env={**os.environ, "PYTHONPATH": PKG})
    assert out.returncode == 0 and "--track" in out.stdout
    with open(os.path.join(ROOT, "include", "ore_hip.h")) as f:
        header = f.read()
    assert "detection tracking" in header and '"track v1"' in header and "overlay v1, track colouring" in header


def test_video_visualizer_tracks_host_instances(ore):
    """VideoVisualizer(track=True) over 3 frames of host Instances: the picture is overlay_host's with the reference's ids, and
    predictions.track_ids holds them; track=False draws what it draws today."""
    from detectron2.data import Metadata
    from detectron2.structures import Boxes, Instances
    from detectron2.utils.video_visualizer import VideoVisualizer
    h, w = 90, 140
    meta = Metadata(name="tt", thing_classes=NAMES)
    rng = np.random.default_rng(4)
    base = np.array([[10, 10, 60, 50], [70, 20, 130, 80], [30, 40, 90, 85], [5, 60, 40, 88]], np.float32)
    frames = []
    for f in range(3):
        b = (base + np.float32(2 * f))[[(k + f) % 4 for k in range(4)]][: 4 - (f == 1)]
        frames.append((b.astype(np.float32), rng.uniform(0.3, 1, len(b)).astype(np.float32), np.array([0, 2, 2, 4])[[(k + f) % 4 for k in range(len(b))]]))
    tracked, plain, ref = VideoVisualizer(meta, track=True), VideoVisualizer(meta), TR.empty_state()
    all_ids = []
    for f, (b, s, c) in enumerate(frames):
        img = np.random.default_rng(f).integers(0, 256, (h, w, 3), dtype=np.uint8)
        inst = Instances((h, w))
        inst.pred_boxes, inst.scores, inst.pred_classes = Boxes(torch.from_numpy(b)), torch.from_numpy(s), torch.from_numpy(c)
        want_ids, ref = TR.update_ref(ref, b, s, c)
        got = tracked.draw_instance_predictions(img, inst).get_image()
        assert np.array_equal(inst.track_ids.numpy(), want_ids)
        kw = dict(palette=ore.OVERLAY_PALETTE, names=NAMES, line_width=2, text_scale=1)
        assert np.array_equal(got, ore.overlay_host(img, b, s, c, ids=want_ids, color_by="track", **kw))
        assert np.array_equal(got, OTR.overlay_track_ref(img, b, s, c, want_ids, atlas=ore.overlay_atlas(), **kw))
        assert np.array_equal(plain.draw_instance_predictions(img, inst).get_image(),
                              OR.overlay_ref(img, b, s, c, atlas=ore.overlay_atlas(), color_by="class", **kw))
        all_ids.append(want_ids)
    assert set(all_ids[0]) == set(all_ids[2]) == {0, 1, 2, 3} and ref["next_id"] == 4       # every id persisted
    assert isinstance(tracked.tracker, ore.BoxTracker) and tracked.tracker.stats()["started"] == 4
