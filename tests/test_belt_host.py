"""CPU: orehip.belt_shift_host, the numpy statement of the contract "belt shift v1" (include/ore_hip.h), equals tests/belt_ref.py -- loops
over np.float32 scalars and a dict for the histogram -- on every field of the track state and of the belt state: on moving sequences,
on the tie rules of the peak, at the edges of the window and of the size gate, with and without classes, on empty inputs and at the
frame's border.  Then the property the shift exists for: on a planted belt every object seen in two consecutive frames keeps its id
under the belt trackers, and none does under "track v1" alone."""
import functools

import numpy as np
import pytest

import belt_ref as BR

SCORE = 0.05                                                   # track_ref.sequence plants scores of 0.01


@pytest.fixture(scope="module")
def ore():
    import orehip
    return orehip


def both(ore_, state, belt, rows, **kw):
    """One shift through the host statement and through the reference: equal on every field; returns the host's pair."""
    got_s, got_b = ore_.belt_shift_host(state, belt, *rows, **kw)
    want_s, want_b = BR.shift_ref(state, belt, *rows, **kw)
    assert BR.same_belt(got_b, want_b), (got_b, want_b)
    assert BR.same_tracks(got_s, want_s)
    assert set(got_b) == set(BR.BELT_KEYS)
    return got_s, got_b, want_s["n_votes"]


@functools.lru_cache(maxsize=None)
def sequence(rows, shift):
    return BR.moving_sequence(rows, shift, frames=5, seed=rows + 1)


@pytest.mark.parametrize("shift", [(3, 0), (37, 2), (-90, 5)], ids=str)
@pytest.mark.parametrize("rows", [5, 64, 320])
def test_moving_sequences(ore, rows, shift):
    """Five frames of track_ref.sequence moved as a whole: the shift, then the "track v1" update, frame after frame."""
    kw = dict(bin=2, half_bins=64, score_thresh=SCORE, frame_h=400, frame_w=400)
    state, belt, votes, accepted = None, None, 0, []
    for b, s, c, n in sequence(rows, shift):
        state, belt, nv = both(ore, state, belt, (b, s, c, n), **kw)
        accepted.append((belt["dx"], belt["dy"], belt["votes"]))
        votes += nv
        _, state = ore.track_host(state, b, s, c, n, capacity=1024, score_thresh=SCORE)
    assert votes > 0 and belt["frames"] == 5 and belt["coasted"] >= 1          # the first frame has no tracks
    if rows >= 64:                                              # enough true pairs: the planted shift is found, to the bin
        assert all(abs(dx - shift[0]) <= 3 and abs(dy - shift[1]) <= 3 and v >= 3 for dx, dy, v in accepted[1:]), accepted
    print(f"rows {rows} shift {shift}: {accepted}, {votes} votes")


def lone(x, y, size=40.0):
    return [x, y, x + size, y + size]


def test_two_equal_peaks_settled_by_the_previous_shift(ore):
    """Two tracks 200 px apart (beyond the window), one row 10 px right of the first, one 10 px left of the second: two peaks of one
    vote, smoothed to two 3 x 3 blocks of S = 1.  The bin nearest the previous shift wins."""
    tracks = BR.tracks_of([lone(100, 100), lone(300, 100)])
    rows = BR.rows_of([lone(110, 100), lone(290, 100)])
    kw = dict(bin=2, half_bins=64, min_votes=1)
    for prev, want in (((8, 0), (8, 0)), ((-8, 0), (-8, 0)), ((12, 2), (12, 2)), ((40, 0), (12, 0)), ((-40, -9), (-12, -2))):
        belt = dict(BR.empty_belt(), dx=prev[0], dy=prev[1])
        _, new, votes = both(ore, tracks, belt, rows, **kw)
        assert votes == 2 and (new["dx"], new["dy"], new["votes"]) == (want[0], want[1], 1), (prev, new)


def test_two_equal_peaks_at_equal_distance(ore):
    """The same two peaks with the previous shift in the middle: qy ascending, then qx ascending decides."""
    kw = dict(bin=2, half_bins=64, min_votes=1)
    tracks = BR.tracks_of([lone(100, 100), lone(300, 100)])
    _, new, _ = both(ore, tracks, None, BR.rows_of([lone(110, 100), lone(290, 100)]), **kw)
    assert (new["dx"], new["dy"]) == (-8, 0)                    # (-8, 0) and (8, 0) are 8 from (0, 0), both at qy = 0: the lower qx
    tracks = BR.tracks_of([lone(100, 100), lone(100, 300)])
    _, new, _ = both(ore, tracks, None, BR.rows_of([lone(100, 110), lone(100, 290)]), **kw)
    assert (new["dx"], new["dy"]) == (0, -8)                    # (0, -8) and (0, 8) are 8 from (0, 0): the lower qy


def test_min_votes_is_the_threshold(ore):
    """Three tracks beyond each other's window.  Two rows moved by (10, 0): a peak of 2 = min_votes - 1 coasts at the previous shift;
    three rows: accepted.  The three votes share one bin, so the smoothed peak is a 3 x 3 block of equal S, and of those the bin nearest
    the previous shift is taken."""
    tracks = BR.tracks_of([lone(100, 100), lone(400, 100), lone(700, 100)])
    moved = [lone(110, 100), lone(410, 100), lone(710, 100)]
    prev = dict(BR.empty_belt(), dx=6, dy=-4, travel_x=60, travel_y=-40, frames=10, coasted=2)
    kw = dict(bin=2, half_bins=64, min_votes=3)
    st, new, votes = both(ore, tracks, prev, BR.rows_of(moved[:2]), **kw)
    assert votes == 2 and new == dict(prev, votes=0, coasted=3, frames=11, travel_x=66, travel_y=-44)
    assert np.array_equal(st["boxes"], tracks["boxes"] + np.array([6, -4, 6, -4], np.float32))   # the belt keeps running
    st, new, votes = both(ore, tracks, prev, BR.rows_of(moved), **kw)
    assert votes == 3 and new == dict(prev, dx=8, dy=-2, votes=3, frames=11, travel_x=68, travel_y=-42)
    assert np.array_equal(st["boxes"], tracks["boxes"] + np.array([8, -2, 8, -2], np.float32))
    st, new, votes = both(ore, tracks, dict(prev, dx=10, dy=0), BR.rows_of(moved), **kw)
    assert (new["dx"], new["dy"], new["votes"]) == (10, 0, 3)


def test_last_bin_and_beyond(ore):
    """bin 16, K = 5: a shift of exactly K * bin = 80 falls into the last bin (a belt already running at it stays there; from rest the
    smoothed tie resolves one bin nearer to 0), one of K * bin + bin = 96 outside: the frame coasts."""
    tracks = BR.tracks_of([lone(100, 100), lone(400, 100), lone(700, 100)])
    kw = dict(bin=16, half_bins=5, min_votes=3)
    for shift, want in (((80, 0), (80, 0, 3, 0)), ((0, -80), (0, -80, 3, 0)), ((-80, 80), (-80, 80, 3, 0)), ((96, 0), (96, 0, 0, 1)), ((0, -96), (0, -96, 0, 1))):
        rows = BR.rows_of(tracks["boxes"] + np.array([shift[0], shift[1]] * 2, np.float32))
        _, new, votes = both(ore, tracks, dict(BR.empty_belt(), dx=shift[0], dy=shift[1]), rows, **kw)
        assert (new["dx"], new["dy"], new["votes"], new["coasted"]) == want and votes == want[2], (shift, new)
        _, new, votes = both(ore, tracks, None, rows, **kw)
        rest = (shift[0] * 4 // 5, shift[1] * 4 // 5, 3, 0) if want[2] else (0, 0, 0, 1)
        assert (new["dx"], new["dy"], new["votes"], new["coasted"]) == rest and votes == want[2], (shift, new)


def test_size_gate_at_equality_and_one_ulp_beyond(ore):
    """size_tol 1 / 8 and a track 64 wide: a row 56 wide is at the gate exactly (8 <= 0.125 * 64, the product is exact) and votes; a row
    one ulp narrower than 56 does not.  The same for the height."""
    kw = dict(bin=2, half_bins=64, min_votes=1, size_tol=0.125)
    tracks = BR.tracks_of([[0, 0, 64, 64]])
    under = np.nextafter(np.float32(56), np.float32(0))
    for box, want in (([0, 0, 56, 64], 1), ([0, 0, under, 64], 0), ([0, 0, 64, 56], 1), ([0, 0, 64, under], 0), ([0, 0, 56, 56], 1)):
        _, new, votes = both(ore, tracks, None, BR.rows_of([box]), **kw)
        assert votes == want and new["votes"] == want and new["coasted"] == 1 - want, (box, new)
    # a larger row: the product is taken with the larger extent, the row's
    tracks = BR.tracks_of([[0, 0, 56, 56]])
    over = np.nextafter(np.float32(64), np.float32(100))
    for box, want in (([0, 0, 64, 64], 1), ([0, 0, over, 64], 0)):
        assert both(ore, tracks, None, BR.rows_of([box]), **kw)[2] == want


def test_class_aware_on_and_off(ore):
    """A row of another class votes only with class_aware off; a sequence with and without its classes."""
    tracks = BR.tracks_of([lone(100, 100), lone(400, 100)], classes=[1, 2])
    rows = BR.rows_of([lone(110, 100), lone(410, 100)], classes=[1, 3])
    assert both(ore, tracks, None, rows, min_votes=1, class_aware=True)[2] == 1
    assert both(ore, tracks, None, rows, min_votes=1, class_aware=False)[2] == 2
    counts = []
    for aware in (True, False):
        state, belt, total = None, None, 0
        for b, s, c, n in sequence(64, (37, 2)):
            state, belt, nv = both(ore, state, belt, (b, s, c, n), score_thresh=SCORE, class_aware=aware)
            total += nv
            _, state = ore.track_host(state, b, s, c, n, score_thresh=SCORE, class_aware=aware)
        counts.append(total)
    assert counts[1] > counts[0] > 0


def test_no_tracks_and_no_rows(ore):
    """m = 0, n = 0, and zero rows: no votes, the belt coasts at its shift and the tracks still move with it."""
    b, s, c, n = sequence(64, (37, 2))[1]
    prev = dict(BR.empty_belt(), dx=36, dy=2, votes=20, frames=4, travel_x=100, travel_y=8)
    _, new, votes = both(ore, None, prev, (b, s, c, n))
    assert votes == 0 and new == dict(prev, votes=0, coasted=1, frames=5, travel_x=136, travel_y=10)
    _, state = ore.track_host(None, b, s, c, n)
    for rows in ((b, s, c, 0), (b[:0], s[:0], c[:0], 0), (b, s, c, -2)):
        st, new, votes = both(ore, state, prev, rows)
        assert votes == 0 and new["coasted"] == 1 and (new["dx"], new["dy"]) == (36, 2)
        assert np.array_equal(st["boxes"], state["boxes"] + np.array([36, 2, 36, 2], np.float32))
    st, new, _ = both(ore, None, None, (b[:0], s[:0], None, None))
    assert st["m"] == 0 and new == dict(BR.empty_belt(), coasted=1, frames=1)


def test_track_pushed_out_of_the_frame(ore):
    """Frame 200 x 200, the belt moves 20 px right.  Track 3 has no row and its moved box lies outside: ttl 1, gone after the update.
    Track 4's moved box lies outside too, but a row continues it: it stays.  Track 5, missed and still inside, ages by one."""
    kw = dict(bin=2, half_bins=64, min_votes=3, frame_h=200, frame_w=200)
    old = [lone(10, 10, 30.0), lone(60, 60, 30.0), lone(110, 110, 30.0), lone(185, 20, 30.0), lone(181, 150, 30.0), lone(120, 20, 30.0)]
    tracks = BR.tracks_of(old, ttl=5)
    rows = BR.rows_of([lone(30, 10, 30.0), lone(80, 60, 30.0), lone(130, 110, 30.0), lone(201, 150, 30.0)])
    st, new, votes = both(ore, tracks, dict(BR.empty_belt(), dx=20), rows, **kw)
    assert (new["dx"], new["dy"], new["votes"]) == (20, 0, 4) and votes > 4    # in a 200 px frame false pairs vote too, each alone in its bin
    assert st["ttl"].tolist() == [5, 5, 5, 1, 1, 5] and st["ids"].tolist() == [0, 1, 2, 3, 4, 5]
    ids, after = ore.track_host(st, *rows)
    assert ids.tolist() == [0, 1, 2, 4] and after["ids"].tolist() == [0, 1, 2, 4, 5] and after["ttl"].tolist() == [8, 8, 8, 8, 4]
    # the edge itself: x0 == frame_w is outside, one ulp less is inside; a NaN box compares false and stays
    edge = BR.tracks_of([[180, 0, 190, 10], [np.nextafter(np.float32(180), np.float32(0)), 0, 190, 10], [np.nan, 0, 190, 10], [-30, 0, -20, 10],
                         [0, 200, 10, 210], [0, -30, 10, -20]], ttl=5)
    st, new, _ = both(ore, edge, dict(BR.empty_belt(), dx=20), BR.rows_of(np.zeros((0, 4))), **kw)
    assert st["ttl"].tolist() == [1, 5, 5, 1, 1, 1]
    st, _, _ = both(ore, edge, dict(BR.empty_belt(), dx=20), BR.rows_of(np.zeros((0, 4))), bin=2, half_bins=64)
    assert st["ttl"].tolist() == [5] * 6                       # no frame, no test


def test_refused_parameters(ore):
    b, s, c, n = BR.rows_of([lone(0, 0)])
    for bad in (dict(bin=3), dict(bin=32), dict(bin=True), dict(half_bins=0), dict(half_bins=65), dict(size_tol=1.0), dict(size_tol=-0.1),
                dict(size_tol=float("nan")), dict(min_votes=0), dict(min_votes=(1 << 30) + 1), dict(frame_h=10), dict(frame_w=-1, frame_h=-1),
                dict(score_thresh=float("nan"))):
        with pytest.raises(ore.OreError):
            ore.belt_shift_host(None, None, b, s, c, n, **bad)
    for bad in (dict(radius=130), dict(radius=0), dict(bin=16, radius=1025), dict(frame=(0, 10)), dict(frame=5), dict(bin=5)):
        with pytest.raises(ore.OreError):
            ore.BeltTracker("cpu", **bad)
    tr = ore.BeltTracker("cpu")
    tr.update(b, s, c, n)
    before = tr.state_host()
    with pytest.raises(ore.OreError, match="321"):             # refused before the shift: neither state has moved
        tr.update(np.zeros((321, 4), np.float32), np.zeros(321, np.float32))
    after = tr.state_host()
    assert after["belt"] == before["belt"] and BR.same_tracks(after, before)
    assert ore.BeltTracker("cpu", bin=16, radius=1024).belt_params["half_bins"] == 64
    assert ore.BeltTracker("cpu", radius=127).belt_params["half_bins"] == 64 and ore.BeltTracker("cpu").belt_params["bin"] == 2


# ------------------------------------------------------------------------------------------ the property
@functools.lru_cache(maxsize=None)
def planted(objs):
    return BR.belt_sequence(objs, shift=(37, 2), frames=8, seed=objs)


@pytest.mark.parametrize("objs", [30, 400])
def test_ids_persist_on_the_planted_belt(ore, objs):
    """30 and 400 boxes of 20 .. 70 px on 1080 x 1920 moving (37, 2) px per frame, +-1 px of jitter, 5 % misses, 8 frames, bin 2.  With the
    shift in front every object seen in two consecutive frames keeps its id; "track v1" alone keeps none.  (400 rows are beyond the
    one-workgroup tracker's 320: the wide classes take them; 30 rows go through both.)"""
    frames = planted(objs)
    kinds = [(ore.WideBeltTracker, ore.WideBoxTracker)] + ([(ore.BeltTracker, ore.BoxTracker)] if objs <= 320 else [])
    for belt_cls, plain_cls in kinds:
        belt, plain = belt_cls("cpu", bin=2, frame=(1080, 1920)), plain_cls("cpu")
        assert isinstance(belt, ore.BoxTracker) and isinstance(belt, plain_cls)
        ids_belt = [belt.update(b, s, c, n).numpy() for b, s, c, n, _ in frames]
        ids_plain = [plain.update(b, s, c, n).numpy() for b, s, c, n, _ in frames]
        kept, total = BR.kept_ids(frames, ids_belt)
        assert total > 6 * objs and kept == total, (kept, total)
        assert BR.kept_ids(frames, ids_plain) == (0, total)
        stats, st = belt.stats(), belt.state_host()
        assert stats["started"] < 1.1 * objs and plain.stats()["started"] > 6 * objs     # particles, not detections
        assert abs(stats["shift"][0] - 37) <= 1 and abs(stats["shift"][1] - 2) <= 1 and stats["votes"] > 0.7 * objs and stats["coasted"] == 1
        assert abs(stats["travel"][0] - 7 * 37) <= 7 and abs(stats["travel"][1] - 7 * 2) <= 7
        assert st["belt"]["frames"] == 8 == st["frames"] and st["belt"]["dx"] == stats["shift"][0]
        # the trackers are the composition of the two host statements
        state, b_state = None, None
        for (b, s, c, n, _), want in zip(frames, ids_belt):
            state, b_state = ore.belt_shift_host(state, b_state, b, s, c, n, bin=2, half_bins=64, frame_h=1080, frame_w=1920)
            ids, state = ore.track_host(state, b, s, c, n, wide=True, capacity=belt.capacity)
            assert np.array_equal(ids, want)
        assert BR.same_belt(b_state, st["belt"]) and BR.same_tracks(st, state)
        belt.reset()
        assert belt.stats() == {"tracks": 0, "started": 0, "frames": 0, "dropped": 0, "shift": (0, 0), "travel": (0, 0), "votes": 0, "coasted": 0}


def test_instances_form_and_out(ore):
    """update(Instances) and out= go through the shift like the tensor form."""
    import torch
    from detectron2.structures import Boxes, Instances
    frames = planted(30)
    a, b_ = ore.BeltTracker("cpu"), ore.BeltTracker("cpu")
    for b, s, c, n, _ in frames[:3]:
        inst = Instances((1080, 1920))
        inst.pred_boxes, inst.scores, inst.pred_classes = Boxes(torch.from_numpy(b)), torch.from_numpy(s), torch.from_numpy(c)
        out = torch.empty(len(s), dtype=torch.int64)
        got = a.update(inst, out=out)
        assert got is out and torch.equal(inst.track_ids, out) and torch.equal(out, b_.update(b, s, c, n))
    assert a.stats() == b_.stats() and a.stats()["shift"] != (0, 0)


# ------------------------------------------------------------------------------------------ the surfaces
def test_surfaces_exist(ore):
    """The C entry points, their refusals (ORE_EINVAL comes before any launch, so the addresses are never read), the classes and the
    demo's flags."""
    import inspect
    import demo
    from predictor import VisualizationDemo
    L = ore.lib()
    for name in ("ore_belt_state_bytes", "ore_belt_reset", "ore_belt_workspace_bytes", "ore_belt_shift_form", "ore_belt_shift_fwd"):
        assert name in ore.SYMBOLS and hasattr(L, name), name
    assert L.ore_belt_state_bytes() == 64 and ore.BELT_MAX_HALF_BINS == 64
    assert L.ore_belt_workspace_bytes(16384, 8192, 64) == (129 * 129 * 4 + 255) // 256 * 256 and L.ore_belt_workspace_bytes(1024, 320, 5) == 512
    assert L.ore_belt_workspace_bytes(16385, 8192, 64) == 0 and L.ore_belt_workspace_bytes(16, 8193, 64) == 0 and L.ore_belt_workspace_bytes(16, 8, 65) == 0
    assert [L.ore_belt_shift_form(*a) for a in ((1024, 320, 64), (1025, 320, 1), (1, 321, 64), (16384, 8192, 64))] == [1, 2, 2, 2]
    assert L.ore_belt_shift_form(0, 8, 8) == -22 and L.ore_belt_shift_form(16, 8, 0) == -22 and L.ore_belt_reset(None, None) == -22
    belt, st, rows, ws = 0x10000, 0x20000, 0x80000, 0x100000
    ok = dict(belt=belt, state=st, capacity=16, n_host=8, max_rows=8, score=0.0, bin=2, K=64, tol=0.125, votes=3, fh=0, fw=0, form=0, ws=ws, wsb=1 << 20)
    for bad in (dict(bin=3), dict(bin=-2), dict(K=65), dict(K=0), dict(tol=1.0), dict(tol=float("inf")), dict(votes=0), dict(fh=5), dict(fw=5), dict(fh=-1, fw=-1),
                dict(form=1, capacity=1025), dict(form=1, max_rows=321), dict(form=2, wsb=1024), dict(form=2, ws=0), dict(form=2, ws=ws + 8), dict(form=5),
                dict(belt=0), dict(belt=belt + 4), dict(belt=st + 32), dict(state=rows), dict(belt=rows + 0x1000), dict(form=2, ws=st), dict(n_host=-1),
                dict(capacity=0), dict(capacity=16385), dict(max_rows=8193), dict(score=float("nan"))):
        a = dict(ok, **bad)
        rc = L.ore_belt_shift_fwd(a["belt"], a["state"], a["capacity"], rows, rows + 0x1000, rows + 0x2000, None, a["n_host"], a["max_rows"], a["score"], 1,
                                  a["bin"], a["K"], a["tol"], a["votes"], a["fh"], a["fw"], a["form"], a["ws"], a["wsb"], None)
        assert rc == -22 and L.ore_last_error().startswith(b"ore_belt_shift_fwd"), (bad, rc)
    for cls, base in ((ore.BeltTracker, ore.BoxTracker), (ore.WideBeltTracker, ore.WideBoxTracker)):
        assert issubclass(cls, base) and issubclass(cls, ore.BoxTracker)
        p = inspect.signature(cls.__init__).parameters
        assert {k: p[k].default for k in ("bin", "radius", "size_tol", "min_votes", "frame")} == ore.BELT_DEFAULTS
    p = inspect.signature(VisualizationDemo.__init__).parameters
    assert p["track"].default is False and p["belt"].default is None
    args = demo.get_parser().parse_args(["--track", "--track-motion", "belt", "--belt-radius", "96", "--belt-bin", "4", "--input", "a.png", "b.png"])
    assert (args.track_motion, args.belt_radius, args.belt_bin) == ("belt", 96, 4)
    plain = demo.get_parser().parse_args(["--track", "--input", "a.png", "b.png"])
    assert (plain.track_motion, plain.belt_radius, plain.belt_bin) == (None, None, None)
    for argv in (["--track-motion", "belt"], ["--track", "--belt-radius", "64"], ["--track", "--track-motion", "belt", "--belt-radius", "200"],
                 ["--track", "--track-motion", "belt", "--belt-radius", "0"]):
        with pytest.raises(SystemExit) as e:
            demo.main(argv + ["--input", "a.png", "b.png", "--output", "o"])
        assert "demo.py: --" in str(e.value), argv
