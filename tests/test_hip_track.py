"""GPU: the tracker kernel (csrc/ore_track.hip, association contract "track v1") against tests/track_ref.py -- ids and the whole state,
np.array_equal after every frame -- the overlay's track colouring against tests/overlay_track_ref.py byte for byte, and what is built
on both: BoxTracker across streams, AsyncPredictor.put(track=), VisualizationDemo(track=True).  The reference of a sequence is computed
once and shared by the ways it is run."""
import functools

import numpy as np
import pytest
import torch

import overlay_ref as OR
import overlay_track_ref as OTR
import track_ref as TR
from test_hip_overlay import BAND, guarded_draw
from test_hip_resize import RAW_SIZES, _cfg, _load, assert_same, fields, raw_image
from test_track_host import NAMES, SHAPES

pytestmark = pytest.mark.gpu
SCORE = 0.05                                                   # the score threshold of the sequences (track_ref.sequence plants 0.01s)


@pytest.fixture(scope="module")
def ore():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import orehip
    orehip.lib()
    return orehip


@functools.lru_cache(maxsize=None)
def reference(rows, capacity, classes=True):
    """(frames, [(ids, state arrays) per frame]) of one generated sequence."""
    frames = [(b, s, c if classes else None, n) for b, s, c, n in TR.sequence(rows, seed=rows)]
    st, out = TR.empty_state(), []
    for b, s, c, n in frames:
        ids, st = TR.update_ref(st, b, s, c, n, capacity=capacity, score_thresh=SCORE)
        out.append((ids, st))
    return frames, out


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check_frames(ore_, tracker, frames, want, count="dev", who=""):
    """Every frame through `tracker`; ids (all rows, the -1s included) and the whole state equal the reference's after each."""
    for f, ((b, s, c, n), (ids_w, st_w)) in enumerate(zip(frames, want)):
        n_arg = torch.tensor([n], dtype=torch.int32, device="cuda") if count == "dev" else n
        ids = tracker.update(dev(b), dev(s), dev(c), n_arg)
        assert ids.dtype == torch.int64 and ids.shape == (len(s),)
        got = ids.cpu().numpy()
        assert np.array_equal(got, ids_w), (who, f, np.nonzero(got != ids_w)[0][:8], got[:8], ids_w[:8])
        assert TR.same_state(tracker.state_host(), st_w), (who, f)
        full = tracker.state()                               # the slots behind the list hold zeros
        torch.cuda.synchronize()
        m = int(full["m"].item())
        assert all(not t[m:].any().item() for t in (full["boxes"], full["classes"], full["ids"], full["ttl"])), (who, f)


@pytest.mark.parametrize("rows,capacity", SHAPES, ids=lambda v: str(v))
def test_update_equals_ref(ore, rows, capacity):
    """12 frames: boxes drift, rows drop out for 1 .. 9 frames (both sides of ttl = 8), new rows appear, dead rows in between.  Four
    ways: the count on the device, the count on the host, no classes, on a non-default stream."""
    frames, want = reference(rows, capacity)
    kw = dict(capacity=capacity, score_thresh=SCORE)
    check_frames(ore, ore.BoxTracker("cuda", **kw), frames, want, "dev", "n_dev")
    check_frames(ore, ore.BoxTracker("cuda", **kw), frames, want, "host", "n_host")
    frames0, want0 = reference(rows, capacity, classes=False)
    check_frames(ore, ore.BoxTracker("cuda", **kw), frames0, want0, "dev", "classes=None")
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        check_frames(ore, ore.BoxTracker("cuda", **kw), frames, want, "dev", "side stream")
    last = want[-1][1]
    print(f"rows {rows} capacity {capacity}: {last['next_id']} ids started, {len(last['tracks'])} tracks, {last['dropped']} dropped, "
          f"{sum(st_['n_pairs'] for _, st_ in want)} candidate pairs in 12 frames")


def run_case(ore_, frames, **kw):
    """Frames through a fresh BoxTracker and the reference, equality after each; returns the reference states."""
    ref, out = TR.empty_state(), []
    for b, s, c, n in frames:
        ids_w, ref = TR.update_ref(ref, b, s, c, n, **kw)
        out.append((ids_w, ref))
    check_frames(ore_, ore_.BoxTracker("cuda", **kw), frames, out, "dev")
    check_frames(ore_, ore_.BoxTracker("cuda", **kw), frames, out, "host")
    return out


def test_ties(ore):
    """Duplicate boxes among the rows and among the tracks: many pairs of exactly equal IoU, IoU = 1 included.  The tie order (slot
    ascending, then row ascending) decides, and the result is the reference's."""
    out = run_case(ore, TR.ties_case())
    print("ties: candidate pairs per frame", [st["n_pairs"] for _, st in out])
    assert out[1][1]["n_pairs"] >= 20 and out[2][1]["n_pairs"] >= 40


def test_chain(ore):
    """40 tracks and 40 rows on a line whose accepted pairs free one another one by one: a mutual-best matching needs 40 rounds."""
    frames = TR.chain_case(40)
    rounds = TR.mutual_best_rounds(frames[0][0], frames[1][0], TR.CHAIN_IOU_THRESH)
    out = run_case(ore, frames, iou_thresh=TR.CHAIN_IOU_THRESH)
    print(f"chain: {out[1][1]['n_pairs']} candidate pairs, {rounds} mutual-best rounds")
    assert rounds >= 10 and np.array_equal(out[1][0], np.arange(40))


def test_thresholds_and_bad_rows(ore):
    """NaN and +-inf in any coordinate or in the score; a score exactly at score_thresh (live); an IoU exactly at iou_thresh (no
    candidate) and one just above; class mismatch with class_aware on and off."""
    base = np.array([[0, 0, 4, 1], [10, 10, 30, 40], [50, 5, 80, 25], [100, 100, 140, 160]], np.float32)
    ones = np.full(4, 0.5, np.float32)
    f0 = (base, ones, np.array([0, 1, 2, 3]), 4)
    rows, scores = [], []
    for k in range(4):                                       # every coordinate, every kind of non-finite value
        for bad in (np.nan, np.inf, -np.inf):
            r = base[1].copy()
            r[k] = bad
            rows.append(r)
            scores.append(0.5)
    for bad in (np.nan, np.inf, -np.inf):
        rows.append(base[2].copy())
        scores.append(bad)
    rows += [np.array([1, 0, 5, 1], np.float32), base[1] + np.float32(1), base[2], base[3]]       # inter 3 / union 5 against track 0
    scores += [0.5, 0.25, np.nextafter(np.float32(0.25), np.float32(0)), 0.5]                    # at the threshold; just below it
    b1, s1 = np.array(rows, np.float32), np.array(scores, np.float32)
    c1 = np.array([1] * 12 + [2] * 3 + [0, 1, 2, 7], np.int64)                                     # the last row: another class than track 3
    f1 = (b1, s1, c1, len(s1))
    f2 = (np.array([[0.5, 0, 4.5, 1]], np.float32), np.full(1, 0.5, np.float32), np.array([0]), 1)   # 3.5 / 4.5 against the row at x = 1 .. 5
    assert TR.iou_ref(base[0], b1[15]) == np.float32(0.6)
    for aware in (True, False):
        out = run_case(ore, [f0, f1, f2], iou_thresh=np.float32(0.6), score_thresh=0.25, class_aware=aware)
        ids1 = out[1][0]
        assert (ids1[:15] == -1).all() and ids1[17] == -1                # bad rows, and the score below the threshold
        assert ids1[15] == 4 and ids1[16] == 1                           # IoU == thresh: a new id; the score at the threshold continues track 1
        assert ids1[18] == (4 + 1 if aware else 3)                       # the class mismatch
        assert out[2][0][0] == 4                                         # just above the threshold


def test_overflow(ore):
    """capacity 8, max_rows 8, ttl 8: the survivors exceed the capacity; the cut, `dropped` and the ids are the reference's."""
    rng = np.random.default_rng(1)
    frames = []
    for f in range(6):                                       # every frame 5 .. 8 boxes at fresh places, plus the first two of the frame before
        k = 5 + f % 4
        x0, y0 = rng.uniform(0, 2000, k), rng.uniform(0, 2000, k)
        b = np.stack([x0, y0, x0 + 30, y0 + 30], 1).astype(np.float32)
        if frames:
            b[:2] = frames[-1][0][:2] + np.float32(1)
        full = np.zeros((8, 4), np.float32)
        full[:k] = b
        frames.append((full, np.full(8, 0.9, np.float32), np.zeros(8, np.int64), k))
    out = run_case(ore, frames, capacity=8, ttl=8)
    print("overflow: dropped", out[-1][1]["dropped"], "ids started", out[-1][1]["next_id"])
    assert out[-1][1]["dropped"] >= 10 and all(len(st["tracks"]) <= 8 for _, st in out)
    out = run_case(ore, frames, capacity=3, ttl=8)           # capacity below the live rows: rows themselves are cut, their ids still issued
    assert (out[0][0][:5] >= 0).all() and len(out[0][1]["tracks"]) == 3


class Guarded:
    """The C-ABI on a state buffer and an ids buffer that sit between 4096-byte bands of 0xA5."""

    def __init__(self, ore_, capacity, rows):
        self.L, self.capacity, self.rows = ore_.lib(), capacity, rows
        self.sb = int(self.L.ore_track_state_bytes(capacity))
        assert self.sb == (32 + 36 * capacity + 15) // 16 * 16
        self.buf = torch.full((BAND + self.sb + BAND + rows * 8 + BAND,), 0xA5, dtype=torch.uint8, device="cuda")
        self.state = self.buf[BAND:BAND + self.sb]
        self.ids = self.buf[2 * BAND + self.sb:2 * BAND + self.sb + rows * 8]
        assert self.L.ore_track_reset(self.state.data_ptr(), capacity, None) == 0

    def update(self, b, s, c, n_dev, n_host, max_rows=None, state=None, ids=None, capacity=None, score_thresh=0.0, iou_thresh=0.6, ttl=8,
               class_aware=1):
        p = lambda t: None if t is None else t.data_ptr()
        return self.L.ore_track_update_fwd(p(self.state) if state is None else state, self.capacity if capacity is None else capacity, p(b), p(s),
                                           p(c), p(n_dev), n_host, self.rows if max_rows is None else max_rows, score_thresh, iou_thresh, ttl,
                                           class_aware, p(self.ids) if ids is None else ids, None, 0, None)

    def bands_intact(self):
        h = self.buf.cpu().numpy()
        a, b_ = BAND + self.sb, 2 * BAND + self.sb + self.rows * 8
        return (h[:BAND] == 0xA5).all() and (h[a:a + BAND] == 0xA5).all() and (h[b_:] == 0xA5).all()

    def host(self):
        h = self.buf.cpu().numpy()
        return h[BAND:BAND + self.sb].copy(), h[2 * BAND + self.sb:2 * BAND + self.sb + self.rows * 8].view(np.int64).copy()


@pytest.mark.parametrize("rows,capacity", [(5, 8), (65, 130), (320, 1024), (320, 7)], ids=lambda v: str(v))
def test_guard_bands(ore, rows, capacity):
    """The state and the ids between guard bands: the bands are intact after every update, the input rows unchanged, the ids the
    reference's."""
    frames = TR.sequence(rows, frames=4, seed=rows + 1)
    g = Guarded(ore, capacity, rows)
    assert g.bands_intact()
    ref = TR.empty_state()
    for b, s, c, n in frames:
        db, ds, dc = dev(b), dev(s), dev(c)
        assert g.update(db, ds, dc, None, n, score_thresh=SCORE) == 0
        torch.cuda.synchronize()
        assert g.bands_intact()
        assert np.array_equal(db.cpu().numpy(), b, equal_nan=True) and np.array_equal(ds.cpu().numpy(), s, equal_nan=True)
        assert np.array_equal(dc.cpu().numpy(), c)
        want, ref = TR.update_ref(ref, b, s, c, n, capacity=capacity, score_thresh=SCORE)
        assert np.array_equal(g.host()[1], want)


def test_limits_are_einval_before_any_launch(ore):
    """Every limit of the header is refused with ORE_EINVAL and a message, and nothing is launched: the guarded state and the ids are
    byte for byte what they were."""
    rows, cap = 8, 16
    g = Guarded(ore, cap, rows)
    b, s, c, _ = TR.sequence(rows, frames=1, seed=2)[0]
    db, ds, dc = dev(b), dev(s), dev(c)
    assert g.update(db, ds, dc, None, rows) == 0
    torch.cuda.synchronize()
    state0, ids0 = g.host()
    sp, ip = g.state.data_ptr(), g.ids.data_ptr()
    EINVAL = -22                                               # ORE_EINVAL
    bad = [dict(capacity=0), dict(capacity=1025), dict(max_rows=-1), dict(max_rows=321), dict(ttl=0), dict(ttl=(1 << 20) + 1),
           dict(iou_thresh=-0.5), dict(iou_thresh=float("nan")), dict(iou_thresh=float("inf")), dict(score_thresh=float("nan")),
           dict(state=0), dict(state=sp + 4), dict(ids=0),
           dict(ids=sp), dict(ids=sp + g.sb - 8),                            # ids inside the state
           dict(state=db.data_ptr()), dict(ids=db.data_ptr()), dict(ids=ds.data_ptr()), dict(ids=dc.data_ptr())]       # on the row arrays
    for kw in bad:
        rc = g.update(db, ds, dc, None, rows, **kw)
        assert rc == EINVAL, (kw, rc)
        assert g.L.ore_last_error().startswith(b"ore_track_update_fwd"), kw
    assert g.update(db, ds, dc, None, -1) == EINVAL                            # a negative host count without a device count
    assert g.update(None, ds, dc, None, rows) == EINVAL and g.update(db, None, dc, None, rows) == EINVAL
    assert g.L.ore_track_reset(sp, 0, None) == EINVAL and g.L.ore_track_reset(sp, 1025, None) == EINVAL and g.L.ore_track_reset(None, cap, None) == EINVAL
    torch.cuda.synchronize()
    state1, ids1 = g.host()
    assert np.array_equal(state0, state1) and np.array_equal(ids0, ids1) and g.bands_intact()
    assert np.array_equal(db.cpu().numpy(), b, equal_nan=True)
    for kw in (dict(capacity=0), dict(ttl=0), dict(iou_thresh=float("nan"))):
        with pytest.raises(ore.OreError):
            ore.BoxTracker("cuda", **kw)
    tr = ore.BoxTracker("cuda")
    with pytest.raises(ore.OreError, match="rows"):
        tr.update(torch.zeros(321, 4, device="cuda"), torch.zeros(321, device="cuda"))
    with pytest.raises(ore.OreError, match="n_dev"):
        tr.update(db, ds, dc, torch.tensor([1], dtype=torch.int64, device="cuda"))
    with pytest.raises(ore.OreError):
        tr.update(db.cpu(), ds.cpu())
    assert tr.stats() == {"tracks": 0, "started": 0, "frames": 0, "dropped": 0}


def test_one_tracker_across_streams_and_instances(ore):
    """Consecutive frames on four streams in turn, nothing synchronised in between: the tracker orders its updates on the device, the
    ids are the reference's.  Then an Instances: track_ids is set."""
    from detectron2.structures import Boxes, Instances
    frames, want = reference(65, 130)
    tr = ore.BoxTracker("cuda", capacity=130, score_thresh=SCORE)
    streams = [torch.cuda.Stream() for _ in range(4)]
    rows = [(dev(b), dev(s), dev(c), torch.tensor([n], dtype=torch.int32, device="cuda")) for b, s, c, n in frames]
    torch.cuda.synchronize()
    got = []
    for f, r in enumerate(rows):
        with torch.cuda.stream(streams[f % 4]):
            got.append(tr.update(*r))
    torch.cuda.synchronize()
    for f, ids in enumerate(got):
        assert np.array_equal(ids.cpu().numpy(), want[f][0]), f
    assert TR.same_state(tr.state_host(), want[-1][1])
    assert tr.stats()["started"] == want[-1][1]["next_id"] and tr.stats()["frames"] == 12
    tr.reset()
    b, s, c, _ = frames[0]
    keep = np.isfinite(b).all(1) & np.isfinite(s)
    inst = Instances((400, 400))
    inst.pred_boxes, inst.scores, inst.pred_classes = Boxes(dev(b[keep])), dev(s[keep]), dev(c[keep])
    ids = tr.update(inst)
    assert inst.track_ids is ids and ids.is_cuda
    assert np.array_equal(ids.cpu().numpy(), TR.update_ref(TR.empty_state(), b[keep], s[keep], c[keep], score_thresh=SCORE)[0])


# ------------------------------------------------------------------------------------------ the overlay, coloured by track
def guarded_draw_ids(ore_, img, b, s, c, ids, n_dev=None, inplace=False, **kw):
    return guarded_draw(ore_, img, b, s, c, n_dev, inplace, ids=torch.from_numpy(np.array(ids)).cuda(), color_by="track", **kw)


@pytest.mark.parametrize("hw", [(75, 100), (480, 640)], ids=lambda v: "%dx%d" % v)
def test_overlay_with_ids_equals_ref(ore, hw):
    """Some ids -1, ids beyond the palette, a 19-digit id in front of a 32-byte name (the cut at 40 characters); out of place and in
    place; with the count on the device.  color_by 0 / 1 through the ids entry give the bytes of the old entry."""
    h, w = hw
    L, S = {(75, 100): (1, 1), (480, 640): (3, 2)}[hw]
    img = np.random.default_rng(h + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    b, s, c = OR.cases(h, w, seed=h + w, rows=28)
    c[1] = 1
    ids = OTR.track_ids_for(28, seed=h)
    kw = dict(score_thresh=0.01, line_width=L, text_scale=S, names=NAMES, palette=ore.OVERLAY_PALETTE)
    want = OTR.overlay_track_ref(img, b, s, c, ids, atlas=ore.overlay_atlas(), **kw)
    assert (want != img).any()
    for inplace in (False, True):
        got = guarded_draw_ids(ore, img, b, s, c, ids, inplace=inplace, **kw)
        print(f"{h}x{w} inplace={inplace}: {int((got != want).sum())} differing bytes, {int((want != img).any(2).sum())} pixels drawn")
        assert np.array_equal(got, want)
    assert np.array_equal(got, ore.overlay_host(img, b, s, c, ids=ids, color_by="track", **kw))
    n_dev = torch.tensor([17], dtype=torch.int32, device="cuda")
    assert np.array_equal(guarded_draw_ids(ore, img, b, s, c, ids, n_dev, **kw), OTR.overlay_track_ref(img, b, s, c, ids, 17, atlas=ore.overlay_atlas(), **kw))
    assert np.array_equal(guarded_draw_ids(ore, img, b, s, None, ids, **dict(kw, names=None)),
                          OTR.overlay_track_ref(img, b, s, None, ids, atlas=ore.overlay_atlas(), **dict(kw, names=None)))
    for by in ("instance", "class"):
        want_by = OR.overlay_ref(img, b, s, c, atlas=ore.overlay_atlas(), color_by=by, **kw)
        assert np.array_equal(guarded_draw(ore, img, b, s, c, ids=torch.from_numpy(ids).cuda(), color_by=by, **kw), want_by)
        assert np.array_equal(guarded_draw(ore, img, b, s, c, color_by=by, **kw), want_by)
    frame_d = torch.from_numpy(img).cuda()
    with pytest.raises(ore.OreError, match="ids"):
        ore.overlay_draw(frame_d, dev(b), dev(s), dev(c), color_by="track", **kw)
    with pytest.raises(ore.OreError, match="ids"):
        ore.overlay_draw(frame_d, dev(b), dev(s), dev(c), ids=torch.from_numpy(ids[:5]).cuda(), color_by="track", **kw)
    L_ = ore.lib()                                           # the C entry: color_by 2 without ids, a color_by outside 0 .. 2
    ws = torch.empty(int(L_.ore_overlay_workspace_bytes(28)), dtype=torch.uint8, device="cuda")
    pal = dev(ore.OVERLAY_PALETTE)
    for ids_p, by in ((None, 2), (dev(ids).data_ptr(), 3), (dev(ids).data_ptr(), -1)):
        rc = L_.ore_overlay_draw_ids_fwd(frame_d.data_ptr(), frame_d.data_ptr(), h, w, dev(b).data_ptr(), dev(s).data_ptr(), None, ids_p, None, 28, 28,
                                         0.0, 1, 0, 128, 204, pal.data_ptr(), 20, by, None, 0, None, ws.data_ptr(), ws.numel(), None)
        assert rc != 0 and L_.ore_last_error().startswith(b"ore_overlay_draw_ids_fwd")
    torch.cuda.synchronize()
    assert np.array_equal(frame_d.cpu().numpy(), img)


# ------------------------------------------------------------------------------------------ the predictors
def video_frames():
    """8 frames of two sizes: frames 0 .. 2 the same picture (every id persists), then two shifted copies, then another picture of
    the other size, a shifted copy of it, and it again."""
    p, q = raw_image(300, *RAW_SIZES[0]), raw_image(301, *RAW_SIZES[1])
    roll = lambda a, k: np.ascontiguousarray(np.roll(a, (k, 2 * k), axis=(0, 1)))
    return [p, p.copy(), p.copy(), roll(p, 2), roll(p, 4), q, roll(q, 3), q.copy()]


def track_cfg():
    """The synthetic detector with a threshold low enough that every frame has rows (as the overlay tests' frames do)."""
    return _cfg(["MODEL.ROI_HEADS.SCORE_THRESH_TEST", 0.0])


@pytest.fixture(scope="module")
def tracked_reference(ore):
    """DefaultPredictor one frame at a time, each followed by an update of one fresh BoxTracker: [(frame, result, ids tensor)]."""
    from detectron2.engine.defaults import DefaultPredictor
    p = DefaultPredictor(track_cfg())
    _load(p.model)
    tr = ore.BoxTracker(p.model.device)
    out = []
    for f in video_frames():
        res = p(f)
        out.append((f, res, tr.update(res["instances"]).clone()))
    return out


def ref_track_picture(ore_, bgr, res, ids, names):
    from detectron2.utils.visualizer import default_overlay_params
    _, boxes, scores, classes = fields(res)
    return ore_.overlay_host(bgr, boxes.cpu().numpy(), scores.cpu().numpy(), classes.cpu().numpy(), ids=ids, color_by="track",
                             palette=ore_.OVERLAY_PALETTE[:, ::-1], names=names, **default_overlay_params(*bgr.shape[:2]))


def test_async_predictor_tracks(ore, tracked_reference):
    """8 frames through put(frame, draw=True, track=tr) with 4 in flight: track_ids equal the one-frame-at-a-time tracker's and
    track_host's on the host copies of the rows; vis_image is overlay_host's picture with those ids (and the reference extension's);
    ids persist and new ones appear; nothing synchronises inside put."""
    from detectron2.utils.visualizer import default_overlay_params, thing_classes
    from predictor import AsyncPredictor
    ap = AsyncPredictor(track_cfg(), inflight=4)
    _load(ap.model)
    names = thing_classes(ap.metadata)
    tr = ore.BoxTracker(ap.model.device)
    got = []
    try:
        ap.put(tracked_reference[0][0], draw=True, track=ore.BoxTracker(ap.model.device))      # engines, graphs and tables exist
        ap.get()
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            for f, _, _ in tracked_reference[:4]:
                ap.put(f, draw=True, track=tr)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        for f, _, _ in tracked_reference[4:]:
            got.append(ap.get())
            ap.put(f, draw=True, track=tr)
        while len(ap):
            got.append(ap.get())
        with pytest.raises(ValueError, match="track"):
            ap.put(tracked_reference[0][0], track="yes")
        with pytest.raises(ValueError, match="track"):
            ap.put(tracked_reference[0][0], draw={"color_by": "track"})
        with pytest.raises(ValueError):
            ap.put(tracked_reference[0][0], draw={"line_width": 0}, track=tr)                   # refused on the host: the tracker is untouched
        assert len(ap) == 0 and tr.stats()["frames"] == 8
        # draw says otherwise: tracked, but coloured by class
        ap.put(tracked_reference[7][0], draw={"color_by": "class"}, track=ore.BoxTracker(ap.model.device))
        by_class = ap.get()
    finally:
        ap.shutdown()
    host_state, persisted, fresh, prev = None, 0, 0, set()
    for i, (g, (f, res, ids_w)) in enumerate(zip(got, tracked_reference)):
        assert_same(g, res)
        ids = g["instances"].track_ids
        assert ids.dtype == torch.int64 and torch.equal(ids, ids_w), i
        _, boxes, scores, classes = fields(res)
        ids_h, host_state = ore.track_host(host_state, boxes.cpu().numpy(), scores.cpu().numpy(), classes.cpu().numpy())
        assert np.array_equal(ids.cpu().numpy(), ids_h), i
        pic = ref_track_picture(ore, f, res, ids_h, names)
        assert (pic != f).any() and np.array_equal(g["vis_image"].cpu().numpy(), pic), i
        if i in (0, 5):
            want = OTR.overlay_track_ref(f, boxes.cpu().numpy(), scores.cpu().numpy(), classes.cpu().numpy(), ids_h, atlas=ore.overlay_atlas(),
                                         palette=ore.OVERLAY_PALETTE[:, ::-1], names=names, **default_overlay_params(*f.shape[:2]))
            assert np.array_equal(pic, want)
        now = set(ids_h[ids_h >= 0].tolist())
        persisted += len(now & prev)
        fresh += len([v for v in now if i > 0 and v >= first_next])
        if i == 0:
            first_next = host_state["next_id"]
            assert len(now) >= 1
        prev = now
    print(f"async tracking: {persisted} ids persisted across frame pairs, {fresh} row ids issued after frame 0, {host_state['next_id']} started")
    assert persisted >= 1 and fresh >= 1
    assert tr.stats()["started"] == host_state["next_id"]
    f, res, _ = tracked_reference[7]
    _, boxes, scores, classes = fields(res)
    assert np.array_equal(by_class["vis_image"].cpu().numpy(),
                          OR.overlay_ref(f, boxes.cpu().numpy(), scores.cpu().numpy(), classes.cpu().numpy(), atlas=ore.overlay_atlas(),
                                         palette=ore.OVERLAY_PALETTE[:, ::-1], names=names, color_by="class", **default_overlay_params(*f.shape[:2])))
    assert by_class["instances"].has("track_ids")


def test_run_on_video_with_tracking(ore, tracked_reference):
    """VisualizationDemo(track=True).run_on_video, serial and parallel: the same annotated frames, those of the reference ids; a
    second call starts again from id 0; track=False gives the frames of today's path (coloured by class)."""
    from detectron2.utils.visualizer import default_overlay_params, thing_classes
    from predictor import VisualizationDemo
    frames = [f for f, _, _ in tracked_reference]
    serial = VisualizationDemo(track_cfg(), parallel=False, track=True)
    _load(serial.predictor.model)
    par = VisualizationDemo(track_cfg(), parallel=True, track=True)
    _load(par.predictor.model)
    plain = VisualizationDemo(track_cfg(), parallel=False)
    _load(plain.predictor.model)
    names = thing_classes(serial.metadata)
    try:
        assert serial.track_stats() == {"tracks": 0, "started": 0, "frames": 0, "dropped": 0}
        a = list(serial.run_on_video(frames))
        b = list(par.run_on_video(iter(frames)))
        stats = serial.track_stats()
        assert stats == par.track_stats() and stats["frames"] == 8 and stats["started"] >= 1
        b2 = list(par.run_on_video(frames[:3]))              # again: the tracker starts from id 0
        a2 = list(serial.run_on_video(frames[:3]))
        assert par.track_stats()["frames"] == 3 == serial.track_stats()["frames"]
        c = list(plain.run_on_video(frames[:2]))
        _, vis = serial.run_on_image(frames[0])              # run_on_image ignores the tracker
        assert serial.track_stats()["frames"] == 3
    finally:
        par.predictor.shutdown()
    assert len(a) == len(b) == 8
    for i, (f, res, ids) in enumerate(tracked_reference):
        want = ref_track_picture(ore, f, res, ids.cpu().numpy(), names)
        assert np.array_equal(a[i], want) and np.array_equal(b[i], want), i
    for i in range(3):
        assert np.array_equal(a2[i], a[i]) and np.array_equal(b2[i], a[i]), i
    for i in range(2):
        f, res, _ = tracked_reference[i]
        _, boxes, scores, classes = fields(res)
        assert np.array_equal(c[i], OR.overlay_ref(f, boxes.cpu().numpy(), scores.cpu().numpy(), classes.cpu().numpy(), atlas=ore.overlay_atlas(),
                                                   palette=ore.OVERLAY_PALETTE[:, ::-1], names=names, color_by="class",
                                                   **default_overlay_params(*f.shape[:2])))
