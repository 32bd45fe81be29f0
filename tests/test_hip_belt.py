"""GPU: the belt's shift (csrc/ore_belt.hip: k_belt_one; k_belt_vote + k_belt_finish) computes the contract "belt shift v1" in front of
both trackers.  Every comparison is exact -- torch.equal on the ids and on every field of the track state and of the belt state after
each frame -- against the composition of the host statements orehip.belt_shift_host and orehip.track_host, against an analytic
expectation at the limits, and between the forms.  Then the memory the launch must not touch, the refusals, two streams, the wrappers,
and the property the shift exists for.  The expectation of a case is computed once and shared by the ways it is run."""
import functools

import numpy as np
import pytest
import torch

import belt_ref as BR
from test_hip_resize import _cfg, _load, raw_image

pytestmark = pytest.mark.gpu
SCORE = 0.05                                                   # track_ref.sequence plants scores of 0.01
FIELDS = ("boxes", "classes", "ids", "ttl")
BAND = 4096
EINVAL = -22


@pytest.fixture(scope="module")
def ore():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import orehip
    orehip.lib()
    return orehip


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def t_(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def same_state(got, want):
    """Two state_host() / track_host dicts: the four counters and torch.equal on every array (boxes as bits: a NaN equals itself)."""
    return all(int(got[k]) == int(want[k]) for k in ("m", "next_id", "frames", "dropped")) and \
        all(torch.equal(t_(got[k]).view(torch.int32) if k == "boxes" else t_(got[k]), t_(want[k]).view(torch.int32) if k == "boxes" else t_(want[k]))
            for k in FIELDS)


def contract_kw(tracker):
    return dict(tracker.belt_params, score_thresh=tracker.params["score_thresh"], class_aware=tracker.params["class_aware"])


def host_reference(ore_, frames, belt_kw, track_kw):
    """[(ids, state after the update, belt, state after the shift)] of the frames through belt_shift_host and track_host(wide=True)."""
    st, belt, out = None, None, []
    for b, s, c, n in frames:
        moved, belt = ore_.belt_shift_host(st, belt, b, s, c, n, **belt_kw)
        ids, st = ore_.track_host(moved, b, s, c, n, wide=True, **track_kw)
        out.append((ids, st, belt, moved))
    return out


def check_frames(tracker, frames, want, count="dev", who=""):
    """Every frame through `tracker`: the ids of all rows, the whole track state and the whole belt state equal the expectation's."""
    for f, ((b, s, c, n), (ids_w, st_w, belt_w, _)) in enumerate(zip(frames, want)):
        n_arg = torch.tensor([n], dtype=torch.int32, device="cuda") if count == "dev" else n
        ids = tracker.update(dev(b), dev(s), dev(c), n_arg)
        assert torch.equal(ids.cpu(), t_(ids_w)), (who, f)
        got = tracker.state_host()
        assert BR.same_belt(got["belt"], belt_w), (who, f, got["belt"], belt_w)
        assert same_state(got, st_w), (who, f)
        full = tracker.state()
        m = int(full["m"].item())
        assert all(not t[m:].any().item() for t in (full["boxes"], full["classes"], full["ids"], full["ttl"])), (who, f)


@functools.lru_cache(maxsize=None)
def sequence(rows, frames=5):
    return BR.moving_sequence(rows, (37, 2), frames=frames, seed=rows + 1)


# ------------------------------------------------------------------------------------------ form 1
@pytest.mark.parametrize("bin_,radius", [(1, 64), (2, 128), (16, 80)], ids=lambda v: str(v))
@pytest.mark.parametrize("rows,capacity", [(5, 8), (64, 64), (320, 1024)], ids=lambda v: str(v))
def test_form1_equals_host(ore, rows, capacity, bin_, radius):
    """Five frames moving (37, 2) px per frame with NaN / inf / low-score rows and a varying n: one workgroup, the histogram in LDS
    (129 x 129 bins at K = 64, 11 x 11 at bin 16)."""
    tr = ore.BeltTracker("cuda", capacity=capacity, score_thresh=SCORE, bin=bin_, radius=radius, frame=(400, 500))
    assert tr._belt_form == 1 and tr._belt_ws is None and tr.belt_params["half_bins"] == {1: 64, 2: 64, 16: 5}[bin_]
    frames = sequence(rows)
    want = host_reference(ore, frames, contract_kw(tr), dict(capacity=capacity, score_thresh=SCORE))
    check_frames(tr, frames, want, "dev", "n_dev")
    last = want[-1][2]
    assert last["frames"] == 5 and last["coasted"] >= 1
    if rows >= 64:
        assert last["coasted"] < 5 and any(w[2]["votes"] >= 3 for w in want)
        assert any((w[3]["ttl"] == 1).any() for w in want[1:])      # tracks leave the 400 x 500 frame
    print(f"rows {rows} capacity {capacity} bin {bin_}: shifts {[(w[2]['dx'], w[2]['dy'], w[2]['votes']) for w in want]}")


def test_counts_on_host_and_device(ore):
    """The row count as a host int and as a device word: the same frames, the same states; n = 0, a negative n and zero rows."""
    f = sequence(320)
    frames = [f[0], f[1], (f[2][0], f[2][1], f[2][2], 0), (f[3][0], f[3][1], f[3][2], 100), (f[4][0], f[4][1], f[4][2], -3),
              (f[4][0][:0], f[4][1][:0], f[4][2][:0], 0), f[4]]
    kw = dict(capacity=700, score_thresh=SCORE, ttl=4)
    for cls, extra in ((ore.BeltTracker, {}), (ore.WideBeltTracker, {"max_rows": 321})):
        a, b_ = cls("cuda", **kw, **extra), cls("cuda", **kw, **extra)
        want = host_reference(ore, frames, contract_kw(a), kw)
        assert want[2][2]["coasted"] == want[1][2]["coasted"] + 1 and want[2][2]["dx"] == want[1][2]["dx"] != 0
        check_frames(a, frames, want, "dev", cls.__name__)
        check_frames(b_, frames, want, "host", cls.__name__)
        assert a.stats() == b_.stats() and a.stats()["coasted"] >= 4


# ------------------------------------------------------------------------------------------ form 2
@pytest.mark.parametrize("rows,capacity,frames", [(321, 1024, 5), (2048, 4096, 3)], ids=lambda v: str(v))
def test_form2_equals_host(ore, rows, capacity, frames):
    """Beyond one workgroup: the votes of (1024 tracks) x (64 rows) work items on the whole chip, per-block LDS histograms added into
    the workspace, the finish in one workgroup."""
    tr = ore.WideBeltTracker("cuda", capacity=capacity, max_rows=rows, score_thresh=SCORE, frame=(400, 500))
    assert tr._belt_form == 2 and tr._belt_ws_bytes == (129 * 129 * 4 + 255) // 256 * 256
    fr = sequence(rows, frames)
    want = host_reference(ore, fr, contract_kw(tr), dict(capacity=capacity, score_thresh=SCORE))
    check_frames(tr, fr, want, "dev", "n_dev")
    assert want[-1][2]["coasted"] == 1 and want[-1][2]["votes"] > rows // 4, want[-1][2]
    assert want[-1][1]["m"] > 1024 or rows == 321


def test_limits_analytic(ore):
    """8192 rows on 16384 tracks.  Boxes of 40 px on a lattice of pitch 300 (beyond the window of 128): a pair votes iff it is a row and
    its own track.  Frame 1: ids 0 .. 8191, no tracks, the belt coasts.  Frame 2: every box moved (36, -8), in a fixed permutation: 8192
    votes in one bin, S = 8192 on its 3 x 3 block, of which the bin nearest the shift (0, 0) before it is (34, -6); every row continues
    its track.  Frame 3, no rows: the belt coasts and every track travels on."""
    f1, f2, perm = BR.lattice_case()
    tr = ore.WideBeltTracker("cuda", capacity=ore.TRACK_WIDE_MAX_TRACKS, max_rows=ore.TRACK_WIDE_MAX_ROWS, bin=2, radius=128)
    n = torch.tensor([8192], dtype=torch.int32, device="cuda")
    assert torch.equal(tr.update(dev(f1[0]), dev(f1[1]), dev(f1[2]), n).cpu(), torch.arange(8192))
    assert tr.state_host()["belt"] == dict(BR.empty_belt(), frames=1, coasted=1)
    ids2 = tr.update(dev(f2[0]), dev(f2[1]), dev(f2[2]), n)
    assert torch.equal(ids2.cpu(), t_(perm))
    st = tr.state_host()
    assert st["belt"] == dict(BR.empty_belt(), dx=34, dy=-6, votes=8192, travel_x=34, travel_y=-6, frames=2, coasted=1)
    assert st["m"] == 8192 and st["next_id"] == 8192 and torch.equal(t_(st["boxes"]), t_(f2[0])) and torch.equal(t_(st["ids"]), t_(perm))
    assert tr.stats() == {"tracks": 8192, "started": 8192, "frames": 2, "dropped": 0, "shift": (34, -6), "travel": (34, -6), "votes": 8192, "coasted": 1}
    tr.update(dev(f2[0]), dev(f2[1]), dev(f2[2]), 0)
    st = tr.state_host()
    assert st["belt"] == dict(BR.empty_belt(), dx=34, dy=-6, votes=0, travel_x=68, travel_y=-12, frames=3, coasted=2)
    assert st["m"] == 8192 and (st["ttl"] == 7).all() and torch.equal(t_(st["boxes"]), t_(f2[0] + np.array([34, -6, 34, -6], np.float32)))


# ------------------------------------------------------------------------------------------ the C entry on buffers of the test's own
class Raw:
    """ore_belt_shift_fwd on a belt state and a track state that sit between bands of 0xFF (NaN as floats) in one buffer."""

    def __init__(self, ore_, capacity, state_bytes=None, belt_bytes=None, half_bins=64):
        self.L, self.capacity = ore_.lib(), capacity
        self.sb = int(self.L.ore_track_wide_state_bytes(capacity))
        assert int(self.L.ore_belt_state_bytes()) == 64
        self.buf = torch.full((3 * BAND + 64 + self.sb,), 0xFF, dtype=torch.uint8, device="cuda")
        self.belt = self.buf[BAND:BAND + 64]
        self.state = self.buf[2 * BAND + 64:2 * BAND + 64 + self.sb]
        self.ws_bytes = int(self.L.ore_belt_workspace_bytes(capacity, 320, half_bins))
        self.ws = torch.full((self.ws_bytes,), 0xFF, dtype=torch.uint8, device="cuda")       # the contents mean nothing between calls
        if state_bytes is not None:
            self.state.copy_(state_bytes)
            self.belt.copy_(belt_bytes)

    def shift(self, b, s, c, n_dev=None, n_host=None, **k):
        p = lambda t: None if t is None else t.data_ptr()
        a = dict(belt=p(self.belt), state=p(self.state), capacity=self.capacity, boxes=p(b), scores=p(s), classes=p(c), n_dev=p(n_dev),
                 n_host=len(s) if n_host is None else n_host, max_rows=len(s), score=SCORE, aware=1, bin=2, half_bins=64, tol=0.125, min_votes=3,
                 frame_h=400, frame_w=500, form=0, ws=p(self.ws), ws_bytes=self.ws_bytes, stream=None)
        a.update(k)
        return self.L.ore_belt_shift_fwd(*[a[key] for key in ("belt", "state", "capacity", "boxes", "scores", "classes", "n_dev", "n_host", "max_rows",
                                                             "score", "aware", "bin", "half_bins", "tol", "min_votes", "frame_h", "frame_w", "form", "ws",
                                                             "ws_bytes", "stream")])

    def host(self):
        h = self.buf.cpu().numpy()
        return h[BAND:BAND + 64].copy(), h[2 * BAND + 64:2 * BAND + 64 + self.sb].copy()

    def bands_intact(self):
        h = self.buf.cpu().numpy()
        return (h[:BAND] == 0xFF).all() and (h[BAND + 64:2 * BAND + 64] == 0xFF).all() and (h[2 * BAND + 64 + self.sb:] == 0xFF).all()


@pytest.fixture(scope="module")
def running(ore):
    """A BeltTracker of capacity 1024 after three frames of 320 rows, and the fourth frame: (state bytes, belt bytes, frame, the host's
    expectation of the fourth shift)."""
    frames = sequence(320)
    tr = ore.BeltTracker("cuda", capacity=1024, score_thresh=SCORE, frame=(400, 500))
    for b, s, c, n in frames[:3]:
        tr.update(dev(b), dev(s), dev(c), n)
    st = tr.state_host()
    belt = st.pop("belt")
    moved, belt_w = ore.belt_shift_host(st, belt, *frames[3], **contract_kw(tr))
    torch.cuda.synchronize()
    return tr._buf.clone(), tr._belt.clone(), frames[3], moved, belt_w


def test_forms_agree_and_repeat(ore, running):
    """(320, 1024) takes both forms: form 1, form 2 and form 2 with direct global adds (3), each twice from copies of the same state,
    give the same bytes of both states -- those of the host statement."""
    state, belt, (b, s, c, n), moved, belt_w = running
    db, ds, dc = dev(b), dev(s), dev(c)
    assert ore.lib().ore_belt_shift_form(1024, 320, 64) == 1 and ore.lib().ore_belt_shift_form(1025, 320, 64) == 2
    assert ore.lib().ore_belt_shift_form(1024, 321, 64) == 2 and ore.lib().ore_belt_shift_form(1024, 320, 65) == EINVAL
    results = []
    for form in (1, 1, 2, 2, 3, 3, 0):
        r = Raw(ore, 1024, state, belt)
        assert r.shift(db, ds, dc, None, n, form=form, ws=None if form in (0, 1) else r.ws.data_ptr()) == 0, ore.lib().ore_last_error()
        torch.cuda.synchronize()
        assert r.bands_intact()
        results.append(r.host())
    for got in results[1:]:
        assert np.array_equal(got[0], results[0][0]) and np.array_equal(got[1], results[0][1])
    raw_belt, raw_state = results[0]
    got_belt = dict(zip(("dx", "dy", "votes"), raw_belt[:12].view(np.int32).tolist()), **dict(zip(("travel_x", "travel_y", "frames", "coasted"), raw_belt[16:48].view(np.int64).tolist())))
    assert BR.same_belt(got_belt, belt_w) and belt_w["votes"] > 50 and not raw_belt[12:16].any() and not raw_belt[48:].any()
    m = moved["m"]
    assert np.array_equal(raw_state[32:32 + 16 * m].view(np.int32), moved["boxes"].reshape(-1).view(np.int32))
    assert np.array_equal(raw_state[32 + 32 * 1024:32 + 32 * 1024 + 4 * m].view(np.int32), moved["ttl"]) and (moved["ttl"] == 1).any()


@pytest.mark.parametrize("form", [1, 2])
def test_untouched_memory(ore, running, form):
    """Bands of NaN bytes around the belt state and around the track state, and the slots m .. capacity - 1 filled with NaN bytes too:
    all of them come back unchanged, and so do the header, the classes, the ids and the input rows."""
    state, belt, (b, s, c, n), moved, _ = running
    cap, m = 1024, moved["m"]
    r = Raw(ore, cap, state, belt)
    o = 32
    for lo, hi, size in ((o, o + 16 * cap, 16), (o + 16 * cap, o + 24 * cap, 8), (o + 24 * cap, o + 32 * cap, 8), (o + 32 * cap, o + 36 * cap, 4)):
        r.state[lo + size * m:hi] = 0xFF
    before = r.host()[1]
    db, ds, dc = dev(b), dev(s), dev(c)
    assert r.shift(db, ds, dc, torch.tensor([n], dtype=torch.int32, device="cuda"), -1, form=form) == 0
    torch.cuda.synchronize()
    after = r.host()[1]
    assert r.bands_intact() and m < cap
    changed = np.nonzero(before != after)[0]
    ttl0 = o + 32 * cap
    assert len(changed) > 0 and all(o <= i < o + 16 * m or ttl0 <= i < ttl0 + 4 * m for i in changed)      # boxes and ttl of tracks 0 .. m - 1
    assert np.array_equal(after[o:o + 16 * m].view(np.int32), moved["boxes"].reshape(-1).view(np.int32))
    assert np.array_equal(db.cpu().numpy(), b, equal_nan=True) and np.array_equal(ds.cpu().numpy(), s, equal_nan=True) and np.array_equal(dc.cpu().numpy(), c)


def test_refusals(ore, running):
    """Each refused argument is ORE_EINVAL with a message before any launch: both states are byte for byte what they were."""
    state, belt, (b, s, c, n), _, _ = running
    r = Raw(ore, 1024, state, belt)
    db, ds, dc = dev(b), dev(s), dev(c)
    before = r.host()
    sp, bp, wp = r.state.data_ptr(), r.belt.data_ptr(), r.ws.data_ptr()
    bad = [dict(form=2, ws_bytes=r.ws_bytes - 256), dict(form=2, ws=None), dict(form=2, ws=wp + 16), dict(form=3, ws_bytes=0),
           dict(belt=sp), dict(belt=sp + r.sb - 64), dict(state=db.data_ptr()), dict(belt=ds.data_ptr()), dict(form=2, ws=sp), dict(form=2, ws=db.data_ptr()),
           dict(bin=3), dict(bin=0), dict(bin=32), dict(half_bins=65), dict(half_bins=0), dict(form=1, capacity=1025), dict(form=4), dict(form=-1),
           dict(tol=1.0), dict(tol=-0.5), dict(tol=float("nan")), dict(min_votes=0), dict(min_votes=(1 << 30) + 1), dict(frame_h=0), dict(frame_w=-1),
           dict(score=float("nan")), dict(capacity=0), dict(capacity=16385), dict(belt=None), dict(belt=bp + 8), dict(state=None), dict(state=sp + 4),
           dict(boxes=None), dict(boxes=db.data_ptr() + 4), dict(scores=None), dict(n_host=-1)]
    for kw in bad:
        assert r.shift(db, ds, dc, **dict({"n_host": n}, **kw)) == EINVAL, kw
        assert ore.lib().ore_last_error().startswith(b"ore_belt_shift_fwd"), kw
    big = dev(np.zeros((321, 4), np.float32)), dev(np.zeros(321, np.float32))
    assert r.shift(big[0], big[1], None, None, 321, form=1) == EINVAL                      # form 1 forced beyond its rows
    assert ore.lib().ore_belt_reset(None, None) == EINVAL and ore.lib().ore_belt_reset(bp + 4, None) == EINVAL
    assert ore.lib().ore_belt_workspace_bytes(1024, 320, 65) == 0 and ore.lib().ore_belt_workspace_bytes(16385, 320, 64) == 0
    torch.cuda.synchronize()
    after = r.host()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and r.bands_intact()
    for kw in (dict(radius=130), dict(bin=3), dict(size_tol=1.0), dict(min_votes=0), dict(frame=(0, 5))):
        with pytest.raises(ore.OreError):
            ore.BeltTracker("cuda", **kw)
    tr = ore.BeltTracker("cuda")
    with pytest.raises(ore.OreError, match="rows"):                                        # refused by the tracker's checks: no shift was enqueued
        tr.update(torch.zeros(321, 4, device="cuda"), torch.zeros(321, device="cuda"))
    assert tr.stats()["frames"] == 0 and tr.state_host()["belt"] == BR.empty_belt()


# ------------------------------------------------------------------------------------------ two streams
@pytest.mark.parametrize("wide", [False, True])
def test_two_streams(ore, wide):
    """Updates issued alternately on two streams give the ids and the states of the same calls on one stream."""
    rows = 321 if wide else 320
    make = (lambda: ore.WideBeltTracker("cuda", capacity=700, max_rows=rows, score_thresh=SCORE)) if wide else \
        (lambda: ore.BeltTracker("cuda", capacity=700, score_thresh=SCORE))
    args = [(dev(b), dev(s), dev(c), torch.tensor([n], dtype=torch.int32, device="cuda")) for b, s, c, n in sequence(rows)]
    one = make()
    want = [one.update(*a) for a in args]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    two = make()
    got = []
    for k, a in enumerate(args):
        st = streams[k & 1]
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            got.append(two.update(*a))
    torch.cuda.synchronize()
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    a, b_ = two.state_host(), one.state_host()
    assert a["belt"] == b_["belt"] and same_state(a, b_) and one.stats()["votes"] > 0


# ------------------------------------------------------------------------------------------ the wrappers
def fields(out):
    i = out["instances"]
    return i.pred_boxes.tensor, i.scores, i.pred_classes


def moving_frames(h, w, seed, k=3, step=(2, 12)):
    """k frames: a synthetic image moved `step` (down, right) pixels per frame, so that detections persist and move together."""
    raw = raw_image(seed, h, w)
    return [np.ascontiguousarray(np.roll(raw, (f * step[0], f * step[1]), (0, 1))) for f in range(k)]


def check_composition(ore_, tracker, results, capacity):
    """track_ids of every result = belt_shift_host + track_host fed with the result's own rows."""
    st, belt = None, None
    for out in results:
        b, s, c = (t.cpu().numpy() for t in fields(out))
        st, belt = ore_.belt_shift_host(st, belt, b, s, c, **contract_kw(tracker))
        ids, st = ore_.track_host(st, b, s, c, wide=True, capacity=capacity)
        assert len(s) > 0 and torch.equal(out["instances"].track_ids.cpu(), t_(ids))
    got = tracker.state_host()
    assert got["belt"] == belt and same_state(got, st) and belt["frames"] == len(results)
    return belt


def test_async_predictor_takes_a_belt_tracker(ore):
    """AsyncPredictor.put(frame, draw=True, track=BeltTracker(...)) on the synthetic detector: the tracker is a BoxTracker, nothing in
    put synchronises, and the ids are the host composition's."""
    from predictor import AsyncPredictor
    ap = AsyncPredictor(_cfg(["MODEL.ROI_HEADS.SCORE_THRESH_TEST", 0.0]), inflight=2)
    _load(ap.model)
    frames = moving_frames(300, 500, 300)
    tr = ore.BeltTracker(ap.model.device, frame=(300, 500))
    got = []
    try:
        ap.put(frames[0], draw=True, track=ore.BeltTracker(ap.model.device))       # engines, graphs and tables exist
        ap.get()
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            ap.put(frames[0], draw=True, track=tr)
            ap.put(frames[1], draw=True, track=tr)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        got.append(ap.get())
        ap.put(frames[2], draw=True, track=tr)
        while len(ap):
            got.append(ap.get())
    finally:
        ap.shutdown()
    assert all("vis_image" in g for g in got)
    belt = check_composition(ore, tr, got, 1024)
    print(f"async belt tracking: belt {belt}, {tr.stats()['started']} ids started")


def test_tiled_predictor_takes_a_wide_belt_tracker(ore):
    """TiledPredictor(..., track=WideBeltTracker(...)) on a 640 x 640 frame with two by two tiles."""
    from predictor import TiledPredictor
    cfg = _cfg()
    tr = ore.WideBeltTracker("cuda", capacity=800, max_rows=400, frame=(640, 640))
    pred = TiledPredictor(cfg, track=tr, tile=320, overlap=0, max_detections=400)
    _load(pred.model)
    assert pred.tiled.tracker is tr and len(pred.tiled.plan(640, 640)[0]["origins"]) == 4
    got = [pred(f) for f in moving_frames(640, 640, 77)]
    belt = check_composition(ore, tr, got, 800)
    stats = pred.track_stats()
    assert stats["frames"] == 3 and stats["shift"] == (belt["dx"], belt["dy"]) and stats["travel"] == (belt["travel_x"], belt["travel_y"])
    print(f"tiled belt tracking: belt {belt}, {stats['started']} ids started")


# ------------------------------------------------------------------------------------------ the property
@pytest.mark.parametrize("objs", [30, 400])
def test_ids_persist_on_the_planted_belt(ore, objs):
    """The host test's property on the device: on the planted belt ((37, 2) px per frame, 8 frames) every object seen in two consecutive
    frames keeps its id under the belt tracker, none under "track v1" alone; the device's ids are the host trackers'."""
    frames = BR.belt_sequence(objs, shift=(37, 2), frames=8, seed=objs)
    kinds = [(ore.WideBeltTracker, ore.WideBoxTracker)] + ([(ore.BeltTracker, ore.BoxTracker)] if objs <= 320 else [])
    for belt_cls, plain_cls in kinds:
        belt, plain, host = belt_cls("cuda", bin=2, frame=(1080, 1920)), plain_cls("cuda"), belt_cls("cpu", bin=2, frame=(1080, 1920))
        ids_belt = [belt.update(dev(b), dev(s), dev(c), n).cpu().numpy() for b, s, c, n, _ in frames]
        ids_plain = [plain.update(dev(b), dev(s), dev(c), n).cpu().numpy() for b, s, c, n, _ in frames]
        kept, total = BR.kept_ids(frames, ids_belt)
        assert total > 6 * objs and kept == total, (kept, total)
        assert BR.kept_ids(frames, ids_plain) == (0, total)
        for (b, s, c, n, _), got in zip(frames, ids_belt):
            assert np.array_equal(host.update(b, s, c, n).numpy(), got)
        assert belt.stats() == host.stats() and belt.stats()["started"] < 1.1 * objs < 6 * objs < plain.stats()["started"]


# ------------------------------------------------------------------------------------------ the demo
def belt_video(k=5, step=64):
    """k frames of one synthetic picture moved `step` px to the right per frame: a multiple of the coarsest stride, so the detections
    move with the picture (the seam of the roll aside)."""
    raw = raw_image(300, 320, 512)
    return [np.ascontiguousarray(np.roll(raw, f * step, 1)) for f in range(k)]


def test_visualization_demo_belt(ore):
    """VisualizationDemo(track="belt"), serial and parallel: a BeltTracker whose frame is the video's, the same statistics both ways, the
    shift of the picture found.  (How many ids that saves is not this test's: the synthetic detector's boxes do not all follow the
    picture.  The planted belt below and test_ids_persist_on_the_planted_belt show it.)"""
    from predictor import VisualizationDemo
    cfg = _cfg(["MODEL.ROI_HEADS.SCORE_THRESH_TEST", 0.0])
    frames = belt_video()
    demos = {k: VisualizationDemo(cfg, parallel=par, track=tr) for k, par, tr in (("serial", False, "belt"), ("parallel", True, "belt"), ("plain", False, True))}
    try:
        for d in demos.values():
            _load(d.predictor.model)
        out = {k: list(d.run_on_video(iter(frames))) for k, d in demos.items()}
        stats = {k: d.track_stats() for k, d in demos.items()}
        print("demo:", stats)
        for k in ("serial", "parallel"):
            tr = demos[k].tracker
            assert type(tr) is ore.BeltTracker and (tr.belt_params["frame_h"], tr.belt_params["frame_w"]) == (320, 512)
        assert type(demos["plain"].tracker) is ore.BoxTracker and set(stats["plain"]) == {"tracks", "started", "frames", "dropped"}
        assert stats["serial"] == stats["parallel"] and stats["serial"]["frames"] == 5
        assert all(np.array_equal(a, b) for a, b in zip(out["serial"], out["parallel"])) and len(out["serial"]) == 5
        assert abs(stats["serial"]["shift"][0] - 64) <= 2 and stats["serial"]["shift"][1] == 0 and stats["serial"]["votes"] >= 3
        list(demos["serial"].run_on_video(frames[:2]))          # again: both states start afresh
        again = demos["serial"].track_stats()
        assert again["frames"] == 2 and again["coasted"] >= 1 and again["travel"][0] <= 66
    finally:
        demos["parallel"].predictor.shutdown()
    with pytest.raises(ValueError, match="belt"):
        VisualizationDemo(cfg, track="kalman")
    with pytest.raises(ValueError, match="belt"):
        VisualizationDemo(cfg, track=True, belt={"bin": 4})


def test_demo_prints_a_count_that_does_not_grow_with_the_frames(ore, tmp_path, monkeypatch, capsys):
    """demo.py --track --track-motion belt over a sequence of image files, with the planted belt's rows in place of the detector's (the
    synthetic detector's boxes do not follow the picture): the particle count printed for 6 frames is the one printed for 3, up to the
    few ids a low IoU restarts; with --track alone it grows by every frame's detections.  The mean shift is the planted one."""
    import re
    from PIL import Image
    from detectron2.structures import Boxes, Instances
    import demo
    import predictor
    planted = BR.belt_sequence(30, shift=(37, 2), frames=6, seed=30)

    class Planted:
        """DefaultPredictor's call with the planted rows of frame 0, 1, ... as its detections."""
        def __init__(self, real):
            self.model, self.metadata, self.calls = real.model, getattr(real, "metadata", None), 0

        def __call__(self, frame):
            b, s, c, _, _ = planted[self.calls]
            self.calls += 1
            inst = Instances(tuple(frame.shape[:2]))
            inst.pred_boxes, inst.scores, inst.pred_classes = Boxes(dev(b)), dev(s), dev(c)
            return {"instances": inst}

    class Demo(predictor.VisualizationDemo):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.predictor = Planted(self.predictor)

    monkeypatch.setattr(predictor, "VisualizationDemo", Demo)
    paths = []
    for f in range(6):
        paths.append(str(tmp_path / f"f{f}.png"))
        Image.fromarray(np.full((1080, 1920, 3), 40 + f, np.uint8)).save(paths[-1])
    (tmp_path / "out").mkdir()
    tail = ["--output", str(tmp_path / "out"), "--opts", "MODEL.DEVICE", "cuda", "MODEL.WEIGHTS", ""]
    started = {}
    for flags in (("--track",), ("--track", "--track-motion", "belt", "--belt-radius", "96")):
        for k in (3, 6):
            demo.main(list(flags) + ["--input"] + paths[:k] + tail)
            line = [l for l in capsys.readouterr().out.splitlines() if l.startswith("tracks started:")][-1]
            started[(len(flags) > 1, k)] = int(re.match(r"tracks started: (\d+)", line)[1])
            if len(flags) > 1:
                m = re.search(r"mean shift per frame: \((-?[\d.]+), (-?[\d.]+)\) px over (\d+) frames, (\d+) coasted", line)
                assert m and int(m[3]) == k and int(m[4]) == 1, line
                assert abs(float(m[1]) * k / (k - 1) - 37) <= 1.5 and abs(float(m[2]) * k / (k - 1) - 2) <= 1.5, line
            assert all((tmp_path / "out" / f"f{f}.png").exists() for f in range(k))
    print("demo.py tracks started:", started)
    assert started[(False, 6)] - started[(False, 3)] > 60 and started[(False, 3)] > 75         # every frame starts its detections afresh
    assert 28 <= started[(True, 3)] <= started[(True, 6)] <= 33                                 # 30 particles, whatever the frame count
