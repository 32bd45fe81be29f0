"""GPU: the wide tracker (csrc/ore_track_wide.hip: k_track_wide_cand + k_track_wide_match) computes the association contract "track v1"
for up to 8192 rows and 16384 tracks.  Every comparison is exact -- torch.equal on the ids and on every field of state_host(): against
the one-workgroup kernel (BoxTracker) where both take the input, against orehip.track_host(wide=True) at the shapes where the kernels'
paths change, against an analytic expectation at the limits; then across two streams and behind the tiled and TTA merges.  The
expectation of a case is computed once and shared by the ways it is run."""
import functools

import numpy as np
import pytest
import torch

import track_ref as TR
import track_wide_ref as WR
from test_hip_resize import _cfg, _load, raw_image
from test_hip_tta import tta_cfg

pytestmark = pytest.mark.gpu
SCORE = 0.05                                                   # track_ref.sequence plants scores of 0.01
FIELDS = ("boxes", "classes", "ids", "ttl")


@pytest.fixture(scope="module")
def ore():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import orehip
    orehip.lib()
    return orehip


@pytest.fixture(scope="module")
def model(ore):
    """The synthetic detector of tests/test_hip_resize.py."""
    from detectron2.modeling import build_model
    cfg = _cfg()
    cfg.freeze()
    return _load(build_model(cfg))


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_state(got, want):
    """Two state_host() / track_host dicts: the four counters and torch.equal on every array."""
    return all(int(got[k]) == int(want[k]) for k in ("m", "next_id", "frames", "dropped")) and \
        all(torch.equal(torch.from_numpy(np.ascontiguousarray(got[k])), torch.from_numpy(np.ascontiguousarray(want[k]))) for k in FIELDS)


def host_reference(ore_, frames, **kw):
    """[(ids, state)] of the frames through track_host(wide=True)."""
    st, out = None, []
    for b, s, c, n in frames:
        ids, st = ore_.track_host(st, b, s, c, n, wide=True, **kw)
        out.append((ids, st))
    return out


def check_frames(tracker, frames, want, count="dev", who=""):
    """Every frame through `tracker`: the ids of all rows (the -1s included) and the whole state equal the expectation's after each,
    and the slots behind the list hold zeros."""
    for f, ((b, s, c, n), (ids_w, st_w)) in enumerate(zip(frames, want)):
        n_arg = torch.tensor([n], dtype=torch.int32, device="cuda") if count == "dev" else n
        ids = tracker.update(dev(b), dev(s), dev(c), n_arg)
        assert ids.dtype == torch.int64 and ids.shape == (len(s),)
        bad = np.nonzero(ids.cpu().numpy() != ids_w)[0]
        assert torch.equal(ids.cpu(), torch.from_numpy(ids_w)), (who, f, bad[:8], ids.cpu().numpy()[bad[:8]], ids_w[bad[:8]])
        assert same_state(tracker.state_host(), st_w), (who, f)
        full = tracker.state()
        m = int(full["m"].item())
        assert all(not t[m:].any().item() for t in (full["boxes"], full["classes"], full["ids"], full["ttl"])), (who, f)


@functools.lru_cache(maxsize=None)
def sequence(rows, seed):
    return TR.sequence(rows, frames=5, seed=seed)


# ------------------------------------------------------------------------------------------ against the one-workgroup kernel
@pytest.mark.parametrize("rows,capacity", [(5, 8), (64, 64), (65, 130), (320, 1024)], ids=lambda v: str(v))
def test_equals_box_tracker(ore, rows, capacity):
    """5 frames through both kernels: the same ids, the same state buffer byte for byte."""
    kw = dict(capacity=capacity, score_thresh=SCORE)
    narrow, wide = ore.BoxTracker("cuda", **kw), ore.WideBoxTracker("cuda", max_rows=rows, **kw)
    started = 0
    for b, s, c, n in sequence(rows, rows):
        n_dev = torch.tensor([n], dtype=torch.int32, device="cuda")
        a, w = narrow.update(dev(b), dev(s), dev(c), n_dev), wide.update(dev(b), dev(s), dev(c), n_dev)
        assert torch.equal(a, w)
        assert same_state(narrow.state_host(), wide.state_host())
        torch.cuda.synchronize()
        used = 32 + 36 * capacity                               # the buffer is rounded up to 16 bytes; the padding is nobody's
        assert torch.equal(narrow._buf[:used], wide._buf[:used])
        started = wide.stats()["started"]
    assert started > rows // 2


# ------------------------------------------------------------------------------------------ against the host twin
# (rows, capacity, keyword arguments): rows on both sides of a 64-bit word and of v1's 320; m on both sides of the 1024 threads and of
# two strides; capacity 1025 / 1023 / 2049 with more live rows plus survivors than slots; a short ttl; classes ignored
HOST_CASES = [(63, 200, {}), (64, 200, {}), (65, 200, {}), (321, 700, {}), (321, 700, {"ttl": 2}), (321, 700, {"class_aware": False}),
              (1200, 1023, {}), (1200, 1025, {}), (2300, 2049, {"ttl": 3})]


@pytest.mark.parametrize("rows,capacity,extra", HOST_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_equals_host_on_sequences(ore, rows, capacity, extra):
    """5 frames: boxes drift, rows drop out and come back, new rows appear, rows with NaN / inf / low scores in between, n below the
    row count in some frames."""
    frames = sequence(rows, rows + 1)
    if extra.get("class_aware") is False:
        frames = [(b, s, None, n) for b, s, _, n in frames]
    kw = dict(capacity=capacity, score_thresh=SCORE, **extra)
    want = host_reference(ore, frames, **kw)
    check_frames(ore.WideBoxTracker("cuda", max_rows=rows, **kw), frames, want, "dev", "n_dev")
    last = want[-1][1]
    assert any((ids == -1).any() for ids, _ in want) and last["next_id"] > want[0][1]["next_id"] > 0
    assert any(n < rows for _, _, _, n in frames)
    if capacity in (1023, 1025, 2049):
        assert last["m"] == capacity and last["dropped"] > 0
        assert want[0][1]["m"] == capacity                      # every later update runs on m = capacity tracks
    else:
        check_frames(ore.WideBoxTracker("cuda", max_rows=rows, **kw), frames, want, "host", "n_host")
    if extra.get("ttl") == 2:
        assert last["m"] < host_reference(ore, frames, **dict(kw, ttl=8))[-1][1]["m"]      # tracks expired
    print(f"rows {rows} capacity {capacity} {extra}: {last['next_id']} ids started, m {last['m']}, dropped {last['dropped']}")


def test_counts_and_empty_state(ore):
    """n_dev = 0 on the empty state and on a full one (every track ages, none matches), n_dev below the row count, a negative count,
    and an update of zero rows."""
    f = sequence(321, 5)
    frames = [(f[0][0], f[0][1], f[0][2], 0), f[1], (f[2][0], f[2][1], f[2][2], 0), (f[3][0], f[3][1], f[3][2], 100),
              (f[4][0], f[4][1], f[4][2], -3), (f[4][0][:0], f[4][1][:0], f[4][2][:0], 0), (f[1][0], f[1][1], f[1][2], 70)]
    kw = dict(capacity=700, score_thresh=SCORE, ttl=4)
    want = host_reference(ore, frames, **kw)
    assert want[0][1]["m"] == 0 and want[0][1]["frames"] == 1 and (want[0][0] == -1).all()
    assert (want[3][0][100:] == -1).all() and (want[3][0][:100] >= 0).any()
    check_frames(ore.WideBoxTracker("cuda", max_rows=321, **kw), frames, want, "dev")
    check_frames(ore.WideBoxTracker("cuda", max_rows=321, **kw), frames, want, "host")


def test_chain_across_words(ore):
    """The 130-pair chain that needs 130 rounds, slots 60 .. 189 and rows 35 .. 164: the chain crosses two word boundaries of either
    mask, and the bounded loop of the match runs to its last round."""
    frames = WR.chain_case(130, t_off=60, r_off=35)
    kw = dict(capacity=512, iou_thresh=WR.CHAIN_IOU_THRESH)
    assert WR.update_rounds(WR.update_rounds(None, *frames[0], **kw)[1], *frames[1], **kw)[2] == 130
    want = host_reference(ore, frames, **kw)
    assert np.array_equal(want[1][0][35:], 60 + np.arange(130))
    check_frames(ore.WideBoxTracker("cuda", max_rows=200, **kw), frames, want)
    frames = WR.chain_case(130)                                  # as many rounds as min(m, live rows): the bound itself
    check_frames(ore.WideBoxTracker("cuda", max_rows=130, **kw), frames, host_reference(ore, frames, **kw))


@pytest.mark.parametrize("aware", [True, False])
def test_tie_heavy_grid(ore, aware):
    """Boxes on a coarse grid: a few dozen distinct IoUs shared by thousands of pairs; slot, then row decides."""
    frames = WR.grid_case(400, seed=5)
    kw = dict(capacity=1500, iou_thresh=0.3, class_aware=aware)
    check_frames(ore.WideBoxTracker("cuda", max_rows=400, **kw), frames, host_reference(ore, frames, **kw))


# ------------------------------------------------------------------------------------------ at the limits
def test_limits_analytic(ore):
    """8192 rows, capacity 16384.  Frame 1: 8192 disjoint boxes -> ids 0 .. 8191.  Frame 2: every box moved 2 pixels, in a fixed
    permutation -> each row overlaps its predecessor alone (IoU 0.846): the ids are the permutation, nothing starts, nothing is lost."""
    f1, f2, perm = WR.limit_case()
    tr = ore.WideBoxTracker("cuda", capacity=ore.TRACK_WIDE_MAX_TRACKS, max_rows=ore.TRACK_WIDE_MAX_ROWS)
    n = torch.tensor([8192], dtype=torch.int32, device="cuda")
    ids1 = tr.update(dev(f1[0]), dev(f1[1]), dev(f1[2]), n)
    assert torch.equal(ids1.cpu(), torch.arange(8192))
    ids2 = tr.update(dev(f2[0]), dev(f2[1]), dev(f2[2]), n)
    assert torch.equal(ids2.cpu(), torch.from_numpy(perm))
    assert tr.stats() == {"tracks": 8192, "started": 8192, "frames": 2, "dropped": 0}
    st = tr.state_host()
    assert st["m"] == 8192 and torch.equal(torch.from_numpy(st["boxes"]), torch.from_numpy(f2[0])) and torch.equal(torch.from_numpy(st["ids"]), torch.from_numpy(perm))
    assert (st["ttl"] == 8).all() and (st["classes"] == 0).all()
    # a third frame without rows: all 8192 tracks survive behind no rows, one frame older
    tr.update(dev(f2[0]), dev(f2[1]), dev(f2[2]), 0)
    st = tr.state_host()
    assert st["m"] == 8192 and (st["ttl"] == 7).all() and torch.equal(torch.from_numpy(st["ids"]), torch.from_numpy(perm))


# ------------------------------------------------------------------------------------------ two streams
def test_two_streams(ore):
    """Updates issued alternately on two streams give the ids of the same calls on one stream: the tracker orders them by its event."""
    frames = sequence(321, 322)
    kw = dict(capacity=700, score_thresh=SCORE, max_rows=321)
    args = [(dev(b), dev(s), dev(c), torch.tensor([n], dtype=torch.int32, device="cuda")) for b, s, c, n in frames]
    one = ore.WideBoxTracker("cuda", **kw)
    want = [one.update(*a) for a in args]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    two = ore.WideBoxTracker("cuda", **kw)
    got = []
    for k, a in enumerate(args):
        st = streams[k & 1]
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            got.append(two.update(*a))
    torch.cuda.synchronize()
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    assert same_state(two.state_host(), one.state_host()) and one.stats()["started"] > 321


# ------------------------------------------------------------------------------------------ behind the merges
def fields(out):
    i = out["instances"]
    return i.pred_boxes.tensor, i.scores, i.pred_classes


def check_wiring(ore_, plain, tracked, requests, **host_kw):
    """The tracked wrapper returns what the plain one returns, plus track_ids = track_host(wide=True) over the returned instances."""
    st, started, total = None, 0, 0
    for req in requests:
        want, got = plain([req])[0], tracked([req])[0]
        for a, b in zip(fields(want), fields(got)):
            assert torch.equal(a, b)
        assert not want["instances"].has("track_ids")
        b, s, c = (t.cpu().numpy() for t in fields(got))
        ids, st = ore_.track_host(st, b, s, c, wide=True, **host_kw)
        assert len(s) > 0 and torch.equal(got["instances"].track_ids.cpu(), torch.from_numpy(ids))
        started, total = st["next_id"], total + len(s)
    print(f"{type(tracked).__name__}: {total} rows in {len(requests)} frames, {started} ids started")
    assert tracked.track_stats() == {"tracks": st["m"], "started": started, "frames": len(requests), "dropped": st["dropped"]}
    assert plain.track_stats() == {"tracks": 0, "started": 0, "frames": 0, "dropped": 0}
    return st


def moving_frames(h, w, seed):
    """Two frames: a synthetic image, and the same image moved 3 pixels right and 2 down, so that detections persist."""
    raw = raw_image(seed, h, w)
    return [raw, np.ascontiguousarray(np.roll(raw, (2, 3), (0, 1)))]


def test_tiled_inference_tracks(ore, model):
    """TiledInference(track=True) on two 1280x1280 frames, 4 tiles and the full frame: one WideBoxTracker sized for the merge."""
    from fewx.modeling import TiledInference
    cfg = _cfg()
    kw = dict(tile=640, overlap=0, max_detections=400)
    plain, tracked = TiledInference(cfg, model, **kw), TiledInference(cfg, model, track=True, **kw)
    assert plain.tracker is None and isinstance(tracked.tracker, ore.WideBoxTracker)
    assert (tracked.tracker.max_rows, tracked.tracker.capacity) == (400, 800)
    frames = moving_frames(1280, 1280, 77)
    assert len(tracked.plan(1280, 1280)[0]["origins"]) == 4
    st = check_wiring(ore, plain, tracked, [{"image_raw": f} for f in frames], capacity=800)
    assert st["frames"] == 2 and st["m"] > 0
    # still one host wait per frame: everything up to the ids is enqueued with torch's sync debug mode on "error"
    dev_frame = torch.from_numpy(frames[0]).cuda()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        p = tracked._enqueue({"image_raw": dev_frame})
    finally:
        torch.cuda.set_sync_debug_mode("default")
    out = tracked._finish(p)
    assert len(out["instances"].track_ids) == len(out["instances"].scores) > 0
    with pytest.raises(ValueError, match="WideBoxTracker"):
        TiledInference(cfg, model, track=ore.BoxTracker("cuda"), **kw)       # 400 rows do not fit the one-workgroup tracker
    with pytest.raises(ValueError, match="track is"):
        TiledInference(cfg, model, track="yes", **kw)


def test_tta_tracks(ore, model):
    """GeneralizedRCNNWithTTA(track=...) with two variants (two sizes, no flip): track=True keeps the one-workgroup tracker, and a
    WideBoxTracker of the caller's gives the same ids."""
    from detectron2.modeling import GeneralizedRCNNWithTTA
    cfg = tta_cfg(["TEST.AUG.MIN_SIZES", [256, 320]], flip=False)
    plain = GeneralizedRCNNWithTTA(cfg, model)
    narrow = GeneralizedRCNNWithTTA(cfg, model, track=True)
    rows = narrow.topk + (narrow.topk & 1)
    wide = GeneralizedRCNNWithTTA(cfg, model, track=ore.WideBoxTracker("cuda", capacity=1024, max_rows=rows))
    assert type(narrow.tracker) is ore.BoxTracker and len(narrow.tta_mapper.variants(300, 500)) == 2
    requests = [{"image_raw": f} for f in moving_frames(300, 500, 78)]
    check_wiring(ore, plain, narrow, requests, capacity=1024)
    check_wiring(ore, plain, wide, requests, capacity=1024)


# ------------------------------------------------------------------------------------------ refusals
def test_refused_arguments(ore):
    """Each refused argument raises OreError before any launch: the tracker's state is what it was."""
    for bad in (dict(capacity=0), dict(capacity=16385), dict(max_rows=8193), dict(max_rows=-1), dict(ttl=0), dict(ttl=(1 << 20) + 1),
                dict(iou_thresh=-0.1), dict(iou_thresh=float("nan")), dict(score_thresh=float("nan")), dict(capacity=1.5), dict(max_rows=True)):
        with pytest.raises(ore.OreError):
            ore.WideBoxTracker("cuda", **bad)
    tr = ore.WideBoxTracker("cuda", capacity=100, max_rows=64)
    b, s, c, n = sequence(65, 66)[0]
    with pytest.raises(ore.OreError, match="65 rows"):
        tr.update(dev(b), dev(s), dev(c))
    with pytest.raises(ore.OreError):
        tr.update(dev(b[:64]).double(), dev(s[:64]), dev(c[:64]))
    with pytest.raises(ore.OreError):
        tr.update(dev(b[:64]), dev(s[:64]), dev(c[:64]), torch.tensor([3], dtype=torch.int64, device="cuda"))
    L, P = ore.lib(), ore._ptr
    bx, sc, out = dev(b[:64]), dev(s[:64]), torch.empty(64, dtype=torch.int64, device="cuda")
    call = lambda **k: L.ore_track_wide_update_fwd(*[{**dict(state=P(tr._buf), capacity=100, boxes=P(bx), scores=P(sc), classes=None, n_dev=None, n_host=64,
                                                            max_rows=64, score=0.0, iou=0.6, ttl=8, aware=1, ids=P(out), ws=P(tr._ws), ws_bytes=tr._ws_bytes,
                                                            stream=None), **k}[key] for key in
                                                     ("state", "capacity", "boxes", "scores", "classes", "n_dev", "n_host", "max_rows", "score", "iou", "ttl", "aware",
                                                      "ids", "ws", "ws_bytes", "stream")])
    for bad in (dict(ws=None), dict(ws_bytes=tr._ws_bytes - 256), dict(ws=P(tr._ws) + 8), dict(ws=P(tr._buf)), dict(ids=P(bx)), dict(boxes=P(bx) + 4),
                dict(capacity=16385), dict(max_rows=8193), dict(boxes=None)):
        assert call(**bad) == -22 and L.ore_last_error().startswith(b"ore_track_wide_update_fwd"), bad
    assert tr.stats() == {"tracks": 0, "started": 0, "frames": 0, "dropped": 0}
    assert call() == 0 and tr.stats()["frames"] == 1
