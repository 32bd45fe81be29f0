"""CPU: the wide form of the tracker on the host.  The rounds of mutually best pairs (tests/track_wide_ref.py, the way
csrc/ore_track_wide.hip reaches the matching) give the sorted greedy matching of orehip.track_host(wide=True) -- on random sequences,
on tie-heavy inputs and on a chain that needs one round per pair; wide=True changes the limits and nothing else; the C-ABI declares
the wide entry points and refuses every limit before any launch."""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
import track_ref as TR
import track_wide_ref as WR


@pytest.fixture(scope="module")
def ore():
    import orehip
    return orehip


def run_both(ore, frames, **kw):
    """Every frame through track_host(wide=True) and the rounds; ids and every field of the state agree after each.  Returns the
    ids, the states and the rounds per frame."""
    host, ref, out = None, None, []
    for f, (b, s, c, n) in enumerate(frames):
        ids, host = ore.track_host(host, b, s, c, n, wide=True, **kw)
        want, ref, rounds = WR.update_rounds(ref, b, s, c, n, **kw)
        assert ids.dtype == np.int64 and np.array_equal(ids, want), (f, np.nonzero(ids != want)[0][:8])
        assert WR.same_state(host, ref), f
        out.append((ids, ref, rounds))
    return out


@pytest.mark.parametrize("rows,capacity", [(0, 1), (5, 8), (65, 130), (321, 1025), (700, 600)], ids=lambda v: str(v))
def test_rounds_equal_sorted_greedy_on_sequences(ore, rows, capacity):
    res = run_both(ore, WR.sequence(rows, seed=rows), capacity=capacity, score_thresh=0.05)
    run_both(ore, [(b, s, None, n) for b, s, _, n in WR.sequence(rows, seed=rows + 1)], capacity=capacity, score_thresh=0.05, class_aware=False, ttl=2)
    if rows >= 65:                                           # the sequences do what they claim
        assert res[-1][1]["next_id"] > res[0][1]["next_id"] > 0 and any((ids == -1).any() for ids, _, _ in res)
        assert set(res[0][0][res[0][0] >= 0]) & set(res[1][0][res[1][0] >= 0])      # ids persist
    if (rows, capacity) == (700, 600):
        assert res[-1][1]["dropped"] > 0 and res[-1][1]["m"] == 600                # beyond v1's limits, and the overflow path


@pytest.mark.parametrize("aware", [True, False])
def test_rounds_equal_sorted_greedy_on_ties(ore, aware):
    """Boxes on a coarse grid: most candidate pairs share their IoU with others exactly, so the tie order decides."""
    frames = WR.grid_case(200, seed=3)
    res = run_both(ore, frames, capacity=512, iou_thresh=0.3, class_aware=aware)
    iou = WR.iou_matrix(frames[0][0], frames[1][0])
    vals, counts = np.unique(iou[iou > np.float32(0.3)], return_counts=True)
    assert len(vals) < 40 and counts.max() > 100, (len(vals), counts.max())       # few distinct values, each shared by many pairs
    assert any(r > 1 for _, _, r in res)
    run_both(ore, TR.ties_case(), capacity=64)


def test_chain_needs_one_round_per_pair(ore):
    """130 tracks and 130 rows whose accepted pairs free one another one by one: the rounds are 130, and the result is the greedy's."""
    frames = WR.chain_case(130)
    res = run_both(ore, frames, capacity=512, iou_thresh=WR.CHAIN_IOU_THRESH)
    assert res[1][2] == 130, res[1][2]
    assert np.array_equal(res[1][0], np.arange(130))
    res = run_both(ore, WR.chain_case(130, t_off=60, r_off=35), capacity=512, iou_thresh=WR.CHAIN_IOU_THRESH)
    assert res[1][2] == 130 and np.array_equal(res[1][0][35:], 60 + np.arange(130)) and np.array_equal(res[1][0][:35], np.arange(35))


@pytest.mark.parametrize("rows,capacity", [(5, 8), (64, 64), (320, 1024)], ids=lambda v: str(v))
def test_wide_flag_changes_nothing_at_v1_sizes(ore, rows, capacity):
    a = b = None
    for bx, s, c, n in TR.sequence(rows, frames=5, seed=rows):
        ids_a, a = ore.track_host(a, bx, s, c, n, capacity=capacity, score_thresh=0.05)
        ids_b, b = ore.track_host(b, bx, s, c, n, capacity=capacity, score_thresh=0.05, wide=True)
        assert np.array_equal(ids_a, ids_b) and WR.same_state(a, b)


def test_limits(ore):
    box = lambda k: np.tile(np.array([[0, 0, 4, 4]], np.float32), (k, 1))
    one = lambda k: np.ones(k, np.float32)
    with pytest.raises(ore.OreError, match="321 scores"):
        ore.track_host(None, box(321), one(321))
    with pytest.raises(ore.OreError, match="1 .. 1024"):
        ore.track_host(None, box(1), one(1), capacity=1025)
    ids, st = ore.track_host(None, box(321), one(321), capacity=1025, wide=True)
    assert len(ids) == 321 and st["m"] == 321
    with pytest.raises(ore.OreError, match="8193 scores"):
        ore.track_host(None, box(8193), one(8193), wide=True)
    with pytest.raises(ore.OreError, match="1 .. 16384"):
        ore.track_host(None, box(1), one(1), capacity=16385, wide=True)
    for bad in (dict(capacity=0), dict(capacity=16385), dict(max_rows=-1), dict(max_rows=8193), dict(ttl=0), dict(iou_thresh=float("nan"))):
        with pytest.raises(ore.OreError):
            ore.WideBoxTracker("cpu", **bad)


def test_wide_box_tracker_on_host_tensors(ore):
    """WideBoxTracker("cpu") is track_host(wide=True) with the state kept; everything else is BoxTracker's."""
    assert issubclass(ore.WideBoxTracker, ore.BoxTracker)
    for name in ("update", "reset", "state", "state_host", "stats", "_updated"):
        assert getattr(ore.WideBoxTracker, name) is getattr(ore.BoxTracker, name), name
    tr = ore.WideBoxTracker("cpu", capacity=2000, max_rows=400, score_thresh=0.05)
    ref = None
    for b, s, c, n in WR.sequence(400, seed=9):
        ids = tr.update(torch.from_numpy(b), torch.from_numpy(s), torch.from_numpy(c), n)
        want, ref, _ = WR.update_rounds(ref, b, s, c, n, capacity=2000, score_thresh=0.05)
        assert ids.dtype == torch.int64 and np.array_equal(ids.numpy(), want)
    assert WR.same_state(tr.state_host(), ref)
    assert tr.stats() == {"tracks": ref["m"], "started": ref["next_id"], "frames": 5, "dropped": 0} and ref["m"] > 400


def test_c_abi_declares_and_refuses(ore):
    import inspect
    with open(os.path.join(ROOT, "include", "ore_hip.h")) as f:
        header = f.read()
    for text in ("#define ORE_TRACK_WIDE_MAX_TRACKS 16384", "#define ORE_TRACK_WIDE_MAX_ROWS 8192", "size_t ore_track_wide_state_bytes(int32_t capacity);",
                 "size_t ore_track_wide_workspace_bytes(int32_t capacity, int32_t max_rows);", "int ore_track_wide_reset(void* state, int32_t capacity, void* stream);",
                 "int ore_track_wide_update_fwd(void* state, int32_t capacity, const float* boxes,"):
        assert text in header, text
    assert "track v2" not in header and "track wide" not in header           # the wide form computes "track v1": no new contract
    L = ore.lib()
    for name in ("ore_track_wide_state_bytes", "ore_track_wide_workspace_bytes", "ore_track_wide_reset", "ore_track_wide_update_fwd"):
        assert name in ore.SYMBOLS and hasattr(L, name), name
    assert (ore.TRACK_WIDE_MAX_TRACKS, ore.TRACK_WIDE_MAX_ROWS) == (16384, 8192)
    assert L.ore_track_wide_state_bytes(16385) == 0 and L.ore_track_wide_state_bytes(0) == 0
    assert L.ore_track_wide_state_bytes(16384) == 32 + 36 * 16384 and L.ore_track_wide_state_bytes(1024) == L.ore_track_state_bytes(1024)
    assert L.ore_track_wide_workspace_bytes(16385, 1) == 0 and L.ore_track_wide_workspace_bytes(1, 8193) == 0 and L.ore_track_wide_workspace_bytes(1, -1) == 0
    need = L.ore_track_wide_workspace_bytes(16384, 8192)
    assert need >= 2 * 16384 * 8192 // 8 + 36 * 16384 and need % 256 == 0     # both bit matrices and the copy of the old list
    assert L.ore_track_wide_workspace_bytes(64, 64) < L.ore_track_wide_workspace_bytes(65, 64) <= L.ore_track_wide_workspace_bytes(65, 65)
    for bad in ((None, 0, None), (None, 16385, None)):
        assert L.ore_track_wide_reset(*bad) == -22 and b"capacity" in L.ore_last_error()
    # ORE_EINVAL comes before any launch, so the refusals can be seen without a device: the addresses are never read
    st, rows, ids, ws = 0x100000, 0x200000, 0x300000, 0x1000000
    ok_bytes = L.ore_track_wide_workspace_bytes(2000, 400)
    ok = dict(state=st, capacity=2000, n_host=8, max_rows=400, score=0.0, iou=0.6, ttl=8, ids=ids, ws=ws, ws_bytes=ok_bytes)
    for bad in (dict(capacity=0), dict(capacity=16385), dict(max_rows=8193), dict(max_rows=-1), dict(n_host=-1), dict(ttl=0), dict(ttl=(1 << 20) + 1),
                dict(iou=-0.1), dict(iou=float("nan")), dict(iou=float("inf")), dict(score=float("nan")), dict(state=0), dict(state=st + 8),
                dict(ids=0), dict(ids=st + 64), dict(ids=rows), dict(state=rows + 16), dict(ws=0), dict(ws=ws + 128), dict(ws_bytes=ok_bytes - 1), dict(ws_bytes=0), dict(ws=st), dict(ws=rows)):
        a = dict(ok, **bad)
        rc = L.ore_track_wide_update_fwd(a["state"], a["capacity"], rows, rows + 0x2000, rows + 0x4000, None, a["n_host"], a["max_rows"], a["score"],
                                         a["iou"], a["ttl"], 1, a["ids"], a["ws"], a["ws_bytes"], None)
        assert rc == -22 and L.ore_last_error().startswith(b"ore_track_wide_update_fwd"), (bad, rc)
    sig = inspect.signature(ore.WideBoxTracker.__init__).parameters
    assert {k: sig[k].default for k in ore.TRACK_WIDE_DEFAULTS} == ore.TRACK_WIDE_DEFAULTS == {
        "capacity": 4096, "max_rows": 2048, "iou_thresh": 0.6, "ttl": 8, "class_aware": True, "score_thresh": 0.0}
    assert "wide" in inspect.signature(ore.track_host).parameters


def test_wiring_surfaces(ore):
    import inspect
    from detectron2.modeling import GeneralizedRCNNWithTTA
    from fewx.modeling import TiledInference
    from predictor import TiledPredictor
    for cls in (TiledInference, GeneralizedRCNNWithTTA):
        assert inspect.signature(cls.__init__).parameters["track"].default is None and callable(cls.track_stats)
    assert callable(TiledPredictor.track_stats)
