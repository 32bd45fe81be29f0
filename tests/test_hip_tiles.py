"""GPU: tiled inference on the device (csrc/ore_tile.hip, fewx/modeling/tiled_inference.py) against tests/tile_ref.py and a host
composition of parts that are pinned elsewhere: numpy crops and Pillow's resize for the sources, the model's own
`inference(do_postprocess=False)` / `inference_many` per source, the reference seam rule and transform, and the host merge with the
oracle's NMS per class."""
import numpy as np
import pytest
import torch

import tile_ref
from oracle import decode as odec
from test_hip_resize import _cfg, _load, _support_dict, raw_image
from test_hip_tta import assert_equal, cross_variant_suppressions, fields
from test_resize_host import pil_resize

pytestmark = pytest.mark.gpu


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


# ------------------------------------------------------------------------------------------ the gather
GATHER_CASES = [((67, 101), (64, 64), 16), ((130, 257), (96, 128), 32), ((64, 64), (64, 64), 0), ((50, 300), (64, 128), 32),
                ((300, 500), (160, 160), 40)]


def frame_at_offset(img, off):
    """The frame as a device tensor that starts `off` bytes into an allocation of its own."""
    n = img.size
    buf = torch.empty(off + n, dtype=torch.uint8, device="cuda")
    src = buf[off:off + n].view(img.shape)
    src.copy_(torch.from_numpy(img))
    return src


def guarded_gather(ore_, src, plan, swap):
    n_t, th, tw = plan["ny"] * plan["nx"], plan["th"], plan["tw"]
    n, band = n_t * 3 * th * tw, 4096
    for lead in (0, 3):                                       # the output 16-byte aligned and not
        buf = torch.full((n + 2 * band + lead,), 0xA5, dtype=torch.uint8, device="cuda")
        out = buf[band + lead:band + lead + n].view(n_t, 3, th, tw)
        got = ore_.tile_gather_u8(src, plan, swap_rb=swap, out=out)
        assert got.data_ptr() == out.data_ptr()
        host = buf.cpu().numpy()
        assert (host[:band + lead] == 0xA5).all() and (host[band + lead + n:] == 0xA5).all(), "bytes outside the output were written"
        yield host[band + lead:band + lead + n].reshape(n_t, 3, th, tw)


@pytest.mark.parametrize("hw,tile,overlap", GATHER_CASES, ids=["%dx%d-%dx%d-%d" % (a + b + (c,)) for a, b, c in GATHER_CASES])
def test_gather_equals_numpy_slicing(ore, hw, tile, overlap):
    """Byte for byte numpy slicing, channel swap off and on, the source at an aligned and at odd byte offsets, into the middle of a buffer of 0xA5 bytes whose guard bands stay untouched."""
    h, w = hw
    img = np.random.default_rng(h * 10007 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    plan = ore.tile_plan(h, w, tile, (overlap, overlap))
    assert plan == tile_ref.plan(h, w, tile, (overlap, overlap))
    if hw == (67, 101):
        assert plan["origins"] == [(0, 0), (0, 37), (3, 0), (3, 37)]
    if hw == (50, 300):
        assert (plan["th"], plan["tw"]) == (50, 128)
    if hw == (300, 500):
        assert (plan["ny"], plan["nx"]) == (3, 4)
    for off in (0, 1, 7):
        src = frame_at_offset(img, off)
        for swap in (False, True):
            want = tile_ref.gather(img, plan, swap)
            for got in guarded_gather(ore, src, plan, swap):
                diff = int((got != want).sum())
                print(f"gather {h}x{w} tile {tile} overlap {overlap} offset {off} swap {swap}: {diff} differing bytes")
                assert diff == 0
    assert np.array_equal(ore.tile_gather_host(img, plan, True), tile_ref.gather(img, plan, True))


def test_gather_wide_tile_on_a_side_stream(ore):
    """A tile wider than one block's 1024 columns, more rows than a block's four, on a side stream."""
    h, w = 37, 2500
    img = np.random.default_rng(11).integers(0, 256, (h, w, 3), dtype=np.uint8)
    plan = ore.tile_plan(h, w, (33, 2051), (5, 1700))
    assert (plan["ny"], plan["nx"], plan["tw"]) == (2, 3, 2051)
    src = frame_at_offset(img, 5)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = ore.tile_gather_u8(src, plan)
    s.synchronize()
    assert np.array_equal(got.cpu().numpy(), tile_ref.gather(img, plan))


def test_gather_refuses_bad_arguments(ore):
    src = torch.zeros(100, 120, 3, dtype=torch.uint8, device="cuda")
    good = ore.tile_plan(100, 120, (64, 64), (16, 16))
    for edit in (dict(th=101), dict(tw=121), dict(th=0), dict(stride_y=0), dict(ny=1), dict(nx=1), dict(ny=16, nx=9)):
        with pytest.raises(ore.OreError, match="ore_tile_gather_u8_fwd"):
            ore.tile_gather_u8(src, dict(good, **edit))
    buf = torch.zeros(2 * 100 * 120 * 3, dtype=torch.uint8, device="cuda")
    one = ore.tile_plan(100, 120, (100, 120), (0, 0))
    with pytest.raises(ore.OreError, match="overlaps"):
        ore.tile_gather_u8(buf[:36000].view(100, 120, 3), one, out=buf[35999:71999].view(1, 3, 100, 120))
    ore.tile_gather_u8(buf[:36000].view(100, 120, 3), one, out=buf[36000:].view(1, 3, 100, 120))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ the collection
def same_bits(a, b):
    """torch.equal with a NaN equal to a NaN in the same place."""
    a, b = a.cpu(), torch.from_numpy(np.ascontiguousarray(b))
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(torch.isnan(a), torch.isnan(b)) and \
        torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))


@pytest.mark.parametrize("edges", range(16))
def test_collect_equals_reference(ore, edges):
    """Three sources of 320 hand-made rows appended in turn -- a tile with a device count, a tile with a host count (beyond max_rows:
    cut to it), the scaled full-frame form with a device count -- for every `edges` value: src_counts, src_dropped, the running count,
    the pool order and every value."""
    ROWS = 320
    specs = [((256, 320), 2.0, dict(sx=1.0, sy=1.0, ox=192.0, oy=37.0), "dev", 300),
             ((300, 333), 2.5, dict(sx=1.0, sy=1.0, ox=3200.0, oy=1520.0), "host", 400),
             ((320, 427), 1.0, dict(sx=640 / 427, sy=480 / 320, ox=0.0, oy=0.0), "dev", 320)]
    pool = ore.TilePool(3, ROWS, "cuda")
    want_b, want_s, want_c, counts, dropped = [], [], [], [], []
    for source, (src_hw, margin, tf, how, n) in enumerate(specs):
        boxes, scores, classes = tile_ref.hand_rows(ROWS, src_hw, margin, seed=100 * edges + source)
        take = min(n, ROWS)
        b, s, c, idx, drop = tile_ref.collect(boxes[:take], scores[:take], classes[:take] if source != 1 else None, src_hw=src_hw, edges=edges,
                                              margin=margin, **tf)
        want_b.append(b), want_s.append(s), want_c.append(c), counts.append(len(idx)), dropped.append(drop)
        n_arg = torch.tensor([n], dtype=torch.int32, device="cuda") if how == "dev" else n
        ore.tile_collect(pool, source, torch.from_numpy(boxes).cuda(), torch.from_numpy(scores).cuda(),
                         torch.from_numpy(classes).cuda() if source != 1 else None, n_arg, ROWS, src_hw=src_hw, edges=edges, margin=margin, **tf)
        # the host statement of the binding agrees with the reference as well
        hb, hs, hc, kept = ore.tile_collect_host(boxes[:take], scores[:take], classes[:take] if source != 1 else None, src_hw=src_hw, edges=edges,
                                                 margin=margin, **tf)
        assert np.array_equal(np.nonzero(kept)[0], idx) and hb.tobytes() == b.tobytes()
    torch.cuda.synchronize()
    total = sum(counts)
    print(f"[tile collect] edges {edges}: kept {counts}, rejected {dropped}")
    assert torch.equal(pool.src_counts.cpu(), torch.tensor(counts, dtype=torch.int32))
    assert torch.equal(pool.src_dropped.cpu(), torch.tensor(dropped, dtype=torch.int32))
    assert int(pool.n.item()) == total and total > 0
    assert (sum(dropped) == 0) == (edges == 0)
    assert same_bits(pool.boxes[:total], np.concatenate(want_b))
    assert same_bits(pool.scores[:total], np.concatenate(want_s))
    assert torch.equal(pool.classes[:total].cpu(), torch.from_numpy(np.concatenate(want_c)))
    # source 0 again restarts the pool
    boxes, scores, classes = tile_ref.hand_rows(ROWS, (256, 320), 2.0, seed=100 * edges)
    ore.tile_collect(pool, 0, torch.from_numpy(boxes).cuda(), torch.from_numpy(scores).cuda(), None, 10, ROWS, src_hw=(256, 320), edges=0,
                     margin=2.0, **specs[0][2])
    assert int(pool.n.item()) == 10 and pool.src_counts.cpu().tolist()[0] == 10


def test_collect_cuts_at_the_pool(ore):
    """Rows that would pass pool_cap are cut; the count stops at the capacity."""
    pool = ore.TilePool(2, 100, "cuda")
    boxes, scores, classes = tile_ref.hand_rows(320, (256, 320), 2.0, seed=3)
    args = (torch.from_numpy(boxes).cuda(), torch.from_numpy(scores).cuda(), torch.from_numpy(classes).cuda())
    kw = dict(sx=1.0, sy=1.0, ox=0.0, oy=0.0, src_hw=(256, 320), edges=0, margin=2.0)
    ore.tile_collect(pool, 0, *args, 150, 320, **kw)
    ore.tile_collect(pool, 1, *args, 150, 320, **kw)
    assert int(pool.n.item()) == 200 and pool.src_counts.cpu().tolist() == [150, 50]
    assert same_bits(pool.boxes, np.concatenate([boxes[:150], boxes[:50]]))


# ------------------------------------------------------------------------------------------ the reference composition
def compose(model, frame, tile, overlap, margin, full_frame, fold, nms_thresh, topk, swap=False):
    """The host composition: numpy crops plus Pillow's resize -> the model per source (fold == 1: `inference`; fold > 1: the tiles
    through `inference_many(max_fold=fold)`) -> tests/tile_ref.py's seam rule and transform -> merge_detections_host with the oracle's
    NMS.  Returns the merged rows and the lists the non-triviality assertions read."""
    import orehip
    from detectron2.modeling.test_time_augmentation import merge_detections_host
    h, w = frame.shape[:2]
    plan = tile_ref.plan(h, w, tile, overlap)
    full_hw = orehip.resize_shortest_edge_shape(h, w, *model._test_size) if full_frame else None
    srcs = tile_ref.sources(frame, plan, full_hw, pil_resize, swap)
    reqs = [{"image": torch.from_numpy(np.ascontiguousarray(s["image"]))} for s in srcs]
    first = 1 if full_frame else 0
    if fold > 1:
        res = [model.inference([r], do_postprocess=False)[0] for r in reqs[:first]]
        res += model.inference_many(reqs[first:], do_postprocess=False, max_fold=fold)
    else:
        res = [model.inference([r], do_postprocess=False)[0] for r in reqs]
    boxes, scores, classes, cand_src, per_source, rejected = [], [], [], [], [], []
    for i, (s, r) in enumerate(zip(srcs, res)):
        assert r.image_size == tuple(s["src_hw"])
        b, sc, c, idx, drop = tile_ref.collect(r.pred_boxes.tensor.cpu().numpy(), r.scores.cpu().numpy(), r.pred_classes.cpu().numpy(), s["sx"],
                                               s["sy"], s["ox"], s["oy"], s["src_hw"], s["edges"], margin)
        boxes.append(b), scores.append(sc), classes.append(c), cand_src.extend([i] * len(idx))
        per_source.append(len(idx)), rejected.append(drop)
    boxes, scores, classes = np.concatenate(boxes), np.concatenate(scores), np.concatenate(classes)
    mb, ms, mc, midx = merge_detections_host(boxes, scores, classes, (h, w), 1e-8, nms_thresh, topk, nms=odec.nms)
    _, _, _, survivors = merge_detections_host(boxes, scores, classes, (h, w), 1e-8, nms_thresh, len(scores) + 1, nms=odec.nms)
    return dict(boxes=mb, scores=ms, classes=mc, idx=midx, survivors=survivors, cand_var=np.asarray(cand_src), cand=(boxes, scores, classes),
                out_hw=(h, w), nms_thresh=nms_thresh, per_source=per_source, rejected=rejected, plan=plan, full_hw=full_hw)


def describe(ref, tag):
    cross, dead = cross_variant_suppressions(ref)
    info = dict(kept_per_source=ref["per_source"], rejected_per_source=ref["rejected"], merged=len(ref["idx"]), survivors=len(ref["survivors"]),
                from_sources=sorted(set(ref["cand_var"][ref["survivors"]].tolist())), suppressed=dead, suppressed_by_other_source=cross)
    print(f"[tiles reference] {tag}: {info}")
    return info


def assert_not_trivial(info):
    """The conditions the reference composition has to show, on its own lists only."""
    assert len(info["from_sources"]) >= 2, info
    assert sum(info["rejected_per_source"]) >= 1, info
    assert info["suppressed_by_other_source"] >= 1, info


def tiled(model, cfg=None, **kw):
    from fewx.modeling import TiledInference
    return TiledInference(_cfg() if cfg is None else cfg, model, **kw)


def defaults(cfg):
    return float(cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST), int(cfg.TEST.DETECTIONS_PER_IMAGE)


SEED_480, SEED_300 = 31 + 480, 31 + 300


# ------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("fold", [1, 4])
def test_tiled_equals_host_composition_480x640(model, fold):
    """480x640, tile 256, overlap 64: 9 tiles plus the full frame; one tile per pass and four.  After the call the pool holds the
    reference's candidates source after source."""
    raw = raw_image(SEED_480, 480, 640)
    cfg = _cfg()
    thr, topk = defaults(cfg)
    ref = compose(model, raw, (256, 256), (64, 64), 2.0, True, fold, thr, topk)
    assert len(ref["plan"]["origins"]) == 9 and ref["full_hw"] == (320, 427)
    assert_not_trivial(describe(ref, f"480x640 fold {fold}"))
    t = tiled(model, cfg, tile=(256, 256), overlap=64, fold=fold)
    p = t._enqueue({"image_raw": raw})
    torch.cuda.synchronize()
    assert p.pool.src_counts.cpu().tolist() == ref["per_source"] and p.pool.src_dropped.cpu().tolist() == ref["rejected"]
    n = sum(ref["per_source"])
    assert int(p.pool.n.item()) == n
    for got, want in zip((p.pool.boxes[:n], p.pool.scores[:n], p.pool.classes[:n]), ref["cand"]):
        assert torch.equal(got.cpu(), torch.from_numpy(np.ascontiguousarray(want)))
    assert_equal(t._finish(p), ref)
    assert t._slots["tile"].engine is not model._engine and t._slots["full"].engine is not model._engine
    for form in (torch.from_numpy(raw), torch.from_numpy(raw).cuda()):
        assert_equal(t([{"image_raw": form, "height": 480, "width": 640}])[0], ref)


def test_tiled_equals_host_composition_300x500(model, tmp_path):
    """300x500, tile 320, overlap 96: 2 tiles of 300x320 (the extent is the frame's height); with and without the full-frame pass;
    the "image" and "file_name" forms of the request; channel swap."""
    from PIL import Image
    raw = raw_image(SEED_300, 300, 500)
    cfg = _cfg()
    thr, topk = defaults(cfg)
    ref = compose(model, raw, (320, 320), (96, 96), 2.0, True, 1, thr, topk)
    assert (ref["plan"]["th"], ref["plan"]["tw"], ref["plan"]["origins"]) == (300, 320, [(0, 0), (0, 180)])
    assert_not_trivial(describe(ref, "300x500"))
    t = tiled(model, cfg, tile=320, overlap=96)
    assert_equal(t([{"image_raw": raw}])[0], ref)
    assert_equal(t([{"image": torch.from_numpy(np.ascontiguousarray(raw.transpose(2, 0, 1)))}])[0], ref)
    path = str(tmp_path / "f.png")
    Image.fromarray(np.ascontiguousarray(raw[:, :, ::-1])).save(path)      # the file holds RGB; the model reads BGR
    assert_equal(t([{"file_name": path}])[0], ref)
    assert_equal(t([{"image_raw": raw, "swap_rb": True}])[0], compose(model, raw, (320, 320), (96, 96), 2.0, True, 1, thr, topk, swap=True))
    ref = compose(model, raw, (320, 320), (96, 96), 2.0, False, 1, thr, topk)
    info = describe(ref, "300x500 without the full frame")
    assert len(ref["per_source"]) == 2 and len(info["from_sources"]) == 2 and sum(info["rejected_per_source"]) >= 1, info
    assert_equal(tiled(model, cfg, tile=320, overlap=96, full_frame=False)([{"image_raw": raw}])[0], ref)


def test_tiled_max_detections(model):
    """max_detections = 400 instead of TEST.DETECTIONS_PER_IMAGE: the merge keeps up to 400 of the 10 sources' rows."""
    raw = raw_image(SEED_480, 480, 640)
    cfg = _cfg()
    thr, topk = defaults(cfg)
    ref = compose(model, raw, (256, 256), (64, 64), 2.0, True, 1, thr, 400)
    info = describe(ref, "max_detections 400")
    assert topk < info["merged"] <= 400, info
    assert_equal(tiled(model, cfg, tile=256, overlap=64, max_detections=400)([{"image_raw": raw}])[0], ref)


def test_tiled_nway(model):
    """support_classes = "all" over two support classes: per source the N-way rows with their class ids (one poll per source; fold is
    ignored)."""
    raw = raw_image(91, 300, 500)
    cfg = _cfg()
    thr, topk = defaults(cfg)
    model.set_support_dict(_support_dict((3, 8)))
    model.support_classes = "all"
    try:
        ref = compose(model, raw, (320, 320), (96, 96), 2.0, True, 1, thr, topk)
        info = describe(ref, "n-way")
        got = tiled(model, cfg, tile=320, overlap=96, fold=4)([{"image_raw": raw}])[0]
    finally:
        model.support_classes = None
        model.set_support_dict(_support_dict())
    assert set(ref["cand"][2].tolist()) == {3, 8} and set(ref["classes"].tolist()) <= {3, 8}
    assert len(info["from_sources"]) >= 2 and info["merged"] > 0, info
    assert_equal(got, ref)


@pytest.mark.parametrize("fmt", ["BGR", "RGB"])
def test_tiled_predictor(ore, fmt):
    """TiledPredictor: DefaultPredictor's contract (a BGR frame in, INPUT.FORMAT decides the swap) over the wrapper."""
    from predictor import TiledPredictor
    cfg = _cfg(["INPUT.FORMAT", fmt])
    pred = TiledPredictor(cfg, tile=320, overlap=96)
    _load(pred.model)
    assert pred.input_format == fmt and hasattr(pred, "metadata") and pred.tiled.model is pred.model
    raw = raw_image(SEED_300, 300, 500)
    thr, topk = defaults(cfg)
    ref = compose(pred.model, raw, (320, 320), (96, 96), 2.0, True, 1, thr, topk, swap=fmt == "RGB")
    assert len(ref["idx"]) > 0
    assert_equal(pred(raw), ref)
    assert_equal(pred(torch.from_numpy(raw).cuda()), ref)


# ------------------------------------------------------------------------------------------ one sync, reproducibility, rebuild
def test_tiled_device_path_issues_no_sync(model):
    """Everything up to the merged record is enqueued without a host synchronisation torch knows of (sync debug mode "error"); the
    count read that follows is the one wait.  fold 4: the batched passes."""
    raw = torch.from_numpy(raw_image(SEED_480, 480, 640)).cuda()
    t = tiled(model, tile=256, overlap=64, fold=4)
    want = t([{"image_raw": raw}])[0]                          # engines, graphs, tables, pool: built outside the measured call
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):                      # the mode is live: a read-back raises
            torch.ones(1, device="cuda").item()
        p = t._enqueue({"image_raw": raw})
    finally:
        torch.cuda.set_sync_debug_mode("default")
    got = t._finish(p)
    for a, b in zip(fields(got), fields(want)):
        assert a == b if isinstance(a, tuple) else torch.equal(a, b)
    assert len(fields(got)[2]) > 0


def test_tiled_engines_rebuilt_on_weight_edit(model):
    """A weight edit between calls changes the result (the wrapper's engines are rebuilt) and undoing it brings the first result back."""
    raw = raw_image(SEED_300, 300, 500)
    t = tiled(model, tile=320, overlap=96)
    a = t([{"image_raw": raw}])[0]
    e0 = t._slots["tile"].engine
    w = model.conv3.weight
    saved = w.detach().clone()
    try:
        with torch.no_grad():
            w.mul_(0.5)
        c = t([{"image_raw": raw}])[0]
        assert t._slots["tile"].engine is not e0
        assert not (fields(c)[1].shape == fields(a)[1].shape and torch.equal(fields(c)[1], fields(a)[1]) and torch.equal(fields(c)[2], fields(a)[2]))
    finally:
        with torch.no_grad():
            w.copy_(saved)
    d = t([{"image_raw": raw}])[0]
    assert all(x == y if isinstance(x, tuple) else torch.equal(x, y) for x, y in zip(fields(d), fields(a))) and len(fields(a)[2]) > 0
