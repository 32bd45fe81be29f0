"""GPU: test-time augmentation on the device (csrc/ore_tta.hip, detectron2/modeling/test_time_augmentation.py) against a host
composition of parts that are pinned elsewhere: Pillow's resize for the variants, the model's own `inference(do_postprocess=False)`
per variant, the numpy inverse transforms (tests/test_tta_host.py) and the host merge with the oracle's NMS per class."""
import numpy as np
import pytest
import torch

from conftest import rel_err
from oracle import decode as odec
from oracle import ref_model as R
from test_hip_resize import _cfg, _load, _support_dict, random_image, ramp_image, raw_image
from test_resize_host import PAIRS, pil_resize

pytestmark = pytest.mark.gpu

MIN_SIZES, MAX_SIZE = [256, 320, 416], 640
RAW_SIZES = [(480, 640), (300, 500)]
AUG = ["TEST.AUG.MIN_SIZES", MIN_SIZES, "TEST.AUG.MAX_SIZE", MAX_SIZE]


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


def T():
    from detectron2.modeling import test_time_augmentation
    return test_time_augmentation


def fields(out):
    i = out["instances"]
    return i.image_size, i.pred_boxes.tensor, i.scores, i.pred_classes


# ------------------------------------------------------------------------------------------ the flipped variant
@pytest.mark.parametrize("hw,nhw", PAIRS, ids=["%dx%d-%dx%d" % (a + b) for a, b in PAIRS])
def test_flipped_resize_equals_pillow(ore, hw, nhw):
    """resize + tta_hflip_u8 == Pillow's resize with the columns reversed, byte for byte, behind either form of the resize, with the
    bytes around the output untouched."""
    (h, w), (nh, nw) = hw, nhw
    forms = [ore.resize_form(h, w, nh, nw)]
    if forms[0] == ore.RESIZE_FORM_LDS:
        forms.append(ore.RESIZE_FORM_WORKSPACE)
    for img in (random_image(h, w), ramp_image(h, w)):
        want = np.ascontiguousarray(pil_resize(img, nh, nw)[:, ::-1].transpose(2, 0, 1))
        for form in forms:
            plain = ore.resize_bilinear_u8(torch.from_numpy(img).cuda(), nh, nw, form=form)
            n, band = 3 * nh * nw, 4096
            buf = torch.full((n + 2 * band,), 0xA5, dtype=torch.uint8, device="cuda")
            out = buf[band:band + n].view(3, nh, nw)
            assert ore.tta_hflip_u8(plain, out=out).data_ptr() == out.data_ptr()
            host = buf.cpu().numpy()
            assert (host[:band] == 0xA5).all() and (host[band + n:] == 0xA5).all(), "bytes outside the output were written"
            diff = int((host[band:band + n].reshape(3, nh, nw) != want).sum())
            print(f"{h}x{w}->{nh}x{nw} flipped, form {form}: {diff} differing bytes")
            assert diff == 0


# ------------------------------------------------------------------------------------------ the reference composition
def iou32(a, b):
    """IoU of box a with boxes b in fp32, the operation order of oracle/ref_decode.c."""
    xx1, yy1 = np.maximum(a[0], b[:, 0]), np.maximum(a[1], b[:, 1])
    xx2, yy2 = np.minimum(a[2], b[:, 2]), np.minimum(a[3], b[:, 3])
    inter = np.maximum(np.float32(0), xx2 - xx1) * np.maximum(np.float32(0), yy2 - yy1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter / ((a[2] - a[0]) * (a[3] - a[1]) + (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]) - inter)


def compose(model, kind, src, out_hw, aug, nms_thresh, topk, swap=False):
    """The host composition.  kind "raw": src [h, w, 3]; "image": src [3, h, w].  Returns the merged rows and the intermediate lists
    the non-triviality assertions read: per candidate its variant, the variants' flip flags, the candidates that survive NMS."""
    t = T()
    hwc = src if kind == "raw" else np.ascontiguousarray(src.transpose(1, 2, 0))
    if swap:
        hwc = np.ascontiguousarray(hwc[:, :, ::-1])
    h, w = hwc.shape[:2]
    variants = t.tta_variants(h, w, *aug)
    per_variant, boxes, scores, classes, cand_var = [], [], [], [], []
    for i, v in enumerate(variants):
        img = pil_resize(hwc, v["h"], v["w"])
        img = img[:, ::-1] if v["flip"] else img
        r = model.inference([{"image": torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1)))}], do_postprocess=False)[0]
        assert r.image_size == (v["h"], v["w"])
        b = t.inverse_boxes(r.pred_boxes.tensor.cpu().numpy(), t.variant_transforms(out_hw, (h, w), v))
        per_variant.append((b, r.scores.cpu().numpy(), r.pred_classes.cpu().numpy()))
        boxes.append(b), scores.append(per_variant[-1][1]), classes.append(per_variant[-1][2]), cand_var.extend([i] * len(b))
    boxes, scores, classes = np.concatenate(boxes), np.concatenate(scores), np.concatenate(classes)
    mb, ms, mc, midx = t.merge_detections_host(boxes, scores, classes, out_hw, 1e-8, nms_thresh, topk, nms=odec.nms)
    _, _, _, survivors = t.merge_detections_host(boxes, scores, classes, out_hw, 1e-8, nms_thresh, len(scores) + 1, nms=odec.nms)
    return dict(boxes=mb, scores=ms, classes=mc, idx=midx, survivors=survivors, cand_var=np.asarray(cand_var), variants=variants,
                per_variant=per_variant, cand=(boxes, scores, classes), out_hw=tuple(out_hw), nms_thresh=nms_thresh)


def cross_variant_suppressions(ref):
    """Candidates that a survivor of ANOTHER variant suppresses: replayed greedily from the reference's own lists (clipped boxes, score
    order, same class, IoU > threshold in fp32)."""
    boxes, scores, classes = ref["cand"]
    h, w = np.float32(ref["out_hw"][0]), np.float32(ref["out_hw"][1])
    b = boxes.copy()
    b[:, 0::2] = np.minimum(np.maximum(b[:, 0::2], np.float32(0)), w)
    b[:, 1::2] = np.minimum(np.maximum(b[:, 1::2], np.float32(0)), h)
    surv = ref["survivors"]
    dead = np.setdiff1d(np.nonzero(np.isfinite(boxes).all(1) & np.isfinite(scores) & (scores > np.float32(1e-8)))[0], surv)
    n = 0
    for j in dead:
        ahead = surv[(classes[surv] == classes[j]) & ((scores[surv] > scores[j]) | ((scores[surv] == scores[j]) & (surv < j)))]
        hit = ahead[iou32(b[j], b[ahead]) > np.float32(ref["nms_thresh"])]
        assert len(hit), "a candidate that did not survive has no suppressor among the survivors"
        n += int(ref["cand_var"][hit[0]] != ref["cand_var"][j])
    return n, len(dead)


def describe(ref, tag):
    sv = ref["cand_var"][ref["idx"]]
    flips = np.asarray([v["flip"] for v in ref["variants"]])
    cross, dead = cross_variant_suppressions(ref)
    info = dict(rows_per_variant=[len(p[1]) for p in ref["per_variant"]], merged=len(ref["idx"]), survivors=len(ref["survivors"]),
                from_variants=sorted(set(sv.tolist())), flipped=int(flips[sv].sum()), plain=int((~flips[sv]).sum()), suppressed=dead,
                suppressed_by_other_variant=cross)
    print(f"[tta reference] {tag}: {info}")
    return info


def assert_not_trivial(info, flip=True):
    """The conditions the reference composition has to show (on its own lists, not on the code under test)."""
    assert len(info["from_variants"]) >= 2, info
    if flip:
        assert info["flipped"] >= 1 and info["plain"] >= 1, info
    assert info["suppressed_by_other_variant"] >= 1, info


def assert_equal(got, ref):
    size, boxes, scores, classes = fields(got)
    assert size == ref["out_hw"]
    for a, b, name in ((boxes, ref["boxes"], "boxes"), (scores, ref["scores"], "scores"), (classes, ref["classes"], "classes")):
        b = torch.from_numpy(np.ascontiguousarray(b))
        a = a.cpu()
        if not torch.equal(a, b):
            rows = (a != b).reshape(len(a), -1).any(1).nonzero().flatten().tolist() if a.shape == b.shape else "shapes %s / %s" % (a.shape, b.shape)
            raise AssertionError(f"{name} differ in rows {rows}")


def tta_cfg(extra=(), flip=True):
    return _cfg(AUG + ["TEST.AUG.FLIP", flip] + list(extra))


def wrapper(model, cfg):
    from detectron2.modeling import GeneralizedRCNNWithTTA
    return GeneralizedRCNNWithTTA(cfg, model)


# ------------------------------------------------------------------------------------------ collection
@pytest.mark.parametrize("hw", RAW_SIZES, ids=lambda v: "%dx%d" % v)
def test_collect_equals_numpy_inverse(ore, model, hw):
    """After one device-path call the pool holds, variant after variant, the numpy inverse of the rows the model returns for that
    variant image, the scores and class ids as they were, and the per-variant counts."""
    raw = raw_image(140 + hw[0], *hw)
    cfg = tta_cfg()
    out_hw = (hw[0] + 40, hw[1] + 70)                          # "image" request with another output size: the pre-transform is in the chain
    chw = np.ascontiguousarray(raw.transpose(2, 0, 1))
    for kind, req, src, ohw in (("raw", {"image_raw": raw}, raw, hw),
                                ("image", {"image": torch.from_numpy(chw), "height": out_hw[0], "width": out_hw[1]}, chw, out_hw)):
        ref = compose(model, kind, src, ohw, (MIN_SIZES, MAX_SIZE, True), cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST, cfg.TEST.DETECTIONS_PER_IMAGE)
        tta = wrapper(model, cfg)
        p = tta._enqueue(req)
        torch.cuda.synchronize()
        counts = p.pool.var_counts.cpu().tolist()
        print(f"[tta collect] {kind} {hw}: rows per variant {counts}")
        assert counts == [len(s) for _, s, _ in ref["per_variant"]] and int(p.pool.n.item()) == sum(counts) and sum(counts) > 0
        n = sum(counts)
        for got, want in zip((p.pool.boxes[:n], p.pool.scores[:n], p.pool.classes[:n]), ref["cand"]):
            assert torch.equal(got.cpu(), torch.from_numpy(np.ascontiguousarray(want)))
        assert_equal(tta._finish(p), ref)


# ------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("hw", RAW_SIZES, ids=lambda v: "%dx%d" % v)
def test_tta_equals_host_composition_raw(model, hw):
    """The acceptance test, "image_raw" requests: numpy array, CPU tensor, device tensor, an explicit output size, channel swap."""
    raw = raw_image(31 + hw[0], *hw)
    cfg = tta_cfg()
    aug, thr, topk = (MIN_SIZES, MAX_SIZE, True), cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST, cfg.TEST.DETECTIONS_PER_IMAGE
    ref = compose(model, "raw", raw, hw, aug, thr, topk)
    assert_not_trivial(describe(ref, f"raw {hw}"))
    tta = wrapper(model, cfg)
    for form in (raw, torch.from_numpy(raw), torch.from_numpy(raw).cuda()):
        assert_equal(tta([{"image_raw": form}])[0], ref)
    assert_equal(tta([{"image_raw": raw, "height": 200, "width": 300}])[0], compose(model, "raw", raw, (200, 300), aug, thr, topk))
    assert_equal(tta([{"image_raw": raw, "swap_rb": True}])[0], compose(model, "raw", raw, hw, aug, thr, topk, swap=True))


@pytest.mark.parametrize("flip", [True, False])
def test_tta_equals_host_composition_image(model, flip):
    """An "image" request (the mapper-resized image) whose output size differs: variants are resized from that image and the
    pre-transform is part of the chain; flip on and off."""
    raw = raw_image(57, 360, 500)
    nh, nw = 320, 444
    chw = np.ascontiguousarray(pil_resize(raw, nh, nw).transpose(2, 0, 1))
    cfg = tta_cfg(flip=flip)
    ref = compose(model, "image", chw, (360, 500), (MIN_SIZES, MAX_SIZE, flip), cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST, cfg.TEST.DETECTIONS_PER_IMAGE)
    assert len(ref["variants"]) == (6 if flip else 3)
    assert_not_trivial(describe(ref, f"image flip={flip}"), flip)
    tta = wrapper(model, cfg)
    for img in (torch.from_numpy(chw), torch.from_numpy(chw).cuda()):
        assert_equal(tta([{"image": img, "height": 360, "width": 500}])[0], ref)


def test_tta_topk_cut(model):
    """TEST.DETECTIONS_PER_IMAGE = 10: more candidates survive the NMS than that, so the cut acts."""
    raw = raw_image(31 + 480, 480, 640)
    cfg = tta_cfg(["TEST.DETECTIONS_PER_IMAGE", 10])
    ref = compose(model, "raw", raw, (480, 640), (MIN_SIZES, MAX_SIZE, True), cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST, 10)
    info = describe(ref, "topk 10")
    assert info["survivors"] > 10 and info["merged"] == 10, info
    assert_equal(wrapper(model, cfg)([{"image_raw": raw}])[0], ref)


def test_tta_nway(model):
    """support_classes = "all" over two support classes: per variant the N-way rows with their class ids (one poll per variant)."""
    raw = raw_image(91, 300, 500)
    cfg = tta_cfg()
    model.set_support_dict(_support_dict((3, 8)))
    model.support_classes = "all"
    try:
        ref = compose(model, "raw", raw, (300, 500), (MIN_SIZES, MAX_SIZE, True), cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST, cfg.TEST.DETECTIONS_PER_IMAGE)
        info = describe(ref, "n-way")
        got = wrapper(model, cfg)([{"image_raw": raw}])[0]
    finally:
        model.support_classes = None
        model.set_support_dict(_support_dict())
    assert set(ref["cand"][2].tolist()) == {3, 8} and set(ref["classes"].tolist()) <= {3, 8}
    assert len(info["from_variants"]) >= 2 and info["merged"] > 0, info
    assert_equal(got, ref)


def test_tta_host_path_with_custom_mapper(model):
    """A custom mapper takes the host path (mapper -> model -> merge kernel); given the default mapper's variants it returns the same."""
    from detectron2.modeling import DatasetMapperTTA, GeneralizedRCNNWithTTA
    raw = raw_image(31 + 300, 300, 500)
    cfg = tta_cfg()
    ref = compose(model, "raw", raw, (300, 500), (MIN_SIZES, MAX_SIZE, True), cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST, cfg.TEST.DETECTIONS_PER_IMAGE)
    tta = GeneralizedRCNNWithTTA(cfg, model, tta_mapper=DatasetMapperTTA(cfg))
    assert not tta.device_path
    assert_equal(tta([{"image_raw": raw}])[0], ref)


def test_tta_file_name_request(model, tmp_path):
    """A request with only "file_name" is read in the model's input format (BGR), as `_maybe_read_image` does, and then equals the
    "image_raw" request of the same pixels."""
    from PIL import Image
    raw = raw_image(31 + 300, 300, 500)
    path = str(tmp_path / "q.png")
    Image.fromarray(np.ascontiguousarray(raw[:, :, ::-1])).save(path)      # the file holds RGB
    tta = wrapper(model, tta_cfg())
    a, b = tta([{"file_name": path}])[0], tta([{"image_raw": raw}])[0]
    assert all(x == y if isinstance(x, tuple) else torch.equal(x, y) for x, y in zip(fields(a), fields(b))) and len(fields(a)[2]) > 0
    assert fields(a)[0] == (300, 500)


# ------------------------------------------------------------------------------------------ one sync, reproducibility, rebuild
def test_tta_device_path_issues_no_sync(model):
    """Everything up to the merged record is enqueued without a host synchronisation torch knows of (sync debug mode "error": .item(),
    .cpu(), blocking copies and stream / device synchronisation raise); the count read that follows is the one wait."""
    raw = torch.from_numpy(raw_image(31 + 480, 480, 640)).cuda()
    tta = wrapper(model, tta_cfg())
    want = tta([{"image_raw": raw}])[0]                        # engine, graphs, tables, pool: built outside the measured call
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):                      # the mode is live: a read-back raises
            torch.ones(1, device="cuda").item()
        p = tta._enqueue({"image_raw": raw})
    finally:
        torch.cuda.set_sync_debug_mode("default")
    got = tta._finish(p)
    for a, b in zip(fields(got), fields(want)):
        assert a == b if isinstance(a, tuple) else torch.equal(a, b)
    assert len(fields(got)[2]) > 0


def test_tta_reproducible_and_engine_rebuilt_on_weight_edit(model):
    """Two calls on one request are torch.equal; a weight edit between calls changes the result (the wrapper's engine is rebuilt) and
    undoing it brings the first result back; the model's own cached engine is not the wrapper's."""
    raw = raw_image(31 + 300, 300, 500)
    tta = wrapper(model, tta_cfg())
    a, b = tta([{"image_raw": raw}])[0], tta([{"image_raw": raw}])[0]
    assert all(x == y if isinstance(x, tuple) else torch.equal(x, y) for x, y in zip(fields(a), fields(b))) and len(fields(a)[2]) > 0
    e0 = tta._tta_engine
    assert e0 is not None and e0 is not model._engine
    w = model.conv3.weight
    saved = w.detach().clone()
    try:
        with torch.no_grad():
            w.mul_(0.5)
        c = tta([{"image_raw": raw}])[0]
        assert tta._tta_engine is not e0
        assert not (fields(c)[1].shape == fields(a)[1].shape and torch.equal(fields(c)[1], fields(a)[1]) and torch.equal(fields(c)[2], fields(a)[2]))
    finally:
        with torch.no_grad():
            w.copy_(saved)
    d = tta([{"image_raw": raw}])[0]
    assert all(x == y if isinstance(x, tuple) else torch.equal(x, y) for x, y in zip(fields(d), fields(a)))


# ------------------------------------------------------------------------------------------ the default config: 18 variants up to 1200x1200
def test_tta_default_config_300x300(model):
    """TEST.AUG as shipped (MIN_SIZES 400 .. 1200, MAX_SIZE 4000, flip) on a 300x300 image: 18 variants, the largest 1200x1200 --
    beyond INPUT.MAX_SIZE_TEST, so the model's own engine (the reference's per-variant path) is sized up for the composition."""
    raw = raw_image(77, 300, 300)
    cfg = _cfg()
    aug = (list(cfg.TEST.AUG.MIN_SIZES), cfg.TEST.AUG.MAX_SIZE, cfg.TEST.AUG.FLIP)
    assert aug == ([400, 500, 600, 700, 800, 900, 1000, 1100, 1200], 4000, True)
    tta = wrapper(model, cfg)
    got = tta([{"image_raw": raw}])[0]
    assert tta._tta_engine_hw == (1200, 1200)
    saved = model.max_hw
    model.max_hw = (1200, 1200)
    model._engine_key = None                                   # the composition's engine: rebuilt at the larger size
    try:
        ref = compose(model, "raw", raw, (300, 300), aug, cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST, cfg.TEST.DETECTIONS_PER_IMAGE)
    finally:
        model.max_hw = saved
        model._engine_key = None
    assert len(ref["variants"]) == 18 and (ref["variants"][-1]["h"], ref["variants"][-1]["w"]) == (1200, 1200)
    describe(ref, "default 300x300")
    assert_equal(got, ref)


def test_engine_dense_maps_at_1200(ore):
    """The dense maps of a 1200x1200 pass (padded to 1216) against the CPU oracle within the 1e-4 gate of the other sizes: the engine
    had not been exercised above 1000."""
    sd = R.synth_state_dict(0)
    img = torch.from_numpy(np.ascontiguousarray(pil_resize(raw_image(77, 300, 300), 1200, 1200).transpose(2, 0, 1)))
    ref = R.eval_dense(img, sd, R.synth_support(0))
    e = ore.Engine(max_batch=1, max_h=1200, max_w=1200)
    e.load_state_dict(sd)
    e.set_support(R.synth_support(0))
    e.finalize()
    try:
        worst = {}
        for use_graph in (False, True):
            e.eval_forward(img.cuda(), use_graph=use_graph)
            torch.cuda.synchronize()
            for l, k in enumerate(("p3", "p4", "p5")):
                s = 1216 >> (l + 3)
                worst[k, use_graph] = rel_err(e.buffer(k, (1, s, s)).cpu().numpy(), ref["features"][k].numpy())
                hd = e.buffer(f"head{l + 3}", (1, s, s)).cpu()
                worst["hm", l, use_graph] = rel_err(hd[:, 4:5].numpy(), ref["hm"][l].numpy())
                worst["reg", l, use_graph] = rel_err(hd[:, :4].numpy(), ref["reg"][l].numpy())
        print("[tta 1200x1200 dense parity]", {str(k): "%.2e" % v for k, v in worst.items()})
        assert max(worst.values()) < 1e-4, worst
    finally:
        e.close()
