"""GPU: every stage of CustomCascadeROIHeads (K = len(ROI_BOX_CASCADE_HEAD.IOUS) > 1): eval and training.

  * ore_roi_cascade_refine_fwd and ore_roi_predict_cascade_fwd through the C ABI against tests/cascade_ref.py (the C twin per stage, the
    numpy-fp32 mean, oracle.decode.nms), bit for bit, over its case table; n_stages = 1 against ore_roi_predict_parts_fwd;
  * ore_cascade_relabel_fwd against the numpy restatement;
  * the module path on the executed reference's three-stage fixture (tests/golden/cascade_stage_eval.npz); an orehip.Engine with the
    cascade -- one image, a folded batch of 3, N-way with 2 classes, fp32 and the bf16 modes -- against the module path on the
    engine's own proposals and pyramid (the fixture holds a pyramid, an engine starts from an image), K = 1 through the new setter
    against ore_engine_set_roi_head;
  * one training iteration at K = 3: the eager one-image form against cascade_stage_train.npz, the padded form against the eager one,
    GraphedTrainStep replays (one size, and a mixed-size batch) against eager steps, two runs bit-identical."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import cascade_ref as CR
import roitail_ref as RT
from conftest import PKG
from oracle import ref_model as R

pytestmark = pytest.mark.gpu

F32 = np.float32
SENT = -7
REC_FILL = 0xA5
NANB = np.float32("nan").view(np.uint32)


@pytest.fixture(scope="module")
def oh():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import orehip
    orehip.lib()
    return orehip


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _p(t):
    return None if t is None else t.data_ptr()


# ---- refine + cascade tail over the case table ---------------------------------------------------------------------------------------
def _run_cascade(oh, c):
    """The K launches of a case through the C ABI into sentinel-filled outputs; everything the launches wrote, on the host."""
    L = oh.lib()
    cap, K = c.cap, c.K
    n_dev = torch.tensor([c.n], dtype=torch.int32, device="cuda") if c.n_on_device else None
    nan = float("nan")
    boxes = [_dev(c.boxes)] + [torch.full((cap, 4), nan, device="cuda") for _ in range(K - 1)]
    ssum = torch.full((cap,), nan, device="cuda")
    dead = torch.full((cap,), 0x5A, dtype=torch.uint8, device="cuda")
    keep = []
    for k in range(K - 1):
        w = [_dev(a) for a in c.heads[k]]
        h, bias = _dev(c.hs[k]), None if c.bias[k] is None else _dev(c.bias[k])
        keep += [w, h, bias]
        rw = (C.c_float * 4)(*c.reg_ws[k])
        rc = L.ore_roi_cascade_refine_fwd(_p(h), c.C, c.parts, _p(bias), _p(w[0]), _p(w[1]), _p(w[2]), _p(w[3]), _p(boxes[k]), _p(n_dev), c.n, cap,
                                          rw, c.img[0], c.img[1], _p(boxes[k + 1]), _p(ssum), _p(dead), 1 if k > 0 else 0, oh._stream())
        assert rc == 0, L.ore_last_error()
    o = {"det_boxes": torch.full((cap, 4), nan, device="cuda"), "det_scores": torch.full((cap,), nan, device="cuda"),
         "det_src": torch.full((cap,), SENT, dtype=torch.int64, device="cuda"), "det_count": torch.full((4,), SENT, dtype=torch.int32, device="cuda"),
         "fin_boxes": torch.full((cap, 4), nan, device="cuda"), "fin_scores": torch.full((cap,), nan, device="cuda"),
         "fin_count": torch.full((4,), SENT, dtype=torch.int32, device="cuda")}
    post = _dev(c.post) if c.post is not None else None
    pin = rec = None
    if c.record != "none":
        pin = torch.full((4,), SENT, dtype=torch.int32, device="cuda")
        rec = torch.full((cap * 28,), REC_FILL, dtype=torch.uint8, device="cuda")
        pin[2:4] = torch.from_numpy(np.array([rec.data_ptr()], np.uint64).view(np.int32).copy()).cuda()
    wsb = L.ore_roi_predict_workspace_bytes(cap)
    ws = torch.full((wsb,), 0xFF, dtype=torch.uint8, device="cuda")
    w = [_dev(a) for a in c.heads[K - 1]]
    h, bias = _dev(c.hs[K - 1]), None if c.bias[K - 1] is None else _dev(c.bias[K - 1])
    rw = (C.c_float * 4)(*c.reg_ws[K - 1])
    has_fin = post is not None
    torch.cuda.synchronize()
    rc = L.ore_roi_predict_cascade_fwd(_p(h), c.C, _p(w[0]), _p(w[1]), _p(w[2]), _p(w[3]), _p(boxes[K - 1]), _p(n_dev), c.n, cap, rw, c.img[0],
                                       c.img[1], c.score_thresh, c.nms_thresh, c.topk, _p(o["det_boxes"]), _p(o["det_scores"]), _p(o["det_src"]),
                                       _p(o["det_count"]), _p(post), _p(o["fin_boxes"]) if has_fin else None,
                                       _p(o["fin_scores"]) if has_fin else None, _p(o["fin_count"]) if has_fin else None, _p(pin), _p(ws), wsb,
                                       oh._stream(), c.parts, _p(bias), _p(ssum), _p(dead), K)
    assert rc == 0, L.ore_last_error()
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in o.items()}
    out.update(stage_boxes=[b.cpu().numpy() for b in boxes], score_sum=ssum.cpu().numpy(), dead=dead.cpu().numpy(),
               pin=None if pin is None else pin.cpu().numpy(), rec=None if rec is None else rec.cpu().numpy())
    return out


@pytest.mark.parametrize("name", CR.case_names())
def test_refine_and_cascade_tail_vs_reference(oh, name):
    c = CR.case(name)
    exp = CR.expected(c)
    o = _run_cascade(oh, c)
    o2 = _run_cascade(oh, c)
    for k in ("det_boxes", "det_scores", "det_src", "det_count", "fin_boxes", "fin_scores", "fin_count", "score_sum", "dead"):
        assert _same_bits(o[k], o2[k]), (name, k, "two runs differ")
    n = c.n
    for k in range(1, c.K):                                                    # the boxes handed from stage to stage
        assert _same_bits(o["stage_boxes"][k][:n], exp["stage_boxes"][k]), (name, k)
        assert np.all(_bits(o["stage_boxes"][k][n:]) == NANB), (name, k, "rows at and beyond the count were written")
    assert _same_bits(o["score_sum"][:n], exp["score_sum"]) and np.all(_bits(o["score_sum"][n:]) == NANB), name
    assert np.array_equal(o["dead"][:n], exp["dead"].astype(np.uint8)) and np.all(o["dead"][n:] == 0x5A), name
    k = len(exp["scores"])
    assert o["det_count"].tolist() == [k, SENT, SENT, SENT], (name, o["det_count"], k)
    assert _same_bits(o["det_boxes"][:k], exp["boxes"]) and _same_bits(o["det_scores"][:k], exp["scores"]), name
    assert np.array_equal(o["det_src"][:k], exp["src"]), name
    assert np.all(_bits(o["det_boxes"][k:]) == NANB) and np.all(_bits(o["det_scores"][k:]) == NANB) and np.all(o["det_src"][k:] == SENT), name
    if c.post is None:
        assert np.all(_bits(o["fin_boxes"]) == NANB) and np.all(o["fin_count"] == SENT)
    else:
        f = len(exp["fin_scores"])
        assert o["fin_count"].tolist() == [f, SENT, SENT, SENT], (name, o["fin_count"], f)
        assert _same_bits(o["fin_boxes"][:f], exp["fin_boxes"]) and _same_bits(o["fin_scores"][:f], exp["fin_scores"]), name
        assert np.all(_bits(o["fin_boxes"][f:]) == NANB) and np.all(_bits(o["fin_scores"][f:]) == NANB), name
        if c.record == "rec":
            assert o["pin"][0] == f and o["pin"][1] == SENT, (name, o["pin"])
            assert np.array_equal(o["rec"], exp["record"]), name
    if "nonfinite" in c.prop:
        assert o["dead"][c.prop["nonfinite"][0]] == 1 and int(o["dead"][:n].sum()) == 1


@pytest.mark.parametrize("name", ["FUSED8-post-up-rec", "FUSED64-post-nonuniform-zero", "FUSED8-thr0.6", "f64-cap65-C208", "GENERAL-thr0.6"])
def test_one_stage_is_predict_parts(oh, name):
    """n_stages = 1 (score_sum = dead = NULL): the bytes of ore_roi_predict_parts_fwd on the same inputs, every launch form."""
    c = RT.case(name)
    res = []
    for casc in (False, True):
        pin = rec = None
        if c.record != "none":
            pin = torch.zeros(4, dtype=torch.int32, device="cuda")
            if c.record == "rec":
                rec = torch.full((c.cap * 28,), REC_FILL, dtype=torch.uint8, device="cuda")
                pin[2:4] = torch.from_numpy(np.array([rec.data_ptr()], np.uint64).view(np.int32).copy()).cuda()
        args = (_dev(c.h), _dev(c.cls_w), _dev(c.cls_b), _dev(c.box_w), _dev(c.box_b), _dev(c.boxes[:min(c.n, c.cap)]), RT.REG_W, c.img,
                c.score_thresh, c.nms_thresh, c.topk)
        kw = dict(parts=c.parts, bias=None if c.bias is None else _dev(c.bias), post=None if c.post is None else _dev(c.post), pin=pin)
        if casc:
            L = oh.lib()
            real = L.ore_roi_predict_parts_fwd
            try:                                         # the binding's one-stage call, sent through the cascade entry point
                L.ore_roi_predict_parts_fwd = lambda *a: L.ore_roi_predict_cascade_fwd(*a, None, None, 1)
                o = oh.roi_predict(*args, **kw)
            finally:
                L.ore_roi_predict_parts_fwd = real
        else:
            o = oh.roi_predict(*args, **kw)
        torch.cuda.synchronize()
        res.append({k: v.cpu().numpy() for k, v in o.items() if k != "_ws"} | {"rec": None if rec is None else rec.cpu().numpy()})
    a, b = res
    assert set(a) == set(b) and int(a["count"][0]) == len(RT.expected(c)["scores"])
    for k in a:
        assert (a[k] is None and b[k] is None) or _same_bits(a[k], b[k]), (name, k)


def test_cascade_launchers_refuse_outside_the_fused_domain(oh):
    L = oh.lib()
    z = torch.zeros(8, device="cuda")
    d = torch.zeros(8, dtype=torch.uint8, device="cuda")
    rw = (C.c_float * 4)(10, 10, 5, 5)
    for cap, Cc in ((513, 16), (64, 211), (0, 16)):
        rc = L.ore_roi_cascade_refine_fwd(_p(z), Cc, 0, None, _p(z), _p(z), _p(z), _p(z), _p(z), None, 0, cap, rw, 64.0, 64.0, _p(z), _p(z), _p(d), 0,
                                          oh._stream())
        assert rc != 0 and str(cap).encode() in L.ore_last_error()
    ws = torch.zeros(L.ore_roi_predict_workspace_bytes(600), dtype=torch.uint8, device="cuda")
    i64 = torch.zeros(8, dtype=torch.int64, device="cuda")
    i32 = torch.zeros(8, dtype=torch.int32, device="cuda")
    rc = L.ore_roi_predict_cascade_fwd(_p(z), 16, _p(z), _p(z), _p(z), _p(z), _p(z), None, 0, 600, rw, 64.0, 64.0, 0.0, 0.5, 10, _p(z), _p(z), _p(i64),
                                       _p(i32), None, None, None, None, None, _p(ws), ws.numel(), oh._stream(), 0, None, _p(z), _p(d), 3)
    assert rc != 0 and b"3 stages" in L.ore_last_error()
    rc = L.ore_roi_predict_cascade_fwd(_p(z), 16, _p(z), _p(z), _p(z), _p(z), _p(z), None, 0, 64, rw, 64.0, 64.0, 0.0, 0.5, 10, _p(z), _p(z), _p(i64),
                                       _p(i32), None, None, None, None, None, _p(ws), ws.numel(), oh._stream(), 0, None, None, None, 2)
    assert rc != 0 and b"2 stages" in L.ore_last_error()
    torch.cuda.synchronize()
    assert int(i32.abs().sum()) == 0


# ---- the training seam ----------------------------------------------------------------------------------------------------------------
_RELABEL = {c.name: c for c in CR.relabel_cases()}


@pytest.mark.parametrize("name", list(_RELABEL))
def test_relabel_vs_restatement(oh, name):
    c = _RELABEL[name]
    want = CR.relabel(c.boxes, c.deltas, c.valid, c.img_hw, c.gtp, c.gt_n, c.reg_w, c.thr)
    got = oh.cascade_relabel(_dev(c.boxes), _dev(c.deltas), _dev(c.valid), _dev(c.img_hw), _dev(c.gtp), _dev(c.gt_n), c.reg_w, c.thr)
    again = oh.cascade_relabel(_dev(c.boxes), _dev(c.deltas), _dev(c.valid), _dev(c.img_hw), _dev(c.gtp), _dev(c.gt_n), c.reg_w, c.thr)
    torch.cuda.synchronize()
    for i, what in enumerate(("boxes", "labels", "gt", "valid")):
        g = got[i].cpu().numpy()
        assert np.array_equal(g, want[i]), (name, what)
        assert np.array_equal(g, again[i].cpu().numpy()), (name, what, "two launches differ")
    if "valid" in c.prop:
        assert got[3].cpu().numpy().tolist() == [list(c.prop["valid"])]


def test_relabel_refuses_more_than_256_ground_truth_boxes(oh):
    z = torch.zeros(1, 4, 4, device="cuda")
    with pytest.raises(oh.OreError, match="G=257"):
        oh.cascade_relabel(z, z, torch.ones(1, 4, dtype=torch.bool, device="cuda"), torch.ones(1, 2, device="cuda"),
                           torch.zeros(1, 257, 4, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"), CR.REG_W[0], 0.7)


# ---- module path and engine -----------------------------------------------------------------------------------------------------------
def _sd3(scale=None):
    sd = CR.synth_cascade_state(R.synth_roi_state(R.synth_state_dict(0), 0), 0, 3)
    if scale is not None:
        for k in range(3):
            sd[f"roi_heads.box_head.{k}.fc1.weight"] = sd[f"roi_heads.box_head.{k}.fc1.weight"] * scale
    return sd


def _model(yaml, extra=()):
    from fewx.config import get_cfg
    from detectron2.modeling import build_model
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(PKG, "configs", "fsod", yaml))
    cfg.merge_from_list(["MODEL.DEVICE", "cuda", "INPUT.MAX_SIZE_TEST", 640] + list(extra))
    cfg.freeze()
    torch.manual_seed(0)
    return build_model(cfg), cfg


@pytest.fixture(scope="module")
def model3(oh):
    m, _ = _model("finetune_vovnet_cascade.yaml")
    missing, unexpected = m.load_state_dict(_sd3(), strict=False)
    assert not unexpected and not missing, (missing, unexpected)
    return m.eval()


def test_module_path_vs_reference_run(model3, golden):
    """The executed reference's three stages (tests/golden/cascade_stage_eval.npz) through the registered module: the same kept rows,
    scores and boxes within the bounds of test_hip_parity.py::test_roi_heads_module_vs_reference_run."""
    from detectron2.structures import Boxes, ImageList, Instances
    g = golden("cascade_stage_eval")
    hw = tuple(int(v) for v in g["image_hw"])
    prop = Instances(hw)
    prop.proposal_boxes = Boxes(torch.from_numpy(g["proposals"]).cuda())
    prop.objectness_logits = torch.from_numpy(g["proposal_scores"]).cuda()
    feats = {k: torch.from_numpy(golden("roi_stage_eval")[k]).cuda() for k in ("p3", "p4", "p5")}
    sup = [torch.from_numpy(golden("roi_stage_eval")[k]).cuda() for k in ("sup8", "sup4")]
    res, _ = model3.roi_heads(ImageList(torch.empty(0), [hw]), feats, sup, [prop], None)
    r = res[0]
    assert len(r) == len(g["scores"]) and r.image_size == hw
    np.testing.assert_allclose(r.scores.cpu().numpy(), g["scores"], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(r.pred_boxes.tensor.cpu().numpy(), g["pred_boxes"], rtol=1e-4, atol=2e-2)
    assert r.pred_classes.dtype == torch.int64 and int(r.pred_classes.abs().sum()) == 0
    res2, _ = model3.roi_heads(ImageList(torch.empty(0), [hw]), feats, sup, [prop], None)
    assert torch.equal(res2[0].scores, r.scores) and torch.equal(res2[0].pred_boxes.tensor, r.pred_boxes.tensor)


HW = (256, 320)


def _supports(n):
    return [(R.synth_support(10 + k), torch.randn(6, 128, 8, 8, generator=torch.Generator().manual_seed(40 + k)) * 0.1) for k in range(n)]


def _engine(oh, sd, roi_sd, sup, stages, max_batch=1, ids=None, sups=None):
    e = oh.Engine(max_batch=max_batch, max_h=HW[0], max_w=HW[1])
    e.load_state_dict(sd)
    if ids is None:
        e.set_support(sup[0])
    e.finalize()
    if stages == "head":
        e.set_roi_head(roi_sd, sup[1], CR.REG_W[0], 0.05, 0.5, 100)
    else:
        e.set_roi_cascade(roi_sd, sup[1], CR.REG_W[:stages], 0.05, 0.5, 100)
    if ids is not None:
        e.set_classes(ids)
        for k, (p, rc8) in enumerate(sups):
            e.set_support(p, slot=k)
            e.set_roi_support(roi_sd, rc8, slot=k)
    return e


def _module_on_engine(oh, m, e, rc8, b, B):
    """The module path (K stages, per-op launches) on image b's proposals and pyramid of the engine's last pass."""
    from detectron2.structures import Boxes, ImageList, Instances
    pb, ps, _ = e.proposals(b)
    prop = Instances(HW)
    prop.proposal_boxes = Boxes(pb.clone())
    prop.objectness_logits = ps.clone()
    # (a bf16-storage engine keeps bf16 maps: their fp32 values are what its ROIAlign reads)
    feats = {f"p{l}": e.buffer(f"p{l}", (B, HW[0] >> l, HW[1] >> l))[b:b + 1].float() for l in (3, 4, 5)}
    res, _ = m.roi_heads(ImageList(torch.empty(0), [HW]), feats, [rc8.cuda(), None], [prop], None)
    return res[0]


def _assert_engine_is_module(e, r, b):
    eb, es, _ = e.detections(b)
    assert len(es) == len(r.scores) and len(es) > 0, (len(es), len(r.scores))
    np.testing.assert_allclose(r.scores.cpu().numpy(), es.cpu().numpy(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(r.pred_boxes.tensor.cpu().numpy(), eb.cpu().numpy(), rtol=1e-4, atol=1e-2)


@pytest.fixture(scope="module")
def casc_model(oh):
    """A detector built from the cascade yaml with un-saturated second-stage weights, score 0.05 / NMS 0.5 / top-100 as the engines."""
    m, _ = _model("finetune_vovnet_cascade.yaml", ["MODEL.ROI_HEADS.SCORE_THRESH_TEST", 0.05, "MODEL.ROI_HEADS.NMS_THRESH_TEST", 0.5])
    sd = _sd3(0.01)
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and not missing
    return m.eval(), sd


@pytest.mark.parametrize("mode", ["fp32", "bf16", "bf16s"])
def test_engine_cascade_one_image_and_folded_batch(oh, casc_model, mode):
    m, sd = casc_model
    sup = _supports(1)[0]
    prev = oh.set_conv_precision(mode)
    try:
        e = _engine(oh, sd, sd, sup, 3, max_batch=1 if mode == "bf16s" else 3)      # (the bf16 storage mode takes one image per pass)
    finally:
        oh.set_conv_precision(prev)
    try:
        assert e.roi_stages == 3
        img = R.synth_image(7, *HW).cuda()
        e.eval_forward(img, use_graph=False)
        torch.cuda.synchronize()
        _assert_engine_is_module(e, _module_on_engine(oh, m, e, sup[1], 0, 1), 0)
        one = [t.clone() for t in e.detections(0)]
        e.eval_forward(img, use_graph=True)                                  # the captured pass: the same bits
        e.eval_forward(img, use_graph=True)
        torch.cuda.synchronize()
        for a, b in zip(one, e.detections(0)):
            assert torch.equal(a, b)
        if mode == "bf16s":
            return
        imgs = torch.stack([img, R.synth_image(8, *HW).cuda(), R.synth_image(9, *HW).cuda()])
        e.eval_forward_batch(imgs, use_graph=False)
        torch.cuda.synchronize()
        for b in range(3):
            _assert_engine_is_module(e, _module_on_engine(oh, m, e, sup[1], b, 3), b)
    finally:
        e.close()


def test_engine_cascade_nway_two_classes(oh, casc_model):
    """Class slot k of the N-way pass runs the three stages with ITS composed fc1 per stage: per class the detections of a single-class
    cascade engine with that class's support (the bound test_hip_nway.py uses between the two: equal rows, scores and boxes)."""
    m, sd = casc_model
    sups = _supports(2)
    img = R.synth_image(7, *HW).cuda()
    en = _engine(oh, sd, sd, sups[0], 3, max_batch=2, ids=[11, 12], sups=sups)
    try:
        en.eval_classes_forward(img, use_graph=False)
        torch.cuda.synchronize()
        for k, s in enumerate(sups):
            e1 = _engine(oh, sd, sd, s, 3)
            try:
                e1.eval_forward(img, use_graph=False)
                torch.cuda.synchronize()
                b1, s1, _ = e1.detections(0)
                bk, sk, _ = en.detections(k)
                assert len(s1) == len(sk) and len(sk) > 0
                np.testing.assert_allclose(sk.cpu().numpy(), s1.cpu().numpy(), rtol=1e-4, atol=1e-6)
                np.testing.assert_allclose(bk.cpu().numpy(), b1.cpu().numpy(), rtol=1e-4, atol=1e-2)
            finally:
                e1.close()
    finally:
        en.close()


def test_engine_nway_pass_refuses_a_slot_without_every_stage(oh, casc_model):
    m, sd = casc_model
    sups = _supports(2)
    e = oh.Engine(max_batch=2, max_h=HW[0], max_w=HW[1])
    try:
        e.load_state_dict(sd)
        e.finalize()
        e.set_roi_cascade(sd, sups[0][1], CR.REG_W, 0.05, 0.5, 100)
        e.set_classes([11, 12])
        for k, (p, rc8) in enumerate(sups):
            e.set_support(p, slot=k)
        e.set_roi_support(sd, sups[0][1], slot=0)
        e.roi_stages = 1                                                     # the binding of before: stage 0 only
        e.set_roi_support(sd, sups[1][1], slot=1)
        with pytest.raises(oh.OreError, match="3 cascade stages"):
            e.eval_classes_forward(R.synth_image(7, *HW).cuda(), use_graph=False)
        with pytest.raises(oh.OreError, match="cascade stages"):
            e.set_roi_cascade(sd, sups[0][1], CR.REG_W + CR.REG_W, 0.05, 0.5, 100)
    finally:
        e.close()


def test_engine_one_stage_through_the_new_setter_is_set_roi_head(oh, casc_model):
    m, sd = casc_model
    sup = _supports(1)[0]
    img = R.synth_image(7, *HW).cuda()
    out = []
    for stages in ("head", 1):
        e = _engine(oh, sd, sd, sup, stages)
        try:
            e.set_profiling(True)
            e.eval_forward(img, use_graph=False)
            torch.cuda.synchronize()
            _, flops, launches = e.read_profile()
            e.set_profiling(False)
            e.eval_forward(img, use_graph=True)
            torch.cuda.synchronize()
            out.append((launches, flops, [t.clone() for t in e.detections(0)], e.buffer("final_boxes").clone()))
        finally:
            e.close()
    assert out[0][0] == out[1][0] and out[0][1] == out[1][1], (out[0][:2], out[1][:2])
    for a, b in zip(out[0][2], out[1][2]):
        assert torch.equal(a, b) and len(a) > 0
    assert torch.equal(out[0][3], out[1][3])
    # and the three-stage engine launches two more rounds of the second-stage GEMM
    e = _engine(oh, sd, sd, sup, 3)
    try:
        e.set_profiling(True)
        e.eval_forward(img, use_graph=False)
        torch.cuda.synchronize()
        _, _, launches3 = e.read_profile()
    finally:
        e.close()
    assert launches3 == out[0][0] + 2, (launches3, out[0][0])


# ---- training -------------------------------------------------------------------------------------------------------------------------
def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _eager_stage_run(rh, g, ge):
    from detectron2.layers import nhwc_view
    from fewx.modeling.fsod.train_forward import roi_stage_losses
    for p in rh.parameters():
        p.grad = None
    feats = [torch.from_numpy(ge[k]).cuda().requires_grad_(True) for k in ("p3", "p4", "p5")]
    qf = [nhwc_view(f)[0] for f in feats]
    s8 = torch.from_numpy(ge["sup8"]).cuda()
    sup8 = s8.permute(0, 2, 3, 1).reshape(s8.shape[0], -1)
    losses, aux = roi_stage_losses(rh, qf, sup8, torch.from_numpy(g["roi_boxes0"]).cuda(), torch.from_numpy(g["roi_labels0"]).cuda(),
                                   torch.from_numpy(g["roi_gt0"]).cuda(), [8, 16, 32], gt_boxes=torch.from_numpy(g["gt"]).cuda(),
                                   image_hw=tuple(int(v) for v in g["image_hw"]))
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    return losses, aux, feats


def test_eager_training_iteration_vs_reference_run(model3, golden):
    """roi_stage_losses (one image, rows dropped between the stages as the reference drops them) on the executed reference's sampled
    rows: per-stage rows and labels, all 2K losses, the sampled gradients -- the bounds of test_oracle_golden.py::
    test_roi_stage_train_matches_reference_run per quantity (labels equal, logits / deltas 1e-5, losses 2e-6, gradients 2e-5)."""
    g, ge = golden("cascade_stage_train"), golden("roi_stage_eval")
    rh = model3.roi_heads
    rh.train()
    try:
        losses, aux, feats = _eager_stage_run(rh, g, ge)
        named = dict(rh.named_parameters())
        fig = {}
        for k in range(3):
            bx, lb, gt = aux["stages"][k]
            assert len(bx) == len(g[f"roi_boxes{k}"]), (k, len(bx))
            assert np.array_equal(lb.cpu().numpy(), g[f"roi_labels{k}"]), k
            fg = g[f"roi_labels{k}"] == 0
            assert np.array_equal(gt.cpu().numpy()[fg], g[f"roi_gt{k}"][fg]), k
            np.testing.assert_allclose(bx.cpu().numpy(), g[f"roi_boxes{k}"], rtol=1e-5, atol=2e-3)
            for n_ in ("loss_cls_stage", "loss_box_reg_stage"):
                fig[f"{n_}{k}"] = abs(float(losses[f"{n_}{k}"].detach()) - float(g[f"{n_}{k}"])) / float(g[f"{n_}{k}"])
            for key, name in ((f"g_cls_w{k}", f"box_predictor.{k}.cls_score.weight"), (f"g_box_w{k}", f"box_predictor.{k}.bbox_pred.weight"),
                              (f"g_fc1_b{k}", f"box_head.{k}.fc1.bias")):
                fig[key] = _rel(named[name].grad.cpu().numpy(), g[key])
        fig["logits2"] = _rel(aux["scores"].detach().cpu().numpy(), g["cls_logits2"])
        fig["deltas2"] = _rel(aux["deltas"].detach().cpu().numpy(), g["deltas2"])
        fig["g_conv3_w"] = _rel(named["conv3.weight"].grad.cpu().numpy(), g["g_conv3_w"])
        fig["g_conv1_b"] = _rel(named["conv1.bias"].grad.cpu().numpy(), g["g_conv1_b"])
        for l, k in enumerate(("p3", "p4", "p5")):
            fig[f"g_{k}_sum"] = _rel(feats[l].grad.sum((0, 2, 3)).cpu().numpy(), g[f"g_{k}_sum"])
        print("cascade train figures:", {k: f"{v:.2e}" for k, v in fig.items()})
        for k, v in fig.items():
            bound = 2e-6 if k.startswith("loss") else 1e-5 if k in ("logits2", "deltas2") else 2e-5
            assert v < bound, (k, v, bound)
        assert sorted(g["dead"]) == sorted(k for k, v in named.items() if v.grad is None)
        # two runs: the same bits
        snap = {k: v.grad.clone() for k, v in named.items() if v.grad is not None}
        losses2, _, feats2 = _eager_stage_run(rh, g, ge)
        assert all(torch.equal(losses[k], losses2[k]) for k in losses)
        assert all(torch.equal(snap[k], named[k].grad) for k in snap) and all(torch.equal(a.grad, b.grad) for a, b in zip(feats, feats2))
    finally:
        rh.eval()


def test_padded_form_equals_the_eager_form(model3, golden):
    """roi_stage_losses_padded (fixed shapes: a dropped row turns into a padding row) on the same rows, in a batch of two with padding:
    the eager form's losses and gradients."""
    from detectron2.layers import nhwc_view
    from fewx.modeling.fsod.train_forward import roi_stage_losses_padded
    g, ge = golden("cascade_stage_train"), golden("roi_stage_eval")
    rh = model3.roi_heads
    rh.train()
    try:
        losses, aux, feats = _eager_stage_run(rh, g, ge)
        named = dict(rh.named_parameters())
        want = {k: v.grad.clone() for k, v in named.items() if v.grad is not None}
        for p in rh.parameters():
            p.grad = None
        B, Rn, Rp = 2, len(g["roi_boxes0"]), 160
        f2 = [torch.from_numpy(ge[k]).cuda().repeat(B, 1, 1, 1).requires_grad_(True) for k in ("p3", "p4", "p5")]
        s8 = torch.from_numpy(ge["sup8"]).cuda()
        sup8 = s8.permute(0, 2, 3, 1).reshape(1, s8.shape[0], -1).repeat(B, 1, 1)
        boxes = torch.tensor([0.0, 0.0, 8.0, 8.0], device="cuda").repeat(B, Rp, 1)
        labels = torch.ones(B, Rp, dtype=torch.int64, device="cuda")
        gt = torch.zeros(B, Rp, 4, device="cuda")
        valid = torch.zeros(B, Rp, dtype=torch.bool, device="cuda")
        boxes[:, :Rn], labels[:, :Rn], gt[:, :Rn], valid[:, :Rn] = torch.from_numpy(g["roi_boxes0"]).cuda(), torch.from_numpy(g["roi_labels0"]).cuda(), \
            torch.from_numpy(g["roi_gt0"]).cuda(), True
        gtp = torch.from_numpy(g["gt"]).cuda()[None].repeat(B, 1, 1).contiguous()
        gt_n = torch.full((B,), len(g["gt"]), dtype=torch.int64, device="cuda")
        hw = torch.tensor([[float(v) for v in g["image_hw"]]] * B, device="cuda")
        lp, ap = roi_stage_losses_padded(rh, [nhwc_view(f) for f in f2], sup8, boxes, labels, gt, valid, [8, 16, 32], gtp=gtp, gt_n=gt_n, img_hw=hw)
        sum(lp.values()).backward()
        torch.cuda.synchronize()
        assert set(lp) == set(losses) == {f"{n_}{k}" for n_ in ("loss_cls_stage", "loss_box_reg_stage") for k in range(3)}
        for k in range(3):
            v = ap["stages"][k][3]
            assert int(v[0].sum()) == int(v[1].sum()) == len(g[f"roi_boxes{k}"])
            # the same rows: equal labels and matched boxes; the boxes of the stages k >= 1 are decoded from deltas that a GEMM of
            # another row count (B x 160 padded rows, not 128) summed in another order, so they agree to the bound the per-stage boxes
            # are held to against the fixture (1e-5 relative, 2e-3 px), stage 0 bit for bit
            np.testing.assert_allclose(ap["stages"][k][0][0][v[0]].cpu().numpy(), aux["stages"][k][0].cpu().numpy(), rtol=1e-5 if k else 0,
                                       atol=2e-3 if k else 0)
            assert torch.equal(ap["stages"][k][1][0][v[0]], aux["stages"][k][1])
            assert torch.equal(ap["stages"][k][2][0][v[0]], aux["stages"][k][2])
            assert torch.equal(ap["stages"][k][0][0], ap["stages"][k][0][1])                 # two identical images: identical rows
        for k in losses:                                                                     # (two identical images: the mean is each one's loss)
            assert abs(float(lp[k]) - float(losses[k])) <= 1e-5 * abs(float(losses[k])), (k, float(lp[k]), float(losses[k]))
        for k, w in want.items():
            assert _rel(named[k].grad.cpu().numpy(), w.cpu().numpy()) < 1e-4, k
    finally:
        rh.eval()


def _train_model3(shots):
    from test_hip_train import _train_model  # noqa: F401  (the one-stage recipe this follows)
    m, cfg = _model("finetune_vovnet_cascade.yaml", ["INPUT.FS.SUPPORT_SHOT", shots])
    sd = _sd3(0.02)
    sd["proposal_generator.centernet_head.agn_hm.bias"] = torch.full((1,), -2.0)
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and not missing, (missing, unexpected)
    m.train()
    for lvl in (3, 4, 5):
        getattr(m, f"vip_p{lvl}").reweighting.drop.p = 0.0
    return m, cfg


def _run_steps(batches, make_stepper):
    from fewx.solver import build_optimizer
    m, cfg = _train_model3(4)
    opt = build_optimizer(cfg, m)
    stepper = make_stepper(m, opt) if make_stepper is not None else None
    log = []
    for it, items in enumerate(batches):
        opt.set_lr_factor(0.02 * (1.0 + 0.25 * it))
        if stepper is not None:
            losses = stepper(items)
        else:
            losses = m(items)
            opt.zero_grad()
            sum(losses.values()).backward()
            opt.step()
        log.append({k: float(v.detach()) for k, v in losses.items()})
    torch.cuda.synchronize()
    return log, opt.bucket.params.detach().clone(), opt.bucket.momentum.detach().clone(), stepper


@pytest.mark.parametrize("mixed", [False, True])
def test_graphed_step_replays_the_cascade(oh, monkeypatch, mixed):
    """GraphedTrainStep at K = 3: two eager + three replayed steps leave the parameters of five eager steps (the bar of
    test_hip_train.py::test_whole_step_graph_matches_eager); mixed: a batch of two sizes staged through the canvas, the sizes the
    relabel kernel clips to read from the canvas table on the device.  And the eager run twice: the same bits."""
    from fewx.solver import GraphedTrainStep
    from test_hip_multiscale_step import _assert_same_training, _fix_sampling_keys, _item
    a, b = _item(2, (256, 320), 5), _item(3, (224, 320) if mixed else (256, 320), 6)
    _fix_sampling_keys(monkeypatch, 2)
    batches = [[a, b] if it % 2 == 0 else [b, a] for it in range(5)]
    eager = _run_steps(batches, None)
    assert {f"loss_cls_stage{k}" for k in range(3)} | {f"loss_box_reg_stage{k}" for k in range(3)} <= set(eager[0][0])
    assert all(np.isfinite(v) for row in eager[0] for v in row.values())
    graph = _run_steps(batches, lambda m, opt: GraphedTrainStep(m, opt, warmup=2, mixed_sizes=mixed))
    st = graph[3]
    assert st.error is None, st.error
    assert st.eager_steps == 2 and st.replays == 3, st.stats()
    _assert_same_training(eager, graph)
    again = _run_steps(batches, None)
    assert eager[0] == again[0] and torch.equal(eager[1], again[1]) and torch.equal(eager[2], again[2])
