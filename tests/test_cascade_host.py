"""CPU: the cascade of CustomCascadeROIHeads without a GPU.

  * the composed reference (tests/cascade_ref.py: the C twin per stage + the numpy mean + oracle.decode.nms; the relabel restatement)
    reproduces the EXECUTED reference (tests/golden/cascade_stage_{eval,train}.npz, tools/gen_cascade_golden.py): the same kept rows
    in the same order, per-stage boxes, final boxes and scores within the bounds test_oracle_golden.py::test_roi_stage_eval uses for
    the same quantities, array-equal labels and matched ground truth in every training stage -- a condition on the fixture's seed;
  * the config checks of the module: both ValueErrors, the new yaml, a 3-stage state dict with strict=True, compose_roi_head(stage=k);
  * every seeded fault of cascade_ref changes at least one case of its table: the table sees it."""
import os

import numpy as np
import pytest
import torch

import cascade_ref as CR
from conftest import PKG, rel_err
from oracle import ref_model as R

F32 = np.float32


def _sd3():
    return CR.synth_cascade_state(R.synth_roi_state(R.synth_state_dict(0), 0), 0, 3)


def _heads(sd, K):
    p = "roi_heads.box_predictor."
    return [tuple(sd[p + f"{k}.{n}"].numpy() for n in ("cls_score.weight", "cls_score.bias", "bbox_pred.weight", "bbox_pred.bias")) for k in range(K)]


# ---- reference against fixture ------------------------------------------------------------------------------------------------------
def test_composed_reference_reproduces_the_executed_eval_fixture(golden):
    g = golden("cascade_stage_eval")
    K = int(g["stages"])
    assert K == 3 and tuple(g["ious"]) == CR.IOUS and np.array_equal(g["reg_weights"], np.array(CR.REG_W))
    sd = _sd3()
    hw = tuple(int(v) for v in g["image_hw"])
    out = CR.cascade_eval([g[f"h{k}"] for k in range(K)], _heads(sd, K), g["proposals"], CR.REG_W, hw, 0.0, 0.9, 100)
    assert np.array_equal(g["boxes0"], g["proposals"])
    for k in range(1, K):                                 # the boxes every stage pooled (the pooler's input in the executed reference)
        np.testing.assert_allclose(out["stage_boxes"][k], g[f"boxes{k}"], rtol=1e-5, atol=2e-3)
    assert not out["dead"].any()
    # the same kept source rows in the same order: the fixture's detections are rows of its own last-stage decode, found by their boxes
    assert len(out["scores"]) == len(g["scores"]) and len(g["scores"]) > 20
    np.testing.assert_allclose(out["scores"], g["scores"], rtol=2e-6, atol=1e-7)
    np.testing.assert_allclose(out["boxes"], g["pred_boxes"], rtol=1e-5, atol=2e-3)
    # (by box AND score: boxes clipped to the whole image coincide)
    d = np.abs(out["raw_boxes"][None, :, :] - g["pred_boxes"][:, None, :]).max(2)
    ds = np.abs(out["raw_scores"][None, :] - g["scores"][:, None])
    match = (d <= 2e-3 + 1e-5 * np.abs(g["pred_boxes"]).max(1)[:, None]) & (ds <= 1e-7 + 2e-6 * g["scores"][:, None])
    assert (match.sum(1) == 1).all()
    src_fix = match.argmax(1)
    assert len(set(src_fix.tolist())) == len(src_fix)
    assert np.array_equal(src_fix, out["src"])
    assert (g["pred_classes"] == 0).all() and np.all(np.diff(g["scores"]) <= 0)
    # the fixture's scores ARE the fp32 mean of its own three softmaxes (MULT_PROPOSAL_SCORE not applied)
    lg = [torch.softmax(torch.from_numpy(g[f"cls_logits{k}"]), 1)[:, 0].numpy() for k in range(K)]
    mean = ((lg[0] + lg[1]) + lg[2]) * F32(1.0 / 3)
    np.testing.assert_allclose(mean[out["src"]], g["scores"], rtol=2e-6, atol=1e-7)
    # and no decision of it sits on a near-tie: every candidate pair's IoU is away from the NMS threshold, every score from the filter
    cand = out["raw_boxes"][out["ok"]]
    iou = _pairwise(cand, cand)[~np.eye(len(cand), dtype=bool)]
    assert np.abs(iou - 0.9).min() > 1e-4 and (iou > 0.9).any()
    assert np.abs(out["raw_scores"]).min() > 1e-4                              # score > 0.0 is no near-tie either


def test_relabel_restatement_reproduces_the_executed_train_fixture(golden):
    g = golden("cascade_stage_train")
    K = int(g["stages"])
    hw = np.array([g["image_hw"]], F32)
    gt = g["gt"][None].astype(F32)
    gt_n = np.array([len(g["gt"])], np.int64)
    for k in range(1, K):
        prev_b, prev_d = g[f"roi_boxes{k - 1}"][None], g[f"deltas{k - 1}"][None]
        R_ = prev_b.shape[1]
        ob, ol, og, ov, oi = CR.relabel(prev_b, prev_d, np.ones((1, R_), bool), hw, gt, gt_n, CR.REG_W[k - 1], CR.IOUS[k])
        keep = ov[0]
        assert int(keep.sum()) == len(g[f"roi_boxes{k}"]), k                 # the reference dropped the same empty rows
        np.testing.assert_allclose(ob[0][keep], g[f"roi_boxes{k}"], rtol=1e-5, atol=2e-3)
        assert np.array_equal(ol[0][keep], g[f"roi_labels{k}"]), k
        assert np.array_equal(og[0][keep], g[f"roi_gt{k}"]), k
        fix_idx = np.abs(g[f"roi_gt{k}"][:, None, :] - g["gt"][None, :, :]).max(2).argmin(1)
        assert np.array_equal(oi[0][keep], fix_idx), k
        assert 0 < int((ol[0][keep] == 0).sum()) < int(keep.sum())
        # run on the fixture's own stage boxes the labels are equal as well (no IoU within rounding of the threshold)
        iou = _pairwise(g[f"roi_boxes{k}"], g["gt"]).max(1)
        assert np.abs(iou - CR.IOUS[k]).min() > 1e-4, k
    assert len(g["roi_boxes1"]) < len(g["roi_boxes0"])                       # the fixture does drop rows: the empty-row rule is exercised
    assert sorted(g["dead"]) == ["fc2.bias", "fc2.weight", "fc3.bias", "fc3.weight"]


def _pairwise(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    iw = np.clip(np.minimum(a[:, None, 2], b[None, :, 2]) - np.maximum(a[:, None, 0], b[None, :, 0]), 0, None)
    ih = np.clip(np.minimum(a[:, None, 3], b[None, :, 3]) - np.maximum(a[:, None, 1], b[None, :, 1]), 0, None)
    inter = iw * ih
    ua = np.maximum(((a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]))[:, None] + ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]))[None, :] - inter, 1e-300)
    return np.where(inter > 0, inter / ua, 0.0)


# ---- config checks ------------------------------------------------------------------------------------------------------------------
def _cfg(*overrides, yaml="finetune_vovnet_cascade.yaml"):
    from fewx.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(PKG, "configs", "fsod", yaml))
    cfg.merge_from_list(list(overrides))
    return cfg


def _heads_of(cfg):
    from detectron2.layers import ShapeSpec
    from fewx.modeling.fsod.fsod_roi_heads import build_roi_heads
    return build_roi_heads(cfg, {k: ShapeSpec(channels=128, stride=s) for k, s in (("p3", 8), ("p4", 16), ("p5", 32))})


def test_cascade_yaml_resolves_and_builds_three_stages():
    cfg = _cfg()
    assert list(cfg.MODEL.ROI_BOX_CASCADE_HEAD.IOUS) == [0.6, 0.7, 0.8]
    assert [list(w) for w in cfg.MODEL.ROI_BOX_CASCADE_HEAD.BBOX_REG_WEIGHTS] == [list(w) for w in CR.REG_W]
    assert cfg.MODEL.ROI_HEADS.NAME == "CustomCascadeROIHeads" and cfg.MODEL.VOVNET.CONV_BODY == _cfg(yaml="finetune_vovnet.yaml").MODEL.VOVNET.CONV_BODY
    rh = _heads_of(cfg)
    assert len(rh.box_head) == len(rh.box_predictor) == rh.num_cascade_stages == 3
    assert rh.iou_thresholds == CR.IOUS and rh.bbox_reg_weights_per_stage == CR.REG_W
    assert rh.iou_threshold == 0.6 and rh.bbox_reg_weights == CR.REG_W[0]           # stage 0, for the callers that know one stage
    one = _heads_of(_cfg(yaml="finetune_vovnet.yaml"))
    assert one.num_cascade_stages == 1 and one.bbox_reg_weights_per_stage == (one.bbox_reg_weights,)


def test_length_mismatch_raises_and_says_what_to_set():
    # the package defaults: three IOUS, ONE weights entry -- the config a user gets without overriding either
    with pytest.raises(ValueError, match="BBOX_REG_WEIGHTS") as ei:
        _heads_of(_cfg("MODEL.ROI_BOX_CASCADE_HEAD.IOUS", [0.6, 0.7, 0.8], yaml="finetune_vovnet.yaml"))
    assert "3 stages" in str(ei.value) and "one 4-tuple" in str(ei.value)


def test_iou_threshold_mismatch_raises_and_says_what_to_set():
    with pytest.raises(ValueError, match=r"IOU_THRESHOLDS") as ei:
        _heads_of(_cfg("MODEL.ROI_BOX_CASCADE_HEAD.IOUS", [0.5, 0.6, 0.7]))
    assert "set IOU_THRESHOLDS: [0.5]" in str(ei.value)


def test_three_stage_state_dict_loads_strict():
    rh = _heads_of(_cfg())
    sd = {k[len("roi_heads."):]: v for k, v in _sd3().items() if k.startswith("roi_heads.")}
    rh.load_state_dict(sd, strict=True)
    assert torch.equal(rh.box_head[2].fc1.weight, sd["box_head.2.fc1.weight"])


def test_compose_roi_head_per_stage_equals_the_uncomposed_chain(golden):
    import orehip
    g = golden("roi_stage_eval")
    sd = _sd3()
    sup = torch.from_numpy(g["sup8"])
    x = torch.randn(9, 128, 8, 8, generator=torch.Generator().manual_seed(3))
    xf = x.permute(0, 2, 3, 1).reshape(9, -1).double()                      # [pos][channel], the ROIAlign kernel's order
    seen = []
    for k in range(3):
        sdk = dict(sd)
        sdk["roi_heads.box_head.0.fc1.weight"], sdk["roi_heads.box_head.0.fc1.bias"] = sd[f"roi_heads.box_head.{k}.fc1.weight"], sd[f"roi_heads.box_head.{k}.fc1.bias"]
        want = R.roi_head_features(x, sup, sdk)
        Wp, bp = orehip.compose_roi_head(sd, sup, stage=k)
        got = torch.relu(xf @ Wp.double().t() + bp.double()).float()
        assert rel_err(got.numpy(), want.numpy()) < 1e-4, k
        seen.append(got)
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
    W0, b0 = orehip.compose_roi_head(sd, sup)
    W0s, b0s = orehip.compose_roi_head(sd, sup, stage=0)
    assert torch.equal(W0, W0s) and torch.equal(b0, b0s)


# ---- the case tables and the seeded faults -------------------------------------------------------------------------------------------
def test_eval_table_covers_the_axes():
    cs = CR.cases()
    assert {c.cap for c in cs} == set(CR.CAPS) and {c.C for c in cs} == set(CR.WIDTHS)
    assert {(c.cap, c.C) for c in cs} >= {(cap, C) for cap in CR.CAPS for C in CR.WIDTHS}
    assert {(c.parts, c.n, c.K) for c in cs if c.cap == 320} >= {(p, n, K) for p in CR.PARTS for n in (0, 1, 320) for K in CR.STAGES}
    assert {c.n_on_device for c in cs} == {False, True}
    assert any(c.post is not None and c.record == "rec" for c in cs)
    for c in cs:
        e = CR.expected(c)
        assert len(e["scores"]) <= max(c.n, 0) and np.all(np.diff(e["scores"]) <= 0)
    full = [c for c in cs if c.n == c.cap and c.cap >= 63 and "nonfinite" not in c.prop]
    assert all(len(CR.expected(c)["scores"]) > 0 for c in full)
    assert any(0 < len(CR.expected(c)["scores"]) < int(CR.expected(c)["ok"].sum()) for c in full)       # NMS / top-k do remove rows


def test_nonfinite_rows_are_dead_and_only_they():
    cs = [c for c in CR.cases() if "nonfinite" in c.prop]
    assert {c.parts for c in cs} == set(CR.PARTS)
    for c in cs:
        e = CR.expected(c)
        r0, r1 = c.prop["nonfinite"]
        assert e["dead"][r0] and int(e["dead"].sum()) == 1                    # the intermediate stage's row is dead from there on
        assert np.array_equal(e["stage_boxes"][1][r0], np.zeros(4, F32)) and e["score_sum"][r0] == 0
        assert r0 not in e["src"]
        if c.parts == 0:                                                      # (K-split partials: fmaxf turns the NaN sum into 0)
            assert not e["ok"][r1] and r1 not in e["src"]


@pytest.mark.parametrize("fault", CR.EVAL_FAULTS)
def test_every_eval_fault_changes_a_case(fault):
    changed = []
    for c in CR.cases():
        if c.n == 0:
            continue
        a, b = CR.expected(c), CR.expected(c, fault)
        if not CR.RT.same(a, b):
            changed.append(c.name)
    assert changed, fault


def test_relabel_table_has_the_listed_properties():
    cs = CR.relabel_cases()
    shapes = {(c.boxes.shape[0], c.boxes.shape[1], int(c.gt_n.max())) for c in cs}
    assert shapes >= {(B, R_, G) for B in (1, 3) for R_ in (1, 64, 512) for G in (0, 1, 7, 256)}
    assert all(len({tuple(hw) for hw in c.img_hw}) == len(c.img_hw) for c in cs)          # a different (h, w) per image
    res = {c.name: CR.relabel(c.boxes, c.deltas, c.valid, c.img_hw, c.gtp, c.gt_n, c.reg_w, c.thr) for c in cs}
    big = res["B3-R512-G7-k1"]
    assert 0 < int((big[1] == 0).sum()) and (big[3] != next(c for c in cs if c.name == "B3-R512-G7-k1").valid).any()
    # padding contract of the rows that are not valid
    for c in cs:
        ob, ol, og, ov, oi = res[c.name]
        assert np.array_equal(ob[~ov], np.tile(CR.PAD_BOX, (int((~ov).sum()), 1))) and (ol[~ov] == 1).all() and not og[~ov].any()
        assert not (ov & ~c.valid).any()
        for b in range(len(c.gt_n)):
            if c.gt_n[b] == 0:
                assert (ol[b] == 1).all() and not og[b].any()
    at = next(c for c in cs if c.name == "at-threshold-0.5")
    assert res[at.name][1].tolist() == [[0, 0, 0, 0]]                          # IoU 0.5 exactly, threshold 0.5: foreground (>=)
    at75 = res["at-threshold-0.75"][1].tolist()
    assert at75 == [[1, 0, 1, 1]]                                             # 0.75 >= 0.75 only
    ties = res["ties"]
    assert ties[4].tolist() == [[0, 0, 1]] and ties[1].tolist() == [[0, 0, 0]]
    em = res["empty"]
    assert em[3].tolist() == [[False, False, False, False, True, True]]


@pytest.mark.parametrize("fault", CR.TRAIN_FAULTS)
def test_every_train_fault_changes_a_case(fault):
    changed = []
    for c in CR.relabel_cases():
        a = CR.relabel(c.boxes, c.deltas, c.valid, c.img_hw, c.gtp, c.gt_n, c.reg_w, c.thr)
        b = CR.relabel(c.boxes, c.deltas, c.valid, c.img_hw, c.gtp, c.gt_n, c.reg_w, c.thr, fault)
        if any(not np.array_equal(x, y) for x, y in zip(a[:4], b[:4])):      # what the kernel writes: boxes, labels, matched gt, valid
            changed.append(c.name)
    assert changed, fault
    want = {"keep_empty": "empty", "iou_gt": "at-threshold-0.5", "tie_last": "ties"}[fault]
    assert want in changed, (fault, changed)


def test_launchers_refuse_outside_the_fused_domain_in_the_source():
    """The cascade launchers name the bound they share with the fused tail (read from the source, as test_roitail_host does)."""
    roi = open(os.path.join(PKG, "csrc", "ore_roi.hip")).read()
    src = open(os.path.join(PKG, "csrc", "ore_cascade.hip")).read()
    assert "bool oreroi::fused_domain(int32_t cap, int32_t C) {\n    return cap >= 1 && C >= 1 && cap <= ROI_FUSED_CAP && (size_t)C * 4 * 71 + 6 * 64 * 4 <= 60 * 1024;" in roi
    assert "static bool cascade_domain(int32_t cap, int32_t C) { return oreroi::fused_domain(cap, C); }" in src
    assert src.count("ORE_CHECK_ARG(cascade_domain(cap, C)") == 2
    assert "FUSED_CAP = 512, FUSED_C = (60 * 1024 - 6 * 64 * 4) / (4 * 71)" in src and (60 * 1024 - 6 * 64 * 4) // (4 * 71) == CR.RT.FUSED_C
    assert CR.RT.form(512, 208, 7) == CR.RT.FUSED8 and CR.RT.form(513, 16, 0) == CR.RT.GENERAL
