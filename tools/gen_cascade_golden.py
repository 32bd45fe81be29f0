"""tests/golden/cascade_stage_eval.npz and cascade_stage_train.npz: the reference's OWN CustomCascadeROIHeads with three cascade stages
(IOUS [0.6, 0.7, 0.8], BBOX_REG_WEIGHTS [[10,10,5,5],[20,20,10,10],[30,30,15,15]]), executed on the CPU through oracle/refrun/shims.py
the way oracle/refrun/gen_golden.py::gen_roi_stage executes the one-stage head: the same 160 x 192 pyramid, 72 proposals with
near-duplicates, three support crops and 7 ground-truth boxes (the same generator seed, 77, drawn in the same order).

    python tools/gen_cascade_golden.py            # writes the two fixtures (this needs the reference tree; no test runs it)

The fixtures are data only.  Weights: oracle.ref_model.synth_roi_state(synth_state_dict(0), 0) plus tests/cascade_ref.py::
synth_cascade_state for the stages 1 and 2, so a test rebuilds them from the seed.

Seeds.  SEED = 0 / generator 77 / randperm 31 are gen_roi_stage's.  The condition on a seed (tests/test_cascade_host.py checks it on the
CPU) is that the composed reference of tests/cascade_ref.py reproduces the executed reference with the SAME kept rows in the same
order and, in training, array-equal labels and matched ground truth in every stage: no NMS decision and no label may sit on a
near-tie that the two exponentials (torch.exp here, ore_expf in the twin) resolve differently.  These seeds satisfy it; none had to be
replaced.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import ref_model as R  # noqa: E402
from oracle.refrun import shims  # noqa: E402
from oracle.refrun.gen_golden import SEED, grad_sample, np_, save, sub_sd  # noqa: E402
import cascade_ref as CR  # noqa: E402

K = 3


def main():
    torch.manual_seed(SEED)
    torch.set_num_threads(8)
    ns = shims.load_roi_heads()
    cfg = shims.logged_cfg()
    cfg.MODEL.ROI_BOX_CASCADE_HEAD.IOUS = list(CR.IOUS)
    cfg.MODEL.ROI_BOX_CASCADE_HEAD.BBOX_REG_WEIGHTS = [list(w) for w in CR.REG_W]
    cfg.MODEL.ROI_HEADS.IOU_THRESHOLDS = [CR.IOUS[0]]
    SS = ns.layers.ShapeSpec
    Boxes, Instances = ns.boxes.Boxes, ns.instances.Instances
    shape = {k: SS(channels=128, stride=st) for k, st in (("p3", 8), ("p4", 16), ("p5", 32))}
    rh = ns.roi_heads.CustomCascadeROIHeads(cfg, shape)
    assert rh.num_cascade_stages == K
    sd = CR.synth_cascade_state(R.synth_roi_state(R.synth_state_dict(SEED), SEED), SEED, K)
    rh.load_state_dict(sub_sd(sd, "roi_heads."), strict=True)
    # ---- gen_roi_stage's inputs, drawn in its order
    g = torch.Generator().manual_seed(77)
    H, W = 160, 192
    feats = {f"p{l}": torch.randn(1, 128, H >> l, W >> l, generator=g) for l in (3, 4, 5)}
    sup8 = torch.randn(3, 128, 8, 8, generator=g) * 0.5
    sup4 = torch.randn(3, 128, 4, 4, generator=g) * 0.5
    n = 72
    wh = torch.exp(torch.rand(n, 1, generator=g) * 4.6 + 1.8) * torch.exp(torch.randn(n, 2, generator=g) * 0.25)
    ctr = torch.rand(n, 2, generator=g) * torch.tensor([W + 20.0, H + 20.0]) - 10.0
    pb = torch.cat([ctr - wh / 2, ctr + wh / 2], 1)
    pb[:8] = pb[8:16] + torch.randn(8, 4, generator=g) * 1.5
    ps = torch.rand(n, generator=g)
    cap = {"boxes": [], "h": {}, "pred": {}}
    rh.box_pooler.register_forward_pre_hook(lambda m, a: cap["boxes"].append(a[1][0].tensor.detach().clone()))
    for k in range(K):
        rh.box_head[k].register_forward_hook(lambda m, i, o, k=k: cap["h"].__setitem__(k, o.detach().clone()))
        rh.box_predictor[k].register_forward_hook(lambda m, i, o, k=k: cap["pred"].__setitem__(k, (o[0].detach().clone(), o[1].detach().clone())))
    # ---- eval
    rh.eval()
    prop = Instances((H, W))
    prop.proposal_boxes, prop.objectness_logits = Boxes(pb.clone()), ps.clone()
    prop.scores, prop.pred_classes = ps.clone(), torch.zeros(n, dtype=torch.int64)
    with torch.no_grad():
        pred, _ = rh(None, feats, [sup8, sup4], [prop])
    pi = pred[0]
    assert len(cap["boxes"]) == K
    ev = {}
    for k in range(K):
        ev[f"boxes{k}"], ev[f"h{k}"] = np_(cap["boxes"][k]), np_(cap["h"][k])
        ev[f"cls_logits{k}"], ev[f"deltas{k}"] = np_(cap["pred"][k][0]), np_(cap["pred"][k][1])
    save("cascade_stage_eval", seed=np.int64(SEED), stages=np.int64(K), ious=np.array(CR.IOUS), reg_weights=np.array(CR.REG_W),
         proposals=np_(pb), proposal_scores=np_(ps), image_hw=np.array([H, W]), **ev,
         pred_boxes=np_(pi.pred_boxes.tensor), scores=np_(pi.scores), pred_classes=np_(pi.pred_classes))
    # ---- train (gen_roi_stage's ground truth and proposals, its randperm seed)
    rh.train()
    n_g = 7
    gwh = torch.rand(n_g, 2, generator=g) * 60 + 20
    gctr = torch.rand(n_g, 2, generator=g) * (torch.tensor([float(W), float(H)]) - gwh) + gwh / 2
    gtb = torch.cat([gctr - gwh / 2, gctr + gwh / 2], 1)
    tp = torch.cat([gtb[torch.randint(0, n_g, (150,), generator=g)] + torch.randn(150, 4, generator=g) * 3.0, pb], 0)
    tp[:, 2:] = torch.max(tp[:, 2:], tp[:, :2] + 2.0)
    prop = Instances((H, W))
    prop.proposal_boxes, prop.objectness_logits = Boxes(tp.clone()), torch.rand(len(tp), generator=g)
    tgt = Instances((H, W))
    tgt.gt_boxes, tgt.gt_classes = Boxes(gtb.clone()), torch.zeros(n_g, dtype=torch.int64)
    for pth in rh.parameters():
        pth.grad = None
    cap["boxes"].clear()
    labelled = {}
    orig = rh._match_and_label_boxes

    def spy(proposals, stage, targets):
        out = orig(proposals, stage, targets)
        labelled[stage] = out[0]
        return out
    rh._match_and_label_boxes = spy
    fl = {k: v.clone().requires_grad_(True) for k, v in feats.items()}
    torch.manual_seed(31)
    sampled, losses = rh(None, fl, [sup8, sup4], [prop], [tgt])
    sum(losses.values()).backward()
    labelled[0] = sampled[0]
    named = dict(rh.named_parameters())
    tr = {}
    for k in range(K):
        sp = labelled[k]
        assert torch.equal(sp.proposal_boxes.tensor, cap["boxes"][k])
        tr[f"roi_boxes{k}"], tr[f"roi_labels{k}"], tr[f"roi_gt{k}"] = np_(sp.proposal_boxes.tensor), np_(sp.gt_classes), np_(sp.gt_boxes.tensor)
        tr[f"loss_cls_stage{k}"], tr[f"loss_box_reg_stage{k}"] = np_(losses[f"loss_cls_stage{k}"]), np_(losses[f"loss_box_reg_stage{k}"])
        tr[f"cls_logits{k}"], tr[f"deltas{k}"] = np_(cap["pred"][k][0]), np_(cap["pred"][k][1])
        tr[f"g_cls_w{k}"] = np_(named[f"box_predictor.{k}.cls_score.weight"].grad)
        tr[f"g_box_w{k}"] = np_(named[f"box_predictor.{k}.bbox_pred.weight"].grad)
        tr[f"g_fc1_b{k}"] = np_(named[f"box_head.{k}.fc1.bias"].grad)
    save("cascade_stage_train", seed=np.int64(SEED), stages=np.int64(K), randperm_seed=np.int64(31), ious=np.array(CR.IOUS),
         reg_weights=np.array(CR.REG_W), proposals=np_(tp), gt=np_(gtb), image_hw=np.array([H, W]), **tr,
         g_conv3_w=np_(named["conv3.weight"].grad), g_conv1_b=np_(named["conv1.bias"].grad),
         **{f"g_{k}_sum": np_(v.grad.sum((0, 2, 3))) for k, v in fl.items() if v.grad is not None},
         dead=np.array([k for k, v in named.items() if v.grad is None]))


if __name__ == "__main__":
    main()
