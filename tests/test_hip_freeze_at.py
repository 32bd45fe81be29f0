"""MODEL.BACKBONE.FREEZE_AT: 0 on the GPU: the detector of configs/fsod/finetune_vovnet_unfrozen.yaml trains its stem (orehip.autograd.StemFn
on the kernels of csrc/ore_conv_s2grad.hip), changes nothing from stage 2 up, captures into GraphedTrainStep, and a depthwise body says
why it cannot.  Query 224x288 and 96x96 supports: the smallest sizes tests/test_hip_train.py trains at."""
import os

import pytest
import torch

from conftest import PKG
from oracle import ref_model as R

pytestmark = pytest.mark.gpu

SHOTS, HW, SUP = 4, (224, 288), 96
STEM = "backbone.bottom_up.stem."


@pytest.fixture(scope="module")
def oh():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import orehip
    orehip.lib()
    return orehip


def _cfg(*extra):
    from fewx.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(PKG, "configs", "fsod", "finetune_vovnet_unfrozen.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", "cuda", "INPUT.FS.SUPPORT_SHOT", SHOTS] + list(extra))
    cfg.freeze()
    return cfg


def _model(*extra):
    """The training model of tests/test_hip_train.py::_train_model, from the unfrozen config."""
    from detectron2.modeling import build_model
    cfg = _cfg(*extra)
    torch.manual_seed(0)
    m = build_model(cfg)
    sd = R.synth_roi_state(R.synth_state_dict(0), 0)
    sd["roi_heads.box_head.0.fc1.weight"] = sd["roi_heads.box_head.0.fc1.weight"] * 0.02
    sd["proposal_generator.centernet_head.agn_hm.bias"] = torch.full((1,), -2.0)
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and not missing, (missing, unexpected)
    m.train()
    for lvl in (3, 4, 5):
        getattr(m, f"vip_p{lvl}").reweighting.drop.p = 0.0
    return m, cfg


def _items(n=1):
    from oracle import ref_train as T
    from detectron2.structures import Boxes, Instances
    items = []
    for b in range(n):
        img, gt, sup, sbox = T.synth_train_inputs(2 + b, HW, n_gt=5 + b, shots=SHOTS, support_hw=SUP)
        inst = Instances(HW)
        inst.gt_boxes, inst.gt_classes = Boxes(gt.cuda()), torch.zeros(len(gt), dtype=torch.int64).cuda()
        items.append({"image": img.cuda(), "instances": inst, "support_images": sup.cuda(), "support_bboxes": sbox.cuda()})
    return items


@pytest.fixture
def fixed_keys(monkeypatch):
    """The fg / bg subsample draws its keys with torch.rand on the device: the same keys for every run of a test."""
    keys = torch.rand(4, 16384, generator=torch.Generator().manual_seed(3)).cuda()
    real_rand = torch.rand

    def fixed_rand(*shape, **kw):
        if len(shape) == 2 and kw.get("device") is not None and torch.device(kw["device"]).type == "cuda":
            return keys[:shape[0], :shape[1]].clone()
        return real_rand(*shape, **kw)

    monkeypatch.setattr(torch, "rand", fixed_rand)


def _one_iteration(m, items):
    m.zero_grad(set_to_none=True)
    losses = m(items)
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    return {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in m.named_parameters() if p.requires_grad}


def test_stem_receives_gradients_and_the_rest_is_unchanged(oh, fixed_keys):
    """After one iteration at FREEZE_AT 0 every stem parameter has a finite, non-zero gradient (without StemFn it stays None), and every
    other gradient is torch.equal to the same iteration at FREEZE_AT 1: the stem's forward is bit-equal and the launches from stage 2 up
    are the same ones in the same order."""
    items = _items()
    m0, cfg0 = _model()
    assert cfg0.MODEL.BACKBONE.FREEZE_AT == 0
    g0 = _one_iteration(m0, items)
    stem = [n for n in g0 if n.startswith(STEM)]
    assert sorted(stem) == [STEM + f"stem_{i}/conv.weight" for i in (1, 2, 3)], stem
    for n in stem:
        assert g0[n] is not None and bool(torch.isfinite(g0[n]).all()) and float(g0[n].abs().max()) > 0.0, n
    del m0
    m1, _ = _model("MODEL.BACKBONE.FREEZE_AT", 1)
    g1 = _one_iteration(m1, items)
    assert sorted(g1) == sorted(n for n in g0 if not n.startswith(STEM))
    differ = [n for n in g1 if (g1[n] is None) != (g0[n] is None) or (g1[n] is not None and not torch.equal(g1[n], g0[n]))]
    for n in differ[:5]:
        print(n, float((g1[n] - g0[n]).abs().max()), float(g1[n].abs().max()))
    assert not differ, differ[:10]


def test_captured_step_equals_eager_step(oh, fixed_keys):
    """fewx.solver.GraphedTrainStep captures and replays a FREEZE_AT 0 iteration: two eager + two replayed steps leave the parameters of
    four eager steps, and the stem's weights have moved."""
    from fewx.solver import GraphedTrainStep, build_optimizer
    items = _items(2)
    res = {}
    for mode in ("eager", "graph"):
        m, cfg = _model()
        opt = build_optimizer(cfg, m)
        before = m.backbone.bottom_up.stem._modules["stem_1/conv"].weight.detach().clone()
        stepper = GraphedTrainStep(m, opt, warmup=2) if mode == "graph" else None
        for it in range(4):
            opt.set_lr_factor(0.02 * (1.0 + 0.25 * it))
            if stepper is not None:
                stepper(items)
            else:
                losses = m(items)
                opt.zero_grad()
                sum(losses.values()).backward()
                opt.step()
        torch.cuda.synchronize()
        if stepper is not None:
            assert stepper.error is None, stepper.error
            assert stepper.eager_steps == 2 and stepper.replays == 2
        after = m.backbone.bottom_up.stem._modules["stem_1/conv"].weight.detach()
        assert bool(torch.isfinite(after).all()) and not torch.equal(before, after)
        res[mode] = opt.bucket.params.detach().clone()
        del m, opt, stepper
    print("max |eager - graph| parameter difference:", float((res["eager"] - res["graph"]).abs().max()))
    assert torch.equal(res["eager"], res["graph"])


def test_depthwise_body_refuses_to_train_its_stem_and_still_evaluates(oh):
    from detectron2.layers import ShapeSpec
    from detectron2.modeling.backbone.vovnet import build_fcos_vovnet_fpn_backbone
    bb = build_fcos_vovnet_fpn_backbone(_cfg("MODEL.VOVNET.CONV_BODY", "V-19-slim-dw-eSE"), ShapeSpec(channels=3)).cuda()
    x = torch.randn(1, 3, 64, 96, generator=torch.Generator().manual_seed(1)).cuda()
    bb.train()
    with pytest.raises(NotImplementedError, match="ore_dw3x3_fwd"):
        bb(x)
    bb.eval()
    with torch.no_grad():
        out = bb(x)
    assert all(bool(torch.isfinite(out[k]).all()) for k in ("p3", "p4", "p5"))
    # FREEZE_AT >= 1 keeps training the depthwise body as before
    bb1 = build_fcos_vovnet_fpn_backbone(_cfg("MODEL.VOVNET.CONV_BODY", "V-19-slim-dw-eSE", "MODEL.BACKBONE.FREEZE_AT", 1), ShapeSpec(channels=3)).cuda().train()
    y = bb1(x)
    assert y["p3"].requires_grad
