"""MORE_POS on the GPU (csrc/ore_more_pos.hip): ore_centernet_more_pos_fwd returns, for every fixture
tests/golden/cn_more_pos_*.npz, exactly the list the executed reference returned -- through the list form and the `padded=` form of
orehip.centernet_targets --, the same list run to run; the loss kernels fed that list hold the bounds of tests/trainloss_ref.py and
reproduce the losses the reference returned; the detector of configs/fsod/finetune_vovnet_more_pos.yaml trains through the module path
and through GraphedTrainStep (one capture, parameters equal to the eager run's) and infers exactly as finetune_vovnet.yaml's does; bad
arguments come back as the library's error code."""
import os

import numpy as np
import pytest
import torch

import more_pos_ref as MP
import trainloss_ref as TL
from conftest import PKG
from oracle import ref_model as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
DEV = "cuda"
HP = dict(gamma=2.0, beta=4.0, sigmoid_clamp=1e-4, ignore_high_fp=0.85, alpha=0.25, pos_weight=0.5, neg_weight=0.5, reg_weight=1.0)
SHOTS, HW, SUP = 2, (160, 192), 96


@pytest.fixture(scope="module")
def oh():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import orehip
    orehip.lib()
    return orehip


_CASES = {}


def _case(name):
    if name not in _CASES:
        _CASES[name] = MP.load_case(os.path.join(GOLD, f"cn_more_pos_{name}.npz"))
    return _CASES[name]


def _targets(oh, c, form, head=None, extra_capacity=0):
    head = torch.from_numpy(c["head"]).to(DEV) if head is None else head
    mp = (head, c["thresh"], c["topk"])
    kw = dict(strides=c["strides"], soi=c["soi"], device=DEV)
    if form == "list":
        return oh.centernet_targets([torch.from_numpy(c["gt"][b, :int(n)]).to(DEV) for b, n in enumerate(c["counts"])], c["shapes"],
                                    more_pos=mp, **kw), head
    gt = torch.zeros(c["gt"].shape[0], c["gt"].shape[1] + extra_capacity, 4)
    gt[:, :c["gt"].shape[1]] = torch.from_numpy(c["gt"])
    if extra_capacity:
        gt[:, c["gt"].shape[1]:] = torch.tensor([8.0, 8.0, 40.0, 40.0])            # beyond the count: never an object
    return oh.centernet_targets(None, c["shapes"], padded=(gt.to(DEV), torch.from_numpy(c["counts"]).to(DEV)), more_pos=mp, **kw), head


@pytest.mark.parametrize("form", ["list", "padded", "padded+3"])
@pytest.mark.parametrize("name", MP.CASES)
def test_list_equals_the_reference(oh, name, form):
    """pos_inds[:pos_count] and pos_count equal the fixture exactly; a second run gives the same tensor; capacity B * max_n * L * 9; the
    two target tensors are the ones the call without more_pos gives."""
    c = _case(name)
    cap = 3 if form == "padded+3" and c["gt"].shape[1] + 3 <= 128 else 0
    tg, head = _targets(oh, c, form.split("+")[0], extra_capacity=cap)
    tg2, _ = _targets(oh, c, form.split("+")[0], head=head, extra_capacity=cap)
    n = int(tg["pos_count"].item())
    want = c["pos_inds"]
    print(name, form, "pos_count", n, "fixture", len(want))
    assert tg["pos_inds"].dtype == torch.int64 and tg["pos_count"].dtype == torch.int32
    B, max_n, L = c["gt"].shape[0], max(1, int(c["counts"].max())) if form == "list" else c["gt"].shape[1] + cap, len(c["strides"])
    assert tg["pos_inds"].numel() == B * max_n * L * 9
    assert n == len(want) and np.array_equal(tg["pos_inds"][:n].cpu().numpy(), want)
    assert torch.equal(tg["pos_inds"], tg2["pos_inds"]) and torch.equal(tg["pos_count"], tg2["pos_count"])
    if form == "list":
        plain = oh.centernet_targets([torch.from_numpy(c["gt"][b, :int(k)]).to(DEV) for b, k in enumerate(c["counts"])], c["shapes"],
                                     strides=c["strides"], soi=c["soi"], device=DEV)
        assert torch.equal(plain["reg_targets"], tg["reg_targets"]) and torch.equal(plain["hm_targets"], tg["hm_targets"])
        assert plain["pos_inds"].numel() == B * max_n * L


def _hold(what, got, x, extra_d=0):
    h, r = TL.hold(got, x, extra_d)
    print(f"{what}: hard {h:.3e} rms {r:.3e} d {x.d + extra_d}")
    assert h <= 1 and r <= 1, (what, {"hard": h, "rms": r, "d": x.d + extra_d})


@pytest.mark.parametrize("name", [n for n in MP.CASES if n not in MP.NO_MARGIN])
def test_losses_and_head_gradient_on_the_new_list(oh, name):
    """A.centernet_losses fed the new list: the three losses and d head against the float64 restatements of tests/trainloss_ref.py
    (element and block bounds), the losses also against the ones the reference's forward returned; entries of pos_inds beyond the
    count are never read (they are pointed at another row first)."""
    from orehip import autograd as A
    c = _case(name)
    assert float(TL.cn_margins(c["head"], 1e-4, 0.85).min()) >= TL.S_MARGIN
    tg, _ = _targets(oh, c, "list")
    n = int(tg["pos_count"].item())
    rows = c["head"].shape[0]
    tg["pos_inds"][n:] = rows - 1                                                 # a valid row, but not a positive
    head = torch.from_numpy(c["head"]).to(DEV).requires_grad_(True)
    l3, counts = A.centernet_losses(head, tg["reg_targets"], tg["hm_targets"], tg["pos_inds"], tg["pos_count"], HP, with_counts=True)
    l3.sum().backward()
    ref = TL.centernet_losses_ref(c["head"], tg["reg_targets"], tg["hm_targets"], c["pos_inds"], np.array([n]))
    hm_d = TL.centernet_targets_ref(c["gt"], c["counts"], c["shapes"], c["strides"], c["soi"])["hm"].d
    assert counts.tolist() == [float(ref["count"]), float(n)]
    den = torch.clamp(torch.tensor([float(ref["count"]), float(n)]), min=1.0)      # CenterNetLossFn's fp32 normalisers, one image set
    coef = torch.stack([HP["reg_weight"] / den[0], HP["pos_weight"] * HP["alpha"] / den[1], HP["neg_weight"] * (1.0 - HP["alpha"]) / den[1]])
    for k, i, s in (("giou", 0, 1.0), ("pos", 1, -1.0), ("neg", 2, -1.0)):
        w = s * float(coef[i])
        x = TL.X(ref[k].v * w, ref[k].m * abs(w), ref[k].d)
        _hold(f"{name} loss {k}", l3[i].detach(), x, extra_d=1)
        # the executed reference: weight * sum / normaliser (3 roundings) on its OWN fp32 heat map, which the restatement above took
        # from the kernel as an exact input: the depth of the heat map's chain (tests/trainloss_ref.py::centernet_targets_ref) on top
        _hold(f"{name} loss {k} vs the reference's", torch.tensor([c["losses"][i]], dtype=torch.float64), x, extra_d=3 + hm_d)
    g = TL.centernet_loss_grad_ref(c["head"], tg["reg_targets"], tg["hm_targets"], c["pos_inds"], np.array([n]), coef)
    _hold(f"{name} d head", head.grad[:, :5], g)
    # the tail is not read: the same sums with the tail pointing elsewhere
    a = oh.centernet_loss_sums(head.detach(), tg["reg_targets"], tg["hm_targets"], tg["pos_inds"], tg["pos_count"])
    tg["pos_inds"][n:] = 0
    b = oh.centernet_loss_sums(head.detach(), tg["reg_targets"], tg["hm_targets"], tg["pos_inds"], tg["pos_count"])
    assert torch.equal(a, b)


def test_a_row_named_twice_takes_twice_the_gradient(oh):
    """Case e's overlapping blocks name rows twice.  Against the list that names every row once, with the negative term's coefficient 0:
    the heat-map gradient of a row named twice is EXACTLY twice the single one (k_cn_loss_grad_pos adds one equal addend per entry that
    names the row: 0 + a + a), k times within the k - 1 roundings of k equal addends in case j, and columns 0..3 do not change."""
    for name in ("e", "j"):
        c = _case(name)
        tg, head = _targets(oh, c, "list")
        n = int(tg["pos_count"].item())
        uniq, cnt = torch.unique(tg["pos_inds"][:n], return_counts=True)
        assert int(cnt.max()) >= 2, name
        once = torch.zeros_like(tg["pos_inds"]); once[:len(uniq)] = uniq
        n_once = torch.tensor([len(uniq)], dtype=torch.int32, device=DEV)
        coef = torch.tensor([0.7, 0.3, 0.0], device=DEV)
        d_dup = oh.centernet_loss_grad(head, tg["reg_targets"], tg["hm_targets"], tg["pos_inds"], tg["pos_count"], coef)
        d_one = oh.centernet_loss_grad(head, tg["reg_targets"], tg["hm_targets"], once, n_once, coef)
        k = cnt.to(torch.float32)
        two = cnt == 2
        print(name, "rows named twice:", int(two.sum()), "most often:", int(cnt.max()))
        assert bool((d_one[uniq, 4][two] != 0).any())
        assert torch.equal(d_dup[uniq, 4][cnt <= 2], (d_one[uniq, 4] * k)[cnt <= 2])
        assert torch.allclose(d_dup[uniq, 4], d_one[uniq, 4] * k, rtol=float(cnt.max()) * 2.0 ** -24, atol=0.0)
        assert torch.equal(d_dup[:, :4], d_one[:, :4])
        s_dup = oh.centernet_loss_sums(head, tg["reg_targets"], tg["hm_targets"], tg["pos_inds"], tg["pos_count"])
        s_one = oh.centernet_loss_sums(head, tg["reg_targets"], tg["hm_targets"], once, n_once)
        assert float(s_dup[2]) < float(s_one[2]) < 0.0                           # log p (1 - p)^g < 0 per entry: repeats count again


def test_argument_errors(oh):
    """Bad arguments return the library's error code before any launch."""
    c = _case("f")
    head = torch.from_numpy(c["head"]).to(DEV)
    gt = [torch.from_numpy(c["gt"][0, :2]).to(DEV)]
    kw = dict(strides=c["strides"], soi=c["soi"], device=DEV)
    for thresh, topk in ((0.2, 0), (0.2, 28), (0.0, 9), (-1.0, 9)):
        with pytest.raises(oh.OreError, match="ore_centernet_more_pos_fwd"):
            oh.centernet_targets(gt, c["shapes"], more_pos=(head, thresh, topk), **kw)
    with pytest.raises(oh.OreError, match="more_pos takes"):
        oh.centernet_targets(gt, c["shapes"], more_pos=(head[:-1], 0.2, 9), **kw)
    with pytest.raises(oh.OreError, match="more_pos takes"):
        oh.centernet_targets(gt, c["shapes"], more_pos=(head.double(), 0.2, 9), **kw)
    L = oh.lib()
    import ctypes as C
    H, W, S = (C.c_int32 * 3)(20, 10, 5), (C.c_int32 * 3)(24, 12, 6), (C.c_int32 * 3)(8, 16, 32)
    so = (C.c_float * 6)(0, 64, 48, 192, 128, 1000000)
    g = torch.zeros(1, 1, 4, device=DEV); n = torch.zeros(1, dtype=torch.int32, device=DEV)
    pi = torch.zeros(27, dtype=torch.int64, device=DEV); pc = torch.zeros(1, dtype=torch.int32, device=DEV)
    ok = lambda **o: L.ore_centernet_more_pos_fwd(o.get("L", 3), H, W, S, o.get("B", 1), oh._ptr(g), oh._ptr(n), o.get("max_n", 1), so,
                                                  o.get("head", oh._ptr(head)), o.get("ld", 5), 0.2, 9, o.get("pi", oh._ptr(pi)), oh._ptr(pc),
                                                  oh._stream())
    assert ok() == 0
    torch.cuda.synchronize()
    assert int(pc.item()) == 0
    for bad in (dict(L=0), dict(L=5), dict(B=0), dict(max_n=0), dict(max_n=129), dict(ld=3), dict(head=None), dict(pi=None)):
        assert ok(**bad) != 0, bad
        assert b"ore_centernet_more_pos_fwd" in L.ore_last_error()


# ---- the detector of the new yaml ------------------------------------------------------------------------------------------------
def _cfg(yaml, *extra):
    from fewx.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(PKG, "configs", "fsod", yaml))
    cfg.merge_from_list(["MODEL.DEVICE", "cuda", "INPUT.FS.SUPPORT_SHOT", SHOTS] + list(extra))
    cfg.freeze()
    return cfg


def _model(yaml="finetune_vovnet_more_pos.yaml", *extra):
    from detectron2.modeling import build_model
    cfg = _cfg(yaml, *extra)
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


def _items(n):
    from oracle import ref_train as T
    from detectron2.structures import Boxes, Instances
    items = []
    for b in range(n):
        img, gt, sup, sbox = T.synth_train_inputs(2 + b, HW, n_gt=4 + b, shots=SHOTS, support_hw=SUP)
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


def test_module_path_trains_one_image(oh):
    """CenterNet from the new yaml, one image through proposal_generator(images, features, gt_instances): finite losses, proposals, a
    gradient on the features, and the positives of the call are the MORE_POS list (its capacity says so)."""
    from detectron2.structures import Boxes, ImageList, Instances
    m, cfg = _model()
    pg = m.proposal_generator
    assert pg.more_pos and pg.more_pos_topk == 9
    g = torch.Generator().manual_seed(12)
    H, W = HW
    ctr = torch.rand(5, 2, generator=g) * torch.tensor([float(W), float(H)])
    wh = torch.exp(torch.rand(5, 2, generator=g) * 1.2 + 2.8)
    gt = torch.cat([ctr - wh / 2, ctr + wh / 2], 1).clamp(min=0)
    inst = Instances((H, W))
    inst.gt_boxes, inst.gt_classes = Boxes(gt.cuda()), torch.zeros(5, dtype=torch.int64).cuda()
    feats = {k: (torch.randn(1, 128, H >> s, W >> s, generator=g) * 0.5).cuda().requires_grad_(True) for k, s in (("p3", 3), ("p4", 4), ("p5", 5))}
    images = ImageList(torch.zeros(1, 3, H, W).cuda(), [(H, W)])
    seen = {}
    real = oh.centernet_targets

    def spy(*a, **k):
        o = real(*a, **k)
        seen["more_pos"], seen["numel"], seen["count"] = k.get("more_pos") is not None, o["pos_inds"].numel(), o["pos_count"]
        return o
    oh.centernet_targets = spy
    try:
        props, l3 = pg(images, feats, [inst])
    finally:
        oh.centernet_targets = real
    assert seen["more_pos"] and seen["numel"] == 5 * 3 * 9 and int(seen["count"].item()) >= 1
    assert set(l3) == {"loss_centernet_loc", "loss_centernet_agn_pos", "loss_centernet_agn_neg"}
    assert all(bool(torch.isfinite(v)) for v in l3.values())
    assert len(props) == 1 and len(props[0].proposal_boxes.tensor) > 0 and bool(torch.isfinite(props[0].proposal_boxes.tensor).all())
    sum(l3.values()).backward()
    assert all(bool(torch.isfinite(f.grad).all()) and float(f.grad.abs().max()) > 0 for f in feats.values())


def test_captured_step_equals_eager_step(oh, fixed_keys):
    """GraphedTrainStep over B = 2 at 160 x 192 with 2 shots and MORE_POS on: one capture, no re-capture across 4 steps (2 eager warm-up
    steps, 2 replays), and the parameters after them are torch.equal to four eager steps'."""
    from fewx.solver import GraphedTrainStep, build_optimizer
    items = _items(2)
    res = {}
    for mode in ("eager", "graph"):
        m, cfg = _model()
        assert m.proposal_generator.more_pos
        opt = build_optimizer(cfg, m)
        before = opt.bucket.params.detach().clone()
        stepper = GraphedTrainStep(m, opt, warmup=2) if mode == "graph" else None
        for it in range(4):
            opt.set_lr_factor(0.02 * (1.0 + 0.25 * it))
            if stepper is not None:
                losses = stepper(items)
            else:
                losses = m(items)
                opt.zero_grad()
                sum(losses.values()).backward()
                opt.step()
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(v.detach()).all()) for v in losses.values())
        if stepper is not None:
            assert stepper.error is None, stepper.error
            assert stepper.captures == 1 and stepper.eager_steps == 2 and stepper.replays == 2, (stepper.captures, stepper.eager_steps, stepper.replays)
        after = opt.bucket.params.detach().clone()
        assert bool(torch.isfinite(after).all()) and not torch.equal(before, after)
        res[mode] = after
        del m, opt, stepper
    print("max |eager - graph| parameter difference:", float((res["eager"] - res["graph"]).abs().max()))
    assert torch.equal(res["eager"], res["graph"])


def _item(seed, hw, n_gt):
    from oracle import ref_train as T
    from detectron2.structures import Boxes, Instances
    img, gt, sup, sbox = T.synth_train_inputs(seed, hw, n_gt=n_gt, shots=SHOTS, support_hw=SUP)
    inst = Instances(hw)
    inst.gt_boxes, inst.gt_classes = Boxes(gt), torch.zeros(len(gt), dtype=torch.int64)
    return {"image": img, "instances": inst, "support_images": sup, "support_bboxes": sbox.numpy()}


def test_mixed_size_batch_replays_one_graph(oh, fixed_keys):
    """Two images of different sizes per step, swapping places (GraphedTrainStep(mixed_sizes=True), the canvas form of the targets) with
    MORE_POS on: one capture, and the training of plain eager steps at the bar of tests/test_hip_multiscale_step.py (parameters within
    1e-6 of the largest weight, losses within 1e-5 relative)."""
    from fewx.solver import GraphedTrainStep, build_optimizer
    a, b = _item(2, (160, 192), 5), _item(3, (128, 192), 6)
    batches = [[a, b] if it % 2 == 0 else [b, a] for it in range(4)]
    res = {}
    for mode in ("eager", "graph"):
        m, cfg = _model()
        opt = build_optimizer(cfg, m)
        stepper = GraphedTrainStep(m, opt, warmup=2, mixed_sizes=True) if mode == "graph" else None
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
        if stepper is not None:
            assert stepper.error is None, stepper.error
            assert stepper.captures == 1 and stepper.eager_steps == 2 and stepper.replays == 2, (stepper.captures, stepper.eager_steps, stepper.replays)
        res[mode] = (log, opt.bucket.params.detach().clone())
        del m, opt, stepper
    for it, (le, lg) in enumerate(zip(res["eager"][0], res["graph"][0])):
        for k, v in le.items():
            assert abs(v - lg[k]) <= 1e-5 * max(abs(v), 1e-3), (it, k, v, lg[k])
    pe, pg = res["eager"][1], res["graph"][1]
    print("max |eager - graph| parameter difference:", float((pe - pg).abs().max()))
    assert float((pe - pg).abs().max()) <= 1e-6 * float(pe.abs().max())


def test_bf16_training_selects_on_fp32_head_rows(oh):
    """Under the bf16 training precision the selection still reads fp32 head rows, and the iteration gives finite losses."""
    seen = {}
    real = oh.centernet_targets

    def spy(*a, **k):
        seen["head"] = k["more_pos"][0].dtype if k.get("more_pos") is not None else None
        return real(*a, **k)
    prev = oh.set_conv_precision("bf16")
    oh.centernet_targets = spy
    try:
        m, _ = _model()
        losses = m(_items(1))
        sum(losses.values()).backward()
        torch.cuda.synchronize()
    finally:
        oh.centernet_targets = real
        oh.set_conv_precision(prev)
    assert seen["head"] == torch.float32
    assert all(bool(torch.isfinite(v.detach()).all()) for v in losses.values())


def test_inference_does_not_see_the_switch(oh):
    """MORE_POS is a training rule: the detector of the new yaml returns torch.equal detections to finetune_vovnet.yaml's."""
    H, W = 96, 128
    img = R.synth_image(9, H, W)
    sup = {k: {} for k in ("p3", "p4", "p5", "rcnn_8", "rcnn_4")}
    p = R.synth_support(10)
    for k in ("p3", "p4", "p5"):
        sup[k][7] = p[k]
    sup["rcnn_8"][7] = torch.randn(6, 128, 8, 8, generator=torch.Generator().manual_seed(40)) * 0.1
    sup["rcnn_4"][7] = torch.zeros(6, 128, 4, 4)
    out = {}
    for yaml in ("finetune_vovnet_more_pos.yaml", "finetune_vovnet.yaml"):
        m, _ = _model(yaml, "INPUT.MAX_SIZE_TEST", 128)
        m.eval()
        m.set_support_dict(sup)
        out[yaml] = m([{"image": img, "height": H, "width": W}])[0]["instances"]
        del m
    a, b = out["finetune_vovnet_more_pos.yaml"], out["finetune_vovnet.yaml"]
    assert len(a) > 0
    assert torch.equal(a.pred_boxes.tensor, b.pred_boxes.tensor) and torch.equal(a.scores, b.scores) and torch.equal(a.pred_classes, b.pred_classes)
