"""CPU: the float64 references and the plan restatement of tests/s2grad_ref.py (the stride-2 gradient launches, csrc/ore_conv_s2grad.hip)
against torch.autograd in float64, the reach of the shape matrix, the sensitivity of the bound, and the exported symbols."""
import os

import pytest
import torch
import torch.nn.functional as F

import s2grad_ref as SR
import wgrad_ref as WR
from conftest import ROOT

F64 = torch.float64


def _rel(a, b, mag):
    """max over ELEMENTS of |a - b| / mag, mag = the element's sum of absolute terms (A of the device bound): with operands scaled over six
    decades a whole-tensor max-norm would not see an error in a small channel.  An element without terms (mag == 0) must be equal."""
    err = (a - b).abs()
    if bool(((mag == 0) & (err > 0)).any()):
        return float("inf")
    return float(torch.where(mag > 0, err / mag.clamp(min=1e-300), torch.zeros_like(err)).max())


@pytest.mark.parametrize("B,H,W,Cin,Cout", SR.MATRIX + [SR.CAP_SHAPE])
def test_references_equal_torch_autograd(B, H, W, Cin, Cout):
    x, dz = SR.operands(B, H, W, Cin, Cout, seed=3 + H + W)
    w = SR.scaled_weight(Cout, Cin, seed=5 + H)
    xn = x.double().permute(0, 3, 1, 2).requires_grad_(True)
    wn = w.double().requires_grad_(True)
    y = F.conv2d(xn, wn, stride=2, padding=1)
    assert tuple(y.shape[2:]) == SR.out_hw(H, W)
    gx, gw = torch.autograd.grad(y, (xn, wn), dz.double().permute(0, 3, 1, 2))
    rw = SR.wgrad_s2_ref(x, dz)
    assert _rel(rw["dw"], gw, rw["aw"]) <= 1e-12
    ref = SR.dgrad_s2_ref(dz, w, H, W)
    assert _rel(ref["dx"], gx.permute(0, 2, 3, 1), ref["ax"]) <= 1e-12
    assert _rel(SR.dgrad_s2_by_parity(dz, w, H, W), gx.permute(0, 2, 3, 1), ref["ax"]) <= 1e-12     # the kernel's decomposition is the same sum


@pytest.mark.parametrize("B,H,W,Hp,Wp,Cout", SR.STEM1_MATRIX + [SR.STEM1_CAP_SHAPE])
@pytest.mark.parametrize("u8", [True, False])
def test_stem1_reference_equals_torch_autograd(B, H, W, Hp, Wp, Cout, u8):
    """Through normalise + pad, as the reference's preprocess_image + ImageList.from_tensors + stem_1."""
    img = SR.stem1_image(B, H, W, u8, seed=H + W)
    dz = SR.scaled_dz(B, Hp // 2, Wp // 2, Cout, seed=9)
    m = torch.tensor(SR.MEAN).double().view(1, 3, 1, 1)
    s = torch.tensor(SR.STD).double().view(1, 3, 1, 1)
    xn = F.pad((img.double() - m) / s, (0, Wp - W, 0, Hp - H))
    wn = torch.zeros(Cout, 3, 3, 3, dtype=F64, requires_grad=True)
    (gw,) = torch.autograd.grad(F.conv2d(xn, wn, stride=2, padding=1), wn, dz.double().permute(0, 3, 1, 2))
    ref = SR.stem1_wgrad_ref(img, SR.MEAN, SR.STD, Hp, Wp, dz)
    assert _rel(ref["dw"], gw, ref["aw"]) <= 1e-12


def test_shape_matrix_reaches_every_form():
    """Every (split, reduce) form of both weight-gradient plans, counting the capped-workspace cases; the caps give exactly S = cap."""
    forms = set()
    for B, H, W, Cin, Cout in SR.MATRIX:
        Ho, Wo = SR.out_hw(H, W)
        forms.add(SR.wgrad_s2_plan(B * Ho * Wo, Cin, Cout)[2])
    B, H, W, Cin, Cout = SR.CAP_SHAPE
    M, per = B * SR.out_hw(H, W)[0] * SR.out_hw(H, W)[1], Cout * 9 * Cin
    for cap in SR.CAPS:
        plan = SR.wgrad_s2_plan(M, Cin, Cout, cap * per + per // 2)
        assert plan[0] == cap
        forms.add(plan[2])
    assert forms == set(SR.REDUCES), forms
    assert SR.wgrad_s2_plan(2 * 64 * 64, 64, 128) == (64, 128, 16) and SR.wgrad_s2_plan(2 * 32 * 32, 64, 128) == (16, 128, 4)
    forms = set()
    for B, H, W, Hp, Wp, Cout in SR.STEM1_MATRIX:
        forms.add(SR.stem1_wgrad_plan(B * (Hp // 2) * (Wp // 2), Cout)[2])
    B, H, W, Hp, Wp, Cout = SR.STEM1_CAP_SHAPE
    for cap in SR.CAPS:
        plan = SR.stem1_wgrad_plan(B * (Hp // 2) * (Wp // 2), Cout, cap * Cout * 27 + Cout * 13)
        assert plan[0] == cap
        forms.add(plan[2])
    assert forms == set(SR.REDUCES), forms
    with pytest.raises(ValueError):
        SR.wgrad_s2_plan(100, 16, 16, 16 * 9 * 16 - 1)
    # the parity classes: 1, 2, 2 and 4 taps, every input pixel in exactly one class, 2.25 taps per pixel on an even map
    taps = {(py, px): len(t) for py, px, t in SR.dgrad_s2_classes()}
    assert taps == {(0, 0): 1, (0, 1): 2, (1, 0): 2, (1, 1): 4}
    assert SR.dgrad_s2_blocks(5, 1, 1) == [0, 0, 0, 1] and SR.dgrad_s2_blocks(2, 9, 12) == [1, 1, 1, 1]


def test_bound_sees_injected_faults():
    """A dropped tap, a dropped slab, a wrong parity class and a 1e-3 error in one channel each exceed the bound -- with the operands'
    per-channel scales over six decades."""
    B, H, W, Cin, Cout = 2, 64, 64, 64, 128
    Ho, Wo = SR.out_hw(H, W)
    plan = SR.wgrad_s2_plan(B * Ho * Wo, Cin, Cout)
    d = SR.wgrad_depth(plan)
    x, dz = SR.operands(B, H, W, Cin, Cout, seed=1)
    ref = SR.wgrad_s2_ref(x, dz)
    assert SR.check(ref["dw"].float(), ref["dw"], ref["aw"], d) <= 1.0                    # (rounding the result to fp32 is inside the bound)
    assert SR.check(SR.wgrad_s2_ref(x, dz, drop_tap=(0, 2))["dw"].float(), ref["dw"], ref["aw"], d) > 1.0
    S, chunk, _ = plan
    assert SR.check(SR.wgrad_s2_ref(x, dz, drop_rows=(3 * chunk, 4 * chunk))["dw"].float(), ref["dw"], ref["aw"], d) > 1.0
    bad = ref["dw"].clone()
    bad[:, 7] *= 1.0 + 1e-3
    assert SR.check(bad.float(), ref["dw"], ref["aw"], d) > 1.0
    # stem_1: the same faults against the normalised-image reference (+ 2 roundings)
    img = SR.stem1_image(2, 37, 50, True, seed=2)
    dz1 = SR.scaled_dz(2, 32, 32, 16, seed=3)
    p1 = SR.stem1_wgrad_plan(2 * 32 * 32, 16)
    d1 = SR.wgrad_depth(p1, SR.STEM1_EXTRA)
    r1 = SR.stem1_wgrad_ref(img, SR.MEAN, SR.STD, 64, 64, dz1)
    assert SR.check(r1["dw"].float(), r1["dw"], r1["aw"], d1) <= 1.0
    assert SR.check(SR.stem1_wgrad_ref(img, SR.MEAN, SR.STD, 64, 64, dz1, drop_tap=(1, 1))["dw"].float(), r1["dw"], r1["aw"], d1) > 1.0
    assert SR.check(SR.stem1_wgrad_ref(img, SR.MEAN, SR.STD, 64, 64, dz1, drop_rows=(0, p1[1]))["dw"].float(), r1["dw"], r1["aw"], d1) > 1.0
    # data gradient
    B, H, W, Cin, Cout = 2, 9, 12, 64, 128
    _, dz = SR.operands(B, H, W, Cin, Cout, seed=4)
    w = SR.scaled_weight(Cout, Cin, seed=5)
    rd = SR.dgrad_s2_ref(dz, w, H, W)
    dd = SR.dgrad_depth(Cout)
    assert SR.check(SR.dgrad_s2_by_parity(dz, w, H, W).float(), rd["dx"], rd["ax"], dd) <= 1.0
    for cls in ((1, 1), (1, 0), (0, 1), (0, 0)):
        assert SR.check(SR.dgrad_s2_by_parity(dz, w, H, W, wrong_class=cls).float(), rd["dx"], rd["ax"], dd) > 1.0, cls
    bad = rd["dx"].clone()
    bad[..., 11] *= 1.0 + 1e-3
    assert SR.check(bad.float(), rd["dx"], rd["ax"], dd) > 1.0
    w2 = w.clone()
    w2[:, :, 2, 0] = 0                                                                   # a dropped tap
    assert SR.check(SR.dgrad_s2_ref(dz, w2, H, W)["dx"].float(), rd["dx"], rd["ax"], dd) > 1.0


def test_single_pixels_meet_only_the_centre_tap():
    x, dz = SR.operands(5, 1, 1, 32, 32, seed=6)
    dw = SR.wgrad_s2_ref(x, dz)["dw"]
    off = [(a, b) for a in range(3) for b in range(3) if (a, b) != (1, 1)]
    assert all(float(dw[:, :, a, b].abs().max()) == 0.0 for a, b in off) and float(dw[:, :, 1, 1].abs().min()) > 0.0


def test_symbols_declared_and_exported():
    """The three entry points (and their workspace helpers) are in the header and in the built library; the workspace helpers agree with the
    plan restatement.  Host-only calls."""
    import orehip
    names = ("ore_conv2d_wgrad_s2_fwd", "ore_conv2d_dgrad_s2_fwd", "ore_stem1_wgrad_fwd", "ore_conv_wgrad_s2_workspace_floats",
             "ore_conv_dgrad_s2_workspace_floats", "ore_stem1_wgrad_workspace_floats")
    with open(os.path.join(ROOT, "include", "ore_hip.h")) as f:
        header = f.read()
    assert all(n + "(" in header for n in names) and all(n in orehip.SYMBOLS for n in names)
    if not os.path.exists(orehip.LIB_PATH):
        orehip.build()
    L = orehip.lib()
    assert all(hasattr(L, n) for n in names)
    for B, H, W, Cin, Cout in SR.MATRIX + [SR.CAP_SHAPE]:
        M = B * SR.out_hw(H, W)[0] * SR.out_hw(H, W)[1]
        assert L.ore_conv_wgrad_s2_workspace_floats(M, Cin, Cout) == SR.wgrad_s2_workspace(M, Cin, Cout)
        assert L.ore_conv_dgrad_s2_workspace_floats(Cin, Cout) == 9 * Cin * Cout
    for B, H, W, Hp, Wp, Cout in SR.STEM1_MATRIX + [SR.STEM1_CAP_SHAPE]:
        M = B * (Hp // 2) * (Wp // 2)
        assert L.ore_stem1_wgrad_workspace_floats(M, Cout) == SR.stem1_wgrad_workspace(M, Cout)
    for fn in ("conv2d_wgrad_s2", "conv2d_dgrad_s2", "stem1_wgrad"):
        assert callable(getattr(orehip, fn))
    from orehip import autograd as A
    assert all(hasattr(A, n) for n in ("ConvS2Fn", "StemFn", "conv_s2", "stem"))


def test_unfrozen_config_and_depthwise_refusal_is_documented():
    from fewx.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "faster-orefsdet_amd", "configs", "fsod", "finetune_vovnet_unfrozen.yaml"))
    assert cfg.MODEL.BACKBONE.FREEZE_AT == 0 and cfg.MODEL.VOVNET.CONV_BODY == "V-19-slim-eSE"
    from detectron2.layers import ShapeSpec
    from detectron2.modeling.backbone.vovnet import build_vovnet_backbone
    bb = build_vovnet_backbone(cfg, ShapeSpec(channels=3))
    assert all(p.requires_grad for n, p in bb.stem.named_parameters() if n.endswith("conv.weight"))
