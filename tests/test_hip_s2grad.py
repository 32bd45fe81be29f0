"""The stride-2 gradient kernels (csrc/ore_conv_s2grad.hip: ore_conv2d_wgrad_s2_fwd, ore_conv2d_dgrad_s2_fwd, ore_stem1_wgrad_fwd), the
autograd nodes on them (orehip.autograd.ConvS2Fn, StemFn) and detectron2.layers.Conv2d at stride 2, against float64 references.

tests/s2grad_ref.py restates the host plans, computes the references as shifted-window GEMMs and derives the element-wise bound
|got - ref| <= 2 d u A with d from the plan (its docstring gives the derivation; tests/test_s2grad_host.py checks the references against
torch.autograd and that the bound sees a dropped tap, a dropped slab, a wrong parity class and a 1e-3 error in one channel).  The
operands carry per-channel scales from 1e-3 to 1e3.

ORE_S2GRAD_LOG=<file>: append the largest bound ratio per form to that file."""
import os

import pytest
import torch
import torch.nn.functional as F

import dgrad_ref as DR
import s2grad_ref as SR
import wgrad_ref as WR
from conftest import PKG

pytestmark = pytest.mark.gpu

NAN = float("nan")
_RATIOS = {}
RELU_DEPTH = 2            # ore_relu_affine_bwd: dy * (y > 0) * scale, at most two roundings


@pytest.fixture(scope="module")
def oh():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import orehip
    orehip.lib()
    return orehip


@pytest.fixture(scope="module", autouse=True)
def ratio_report():
    yield
    SR.log_ratios(_RATIOS)


def _within(form, G, ratio, what):
    r0, n0 = _RATIOS.get((form, G), (0.0, 0))
    _RATIOS[(form, G)] = (max(r0, ratio), n0 + 1)
    print(f"{form} reduce {G}: {what}: |got-ref|/bound {ratio:.3e}")
    assert ratio <= 1.0, (form, G, what, ratio)


def _ref_dev(n):
    return "cuda" if n > 2e7 else "cpu"


def _embed(t, ld, coff):
    """t [B,H,W,C] as channels coff .. coff + C of a NaN-filled [B,H,W,ld] tensor."""
    big = torch.full((*t.shape[:3], ld), NAN, device="cuda")
    big[..., coff:coff + t.shape[-1]] = t.cuda()
    return big


# ---- wgrad_s2 / dgrad_s2: the shape matrix --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case():
    """Operands and float64 references of one shape, computed once and shared (never modified)."""
    cache = {}

    def get(B, H, W, Cin, Cout):
        key = (B, H, W, Cin, Cout)
        if key not in cache:
            Ho, Wo = SR.out_hw(H, W)
            M = B * Ho * Wo
            x, dz = SR.operands(B, H, W, Cin, Cout, seed=M + 7 * Cin + Cout)
            w = SR.scaled_weight(Cout, Cin, seed=M + 1)
            dev = _ref_dev(M * Cin * Cout * 9)
            cache[key] = dict(x=x, dz=dz, w=w, wg=SR.wgrad_s2_ref(x, dz, device=dev), dg=SR.dgrad_s2_ref(dz, w, H, W, device=dev))
        return cache[key]
    return get


@pytest.mark.parametrize("B,H,W,Cin,Cout", SR.MATRIX)
def test_wgrad_s2_matrix(oh, case, B, H, W, Cin, Cout):
    c = case(B, H, W, Cin, Cout)
    Ho, Wo = SR.out_hw(H, W)
    plan = SR.wgrad_s2_plan(B * Ho * Wo, Cin, Cout)
    f0, _ = oh.flop_counter()
    gw = oh.conv2d_wgrad_s2(c["x"].cuda(), c["dz"].cuda())
    assert oh.flop_counter()[0] - f0 == 2.0 * B * Ho * Wo * Cout * Cin * 9
    _within("wgrad_s2", plan[2], SR.check(gw, c["wg"]["dw"], c["wg"]["aw"], SR.wgrad_depth(plan)), (B, H, W, Cin, Cout))
    if H * W == 1:                                  # single pixels: every off-centre tap reads outside its image -> exactly 0
        assert float(gw[:, :, [0, 0, 0, 1, 1, 2, 2, 2], [0, 1, 2, 0, 2, 0, 1, 2]].abs().max()) == 0.0


@pytest.mark.parametrize("B,H,W,Cin,Cout", SR.MATRIX)
def test_dgrad_s2_matrix(oh, case, B, H, W, Cin, Cout):
    c = case(B, H, W, Cin, Cout)
    dx = torch.full((B, H, W, Cin), NAN, device="cuda")                      # every element is written, none is read
    oh.conv2d_dgrad_s2(c["dz"].cuda(), c["w"].cuda(), H, W, out=dx)
    _within("dgrad_s2", 0, SR.check(dx, c["dg"]["dx"], c["dg"]["ax"], SR.dgrad_depth(Cout)), (B, H, W, Cin, Cout))
    if H * W == 1:                                  # the centre tap alone: one Cout-long chain
        want = c["dz"].double().reshape(B, Cout) @ c["w"][:, :, 1, 1].double()
        assert SR.check(dx.reshape(B, Cin), want, c["dz"].double().abs().reshape(B, Cout) @ c["w"][:, :, 1, 1].double().abs(), Cout + 1) <= 1.0


# ---- capped workspace -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", SR.CAPS)
def test_wgrad_s2_capped_workspace(oh, case, cap):
    """A workspace of `cap` slabs (+ half a slab) through the C ABI makes the launch split its rows `cap` ways."""
    B, H, W, Cin, Cout = SR.CAP_SHAPE
    c = case(B, H, W, Cin, Cout)
    Ho, Wo = SR.out_hw(H, W)
    per = Cout * 9 * Cin
    n = cap * per + per // 2
    plan = SR.wgrad_s2_plan(B * Ho * Wo, Cin, Cout, n)
    assert plan[0] == cap
    gw = oh.conv2d_wgrad_s2(c["x"].cuda(), c["dz"].cuda(), workspace=torch.empty(n, device="cuda"))
    _within("wgrad_s2", plan[2], SR.check(gw, c["wg"]["dw"], c["wg"]["aw"], SR.wgrad_depth(plan)), ("cap", cap))
    with pytest.raises(oh.OreError):                                      # less than one slab: ORE_ENOMEM
        oh.conv2d_wgrad_s2(c["x"].cuda(), c["dz"].cuda(), workspace=torch.empty(per - 4, device="cuda"))


@pytest.mark.parametrize("cap", SR.CAPS)
def test_stem1_wgrad_capped_workspace(oh, cap):
    B, H, W, Hp, Wp, Cout = SR.STEM1_CAP_SHAPE
    M = B * (Hp // 2) * (Wp // 2)
    n = cap * Cout * 27 + Cout * 13
    plan = SR.stem1_wgrad_plan(M, Cout, n)
    assert plan[0] == cap
    img = SR.stem1_image(B, H, W, True, seed=cap)
    dz = SR.scaled_dz(B, Hp // 2, Wp // 2, Cout, seed=40 + cap)
    ref = SR.stem1_wgrad_ref(img, SR.MEAN, SR.STD, Hp, Wp, dz)
    gw = oh.stem1_wgrad(img.cuda(), Hp, Wp, SR.MEAN, SR.STD, dz.cuda(), workspace=torch.empty(n, device="cuda"))
    _within("stem1_wgrad", plan[2], SR.check(gw, ref["dw"], ref["aw"], SR.wgrad_depth(plan, SR.STEM1_EXTRA)), ("cap", cap))


# ---- argument semantics ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,Cin,Cout", SR.SEMANTICS_SHAPES)
def test_slices_beta_and_determinism(oh, case, B, H, W, Cin, Cout):
    """Channel slices of wider buffers with NaN around them, beta = 1 into existing values, beta = 0 into NaN, and two runs bit-equal."""
    c = case(B, H, W, Cin, Cout)
    Ho, Wo = SR.out_hw(H, W)
    plan = SR.wgrad_s2_plan(B * Ho * Wo, Cin, Cout)
    d = SR.wgrad_depth(plan)
    xv, zv = _embed(c["x"], Cin + 24, 8), _embed(c["dz"], Cout + 12, 4)
    old = torch.randn(Cout, Cin, 3, 3, device="cuda") * c["wg"]["aw"].float().cuda()      # existing values of the gradient's own size
    out = old.clone()
    oh.conv2d_wgrad_s2(xv, zv, x_coff=8, Cin=Cin, dz_coff=4, Cout=Cout, out=out, beta=1.0)
    _within("wgrad_s2", plan[2], SR.check(out, c["wg"]["dw"], c["wg"]["aw"], d, old=old, beta=1.0), ("beta 1, slices", B, H, W))
    out0 = torch.full((Cout, Cin, 3, 3), NAN, device="cuda")
    oh.conv2d_wgrad_s2(xv, zv, x_coff=8, Cin=Cin, dz_coff=4, Cout=Cout, out=out0, beta=0.0)
    _within("wgrad_s2", plan[2], SR.check(out0, c["wg"]["dw"], c["wg"]["aw"], d), ("beta 0 into NaN", B, H, W))
    again = torch.full((Cout, Cin, 3, 3), NAN, device="cuda")
    oh.conv2d_wgrad_s2(xv, zv, x_coff=8, Cin=Cin, dz_coff=4, Cout=Cout, out=again, beta=0.0)
    assert torch.equal(out0, again)
    assert torch.equal(out0, oh.conv2d_wgrad_s2(c["x"].cuda(), c["dz"].cuda()))              # the slices change nothing
    # data gradient: dZ slice in, dX slice out; the channels beside the slice keep their NaN
    dxv = torch.full((B, H, W, Cin + 16), NAN, device="cuda")
    oh.conv2d_dgrad_s2(zv, c["w"].cuda(), H, W, dz_coff=4, out=dxv, out_coff=12)
    _within("dgrad_s2", 0, SR.check(dxv[..., 12:12 + Cin].contiguous(), c["dg"]["dx"], c["dg"]["ax"], SR.dgrad_depth(Cout)), ("slices", B, H, W))
    assert bool(torch.isnan(dxv[..., :12]).all()) and bool(torch.isnan(dxv[..., 12 + Cin:]).all())
    dx2 = oh.conv2d_dgrad_s2(c["dz"].cuda(), c["w"].cuda(), H, W)
    assert torch.equal(dx2, dxv[..., 12:12 + Cin]) and torch.equal(dx2, oh.conv2d_dgrad_s2(c["dz"].cuda(), c["w"].cuda(), H, W))


def test_batches_beyond_one_launch_are_split_into_image_groups(oh, case, monkeypatch):
    """The kernels address a tensor through 32-bit byte offsets; the bindings hand them a batch whose tensors would reach 2 GiB in groups of
    whole images (orehip._S2_MAX_BYTES).  With the limit lowered to one image's bytes a batch of two goes out as two launches: the data
    gradient is bit-equal to the one-launch result, the weight gradients add the second group with beta = 1 -- one more rounding on top of
    a one-image plan."""
    B, H, W, Cin, Cout = 2, 9, 12, 64, 128
    c = case(B, H, W, Cin, Cout)
    x, dz, w = c["x"].cuda(), c["dz"].cuda(), c["w"].cuda()
    dx_one = oh.conv2d_dgrad_s2(dz, w, H, W)
    monkeypatch.setattr(oh, "_S2_MAX_BYTES", H * W * Cin * 4)
    assert oh._s2_image_groups(B, H * W * Cin * 4, 5 * 6 * Cout * 4) == [(0, 1), (1, 2)]
    n0 = oh.flop_counter()[1]
    gw = oh.conv2d_wgrad_s2(x, dz)
    assert oh.flop_counter()[1] - n0 == 2
    d = SR.wgrad_depth(SR.wgrad_s2_plan(5 * 6, Cin, Cout)) + 1
    _within("wgrad_s2", 0, SR.check(gw, c["wg"]["dw"], c["wg"]["aw"], d), "two image groups")
    assert torch.equal(dx_one, oh.conv2d_dgrad_s2(dz, w, H, W))
    Bs, Hs, Ws, Hp, Wp, Cs = 2, 37, 50, 64, 64, 16
    img = SR.stem1_image(Bs, Hs, Ws, True, seed=3)
    dz1 = SR.scaled_dz(Bs, Hp // 2, Wp // 2, Cs, seed=4)
    ref = SR.stem1_wgrad_ref(img, SR.MEAN, SR.STD, Hp, Wp, dz1)
    monkeypatch.setattr(oh, "_S2_MAX_BYTES", (Hp // 2) * (Wp // 2) * Cs * 4)
    plan = SR.stem1_wgrad_plan((Hp // 2) * (Wp // 2), Cs)
    g1 = oh.stem1_wgrad(img.cuda(), Hp, Wp, SR.MEAN, SR.STD, dz1.cuda())
    _within("stem1_wgrad", plan[2], SR.check(g1, ref["dw"], ref["aw"], SR.wgrad_depth(plan, SR.STEM1_EXTRA) + 1), "two image groups")


def test_uncovered_shapes_are_refused(oh):
    x, dz, w = torch.zeros(1, 4, 4, 6, device="cuda"), torch.zeros(1, 2, 2, 8, device="cuda"), torch.zeros(8, 6, 3, 3, device="cuda")
    with pytest.raises(oh.OreError):
        oh.conv2d_wgrad_s2(x, dz)                                            # Cin % 4 != 0
    with pytest.raises(oh.OreError):
        oh.conv2d_dgrad_s2(dz, w, 4, 4)
    with pytest.raises(oh.OreError):                                         # Cout % 16 != 0, and an odd padded size
        oh.stem1_wgrad(torch.zeros(1, 3, 4, 4, device="cuda"), 4, 4, SR.MEAN, SR.STD, dz)
    with pytest.raises(oh.OreError):
        oh.stem1_wgrad(torch.zeros(1, 3, 3, 4, device="cuda"), 3, 4, SR.MEAN, SR.STD, torch.zeros(1, 1, 2, 16, device="cuda"))


def test_fp32_in_bf16_mode(oh, case):
    """The process-wide conv precision does not reach these kernels: bit-equal results in bf16 mode."""
    c = case(2, 9, 12, 64, 128)
    a = oh.conv2d_wgrad_s2(c["x"].cuda(), c["dz"].cuda())
    b = oh.conv2d_dgrad_s2(c["dz"].cuda(), c["w"].cuda(), 9, 12)
    prev = oh.set_conv_precision("bf16")
    try:
        assert torch.equal(a, oh.conv2d_wgrad_s2(c["x"].cuda(), c["dz"].cuda()))
        assert torch.equal(b, oh.conv2d_dgrad_s2(c["dz"].cuda(), c["w"].cuda(), 9, 12))
    finally:
        oh.set_conv_precision(prev)


# ---- stem1_wgrad ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("u8", [True, False], ids=["u8", "f32"])
@pytest.mark.parametrize("B,H,W,Hp,Wp,Cout", SR.STEM1_MATRIX)
def test_stem1_wgrad_matrix(oh, B, H, W, Hp, Wp, Cout, u8):
    M = B * (Hp // 2) * (Wp // 2)
    plan = SR.stem1_wgrad_plan(M, Cout)
    img = SR.stem1_image(B, H, W, u8, seed=H + 3 * W + B)
    dz = SR.scaled_dz(B, Hp // 2, Wp // 2, Cout, seed=M + Cout)
    ref = SR.stem1_wgrad_ref(img, SR.MEAN, SR.STD, Hp, Wp, dz)
    d = SR.wgrad_depth(plan, SR.STEM1_EXTRA)
    gw = oh.stem1_wgrad(img.cuda(), Hp, Wp, SR.MEAN, SR.STD, dz.cuda())
    _within("stem1_wgrad", plan[2], SR.check(gw, ref["dw"], ref["aw"], d), (B, H, W, Hp, Wp, Cout, u8))
    assert torch.equal(gw, oh.stem1_wgrad(img.cuda(), Hp, Wp, SR.MEAN, SR.STD, dz.cuda()))
    # a dZ slice with NaN around it, beta = 1 into existing values
    old = torch.randn(Cout, 3, 3, 3, device="cuda") * ref["aw"].float().cuda()
    out = old.clone()
    oh.stem1_wgrad(img.cuda(), Hp, Wp, SR.MEAN, SR.STD, _embed(dz, Cout + 8, 4), dz_coff=4, Cout=Cout, out=out, beta=1.0)
    _within("stem1_wgrad", plan[2], SR.check(out, ref["dw"], ref["aw"], d, old=old, beta=1.0), ("beta 1, slice", B, H, W, Cout, u8))


# ---- composition: the stem as one autograd node -----------------------------------------------------------------------------------------
def _backbone(body):
    from fewx.config import get_cfg
    from detectron2.layers import ShapeSpec
    from detectron2.modeling.backbone.vovnet import build_vovnet_backbone
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(PKG, "configs", "fsod", "finetune_vovnet_unfrozen.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", "cuda", "MODEL.VOVNET.CONV_BODY", body])
    cfg.freeze()
    bb = build_vovnet_backbone(cfg, ShapeSpec(channels=3))
    g = torch.Generator().manual_seed(17)
    for name, m in bb.stem.named_children():
        if name.endswith("/conv"):
            fan = m.weight.shape[1] * 9
            m.weight.data = torch.randn(m.weight.shape, generator=g) / fan ** 0.5
        elif name.endswith("/norm"):                                         # FrozenBN statistics away from the identity, one negative scale
            m.weight.data = torch.rand(m.weight.shape, generator=g) + 0.5
            m.weight.data[3] *= -1.0
            m.bias.data = torch.randn(m.bias.shape, generator=g) * 0.2
            m.running_mean.data = torch.randn(m.running_mean.shape, generator=g) * 0.1
            m.running_var.data = torch.rand(m.running_var.shape, generator=g) + 0.5
    return bb.cuda().train()


@pytest.mark.parametrize("body", ["V-19-slim-eSE", "V-19-eSE"])
def test_stem_node_forward_bit_equal_and_gradients(oh, body):
    """StemFn at B = 2 on a 40x56 image (unpadded: stem_2 then has 1120 rows, below the 1500 from which its data gradient would run on
    the Winograd kernel, whose bound has its own A -- dgrad_ref).  Forward: torch.equal to the frozen launches.  dW1, dW2, dW3 against a
    float64 restatement that takes its ReLU masks from the device forward (so the backward is linear in dY), A from the same backward on
    absolute values, d_total = the sum of the per-launch depths along the chain."""
    bb = _backbone(body)
    B, H, W = 2, 40, 56
    img = SR.stem1_image(B, H, W, True, seed=23).cuda()
    raw = (SR.MEAN, SR.STD, H, W)
    first = bb.stage2.blocks()[0]
    with torch.no_grad():                                                    # the frozen path's launches (VoVNet.forward, FREEZE_AT >= 1)
        y1 = bb.stem_hip(img, raw)
        y2 = bb._unit("stem_2").hip(y1)
        cat = torch.empty(B, 10, 14, first.cat_ch, device="cuda")
        bb._unit("stem_3").hip(y2, out=cat, out_coff=0)
        want = cat[..., :first.in_ch].contiguous()
    assert y1.shape[0] * y1.shape[1] * y1.shape[2] < 1500
    got = bb._stem_train(img, raw, first.cat_ch)
    assert got.requires_grad and torch.equal(got.detach(), want)
    dY = SR.scaled_dz(B, 10, 14, first.in_ch, seed=29).cuda()
    got.backward(dY)
    conv = {n: bb.stem._modules[n + "/conv"].weight for n in ("stem_1", "stem_2", "stem_3")}
    sc = {n: bb.stem._modules[n + "/norm"].scale_shift()[0].detach().double().cpu() for n in conv}
    w = {n: p.detach().double().cpu() for n, p in conv.items()}
    y1d, y2d, y3d = y1.double().cpu(), y2.double().cpu(), want.double().cpu()
    # float64 backward, and the same on absolute values
    dz3 = dY.double().cpu() * (y3d > 0) * sc["stem_3"]
    a3 = dz3.abs()
    r3 = SR.wgrad_s2_ref(y2d, dz3)
    m3 = SR.wgrad_s2_ref(y2d, a3)["aw"]
    dd = SR.dgrad_s2_ref(dz3, w["stem_3"], 20, 28)
    dz2, a2 = dd["dx"] * (y2d > 0) * sc["stem_2"], dd["ax"] * (y2d > 0) * sc["stem_2"].abs()
    r2 = WR.wgrad_ref(y1d, dz2, 3)
    m2 = WR.wgrad_ref(y1d, a2, 3)["aw"]
    dy1 = F.conv_transpose2d(dz2.permute(0, 3, 1, 2), w["stem_2"], padding=1).permute(0, 2, 3, 1)
    ay1 = F.conv_transpose2d(a2.permute(0, 3, 1, 2), w["stem_2"].abs(), padding=1).permute(0, 2, 3, 1)
    dz1, a1 = dy1 * (y1d > 0) * sc["stem_1"], ay1 * (y1d > 0) * sc["stem_1"].abs()
    r1 = SR.stem1_wgrad_ref(img.cpu(), SR.MEAN, SR.STD, H, W, dz1)
    m1 = SR.stem1_wgrad_ref(img.cpu(), SR.MEAN, SR.STD, H, W, a1)["aw"]
    d3 = RELU_DEPTH + SR.wgrad_depth(SR.wgrad_s2_plan(B * 10 * 14, 64, 128))
    d2 = 2 * RELU_DEPTH + SR.dgrad_depth(128) + WR.rounding_depth(WR.wgrad_plan(B * 20 * 28, 64, 64, 3, False, bias=False))
    d1 = 3 * RELU_DEPTH + SR.dgrad_depth(128) + DR.depth(9 * 64) + SR.wgrad_depth(SR.stem1_wgrad_plan(B * 20 * 28, 64), SR.STEM1_EXTRA)
    _within("stem dW3", 0, SR.check(conv["stem_3"].grad, r3["dw"], m3, d3), body)
    _within("stem dW2", 0, SR.check(conv["stem_2"].grad, r2["dw"], m2, d2), body)
    _within("stem dW1", 0, SR.check(conv["stem_1"].grad, r1["dw"], m1, d1), body)


# ---- detectron2.layers.Conv2d at stride 2 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cout", [48, 40])
@pytest.mark.parametrize("form", ["frozenbn_relu", "bare"])
def test_conv2d_layer_stride2_trains(oh, form, Cout):
    """The training branch no longer raises for 3x3 / stride 2 / pad 1, and its weight, input (and bias) gradients pass the bounds.
    Cout = 40 is no multiple of 16: the forward writes a 48-wide buffer, the backward works on the 40 real channels."""
    from detectron2.layers import Conv2d, FrozenBatchNorm2d
    B, H, W, Cin = 2, 9, 12, 32
    g = torch.Generator().manual_seed(31)
    if form == "frozenbn_relu":
        bn = FrozenBatchNorm2d(Cout)
        bn.weight.data = torch.rand(Cout, generator=g) + 0.5
        bn.bias.data = torch.randn(Cout, generator=g) * 0.2
        bn.running_var.data = torch.rand(Cout, generator=g) + 0.5
        conv = Conv2d(Cin, Cout, 3, stride=2, padding=1, bias=False, norm=bn, activation=F.relu)
    else:
        conv = Conv2d(Cin, Cout, 3, stride=2, padding=1, bias=True)
    conv = conv.cuda()
    xh, dzh = SR.operands(B, H, W, Cin, Cout, seed=37)
    x = xh.cuda().permute(0, 3, 1, 2).requires_grad_(True)                   # logical NCHW over NHWC memory
    y = conv(x)
    assert tuple(y.shape) == (B, Cout, 5, 6)
    y.backward(dzh.cuda().permute(0, 3, 1, 2))
    dz, depth0 = dzh.double(), 0
    if form == "frozenbn_relu":
        scale = conv.norm.scale_shift()[0].detach().double().cpu()
        dz, depth0 = dz * (y.detach().permute(0, 2, 3, 1).double().cpu() > 0) * scale, RELU_DEPTH
    wref = SR.wgrad_s2_ref(xh, dz)
    xref = SR.dgrad_s2_ref(dz, conv.weight.detach().cpu(), H, W)
    plan = SR.wgrad_s2_plan(B * 5 * 6, Cin, Cout)
    _within("Conv2d dW", plan[2], SR.check(conv.weight.grad, wref["dw"], wref["aw"], depth0 + SR.wgrad_depth(plan)), (form, Cout))
    _within("Conv2d dX", 0, SR.check(x.grad.permute(0, 2, 3, 1).contiguous(), xref["dx"], xref["ax"], depth0 + SR.dgrad_depth(Cout)), (form, Cout))
    if form == "bare":                                                       # any summation order of the rows: chains of at most `rows` additions
        rows = B * 5 * 6
        assert SR.check(conv.bias.grad, dz.reshape(rows, Cout).sum(0), dz.abs().reshape(rows, Cout).sum(0), rows) <= 1.0
    # what is still refused says so
    with pytest.raises(NotImplementedError, match="stride"):
        Conv2d(Cin, Cout, 3, stride=2, padding=0).cuda()(x)
    with pytest.raises(NotImplementedError, match="Cout % 4"):
        Conv2d(Cin, 42, 3, stride=2, padding=1).cuda()(x)
