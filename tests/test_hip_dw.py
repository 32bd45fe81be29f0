"""The depthwise VoVNet bodies on the GPU: the three kernels of csrc/ore_conv_dw.hip element-wise against fp64 with derived bounds,
the OSA block's gradients against fp64 autograd of the restatement (tests/vovnet_dw_ref.py), the backbone through the module path and
the engine against the fixtures recorded from the executed reference, and the detector from configs/fsod/finetune_vovnet_dw.yaml end
to end (inference, N-way, one training iteration, captured training steps).

ORE_DW_LOG=<file>: append the largest |got - ref| / bound per kernel to that file."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import PKG, chan_err, rel_err
from oracle import ref_model as R
import vovnet_dw_ref as D

pytestmark = pytest.mark.gpu

NAN = float("nan")
TOL = 1e-4
BODY = "V-19-slim-dw-eSE"
CS = (64, 80, 112, 224)
SHAPES = [((1, 1, 1), 1), ((1, 2, 3), 1), ((2, 13, 19), 1), ((1, 21, 21), 1), ((1, 25, 37), 2), ((2, 6, 8), 2)]
_RATIOS = {}


@pytest.fixture(scope="module")
def oh():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import orehip
    orehip.lib()
    return orehip


@pytest.fixture(scope="module", autouse=True)
def ratio_report():
    yield
    lines = [f"{k:12s} max |got-ref|/bound {r:.3e}  ({n} checks)" for k, (r, n) in sorted(_RATIOS.items())]
    print("\n" + "\n".join(lines))
    log = os.environ.get("ORE_DW_LOG")
    if log and lines:
        with open(log, "a") as f:
            f.write("\n".join(lines) + "\n")


def _within(kind, got, ref, bound, what):
    """got (device, NCHW) within bound of ref (fp64) element by element; a zero bound wants exact equality."""
    err = (got.double().cpu() - ref).abs()
    assert not torch.isnan(err).any(), (kind, what, "NaN in the result")
    ratio = float(torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), err)).max())
    r0, n0 = _RATIOS.get(kind, (0.0, 0))
    _RATIOS[kind] = (max(r0, ratio), n0 + 1)
    assert ratio <= 1.0, (kind, what, ratio)


def _chan_scaled(shape, g, ch_axis=1):
    """Normal values times a per-channel scale running from 1e-3 to 1e3 (shuffled): an error in a small channel fails an element-wise
    bound where a max-norm measure would pass."""
    C = shape[ch_axis]
    sc = 10.0 ** (torch.linspace(-3, 3, C)[torch.randperm(C, generator=g)])
    view = [1] * len(shape)
    view[ch_axis] = C
    return torch.randn(*shape, generator=g) * sc.view(view)


def _embed(t_nchw, ld, coff, head=0, tail=0, into=None):
    """t [B,C,H,W] as channels coff .. coff + C of a [B,H,W,ld] view that starts `head` rows into a NaN-filled allocation with `tail`
    NaN rows behind it (into: write the slice into an existing such view instead).  Returns (view, whole allocation)."""
    B, C, H, W = t_nchw.shape
    M = B * H * W
    if into is None:
        big = torch.full(((head + M + tail) * ld,), NAN, device="cuda")
        v = big[head * ld:(head + M) * ld].view(B, H, W, ld)
    else:
        v, big = into
    v[..., coff:coff + C] = t_nchw.permute(0, 2, 3, 1).cuda()
    return v, big


def _untouched(big_after, big_before, view, coff, C):
    """Nothing outside channels [coff, coff + C) of `view` changed (compared as bits: NaN stays NaN)."""
    a, b = big_after.clone(), big_before.clone()
    lo, n = view.storage_offset(), view.numel()
    for t in (a, b):
        t[lo:lo + n].view(view.shape)[..., coff:coff + C] = 0
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _nchw(v, coff, C):
    return v[..., coff:coff + C].permute(0, 3, 1, 2)


def _unit_operands(C, shape, seed):
    g = torch.Generator().manual_seed(seed)
    B, H, W = shape
    x = _chan_scaled((B, C, H, W), g)
    w_dw = _chan_scaled((C, 1, 3, 3), g, 0) / 3.0
    w_pw = _chan_scaled((C, C, 1, 1), g, 0) / C ** 0.5
    scale = (torch.rand(C, generator=g) + 0.5) * torch.where(torch.rand(C, generator=g) < 0.2, -1.0, 1.0)
    shift = torch.randn(C, generator=g) * 10.0 ** torch.linspace(-2, 2, C)
    return x, w_dw, w_pw, scale, shift


# ---------------------------------------------------------------------------------------------------------------- 1. dwpw
@pytest.mark.parametrize("C", CS)
def test_dwpw_vs_fp64(oh, C):
    for i, (shape, stride) in enumerate(SHAPES):
        x, w_dw, w_pw, scale, shift = _unit_operands(C, shape, 100 * C + i)
        _, ref = D.dwpw_ref(x, w_dw, w_pw, scale, shift, stride)
        bound = D.dwpw_bound(x, w_dw, w_pw, scale, shift, stride)
        B, _, Ho, Wo = ref.shape
        xc, oc = 12, 20
        xv, _ = _embed(x, C + 28, xc, head=7, tail=2 * shape[2] + 9)
        ov, obig = _embed(torch.full((B, C, Ho, Wo), NAN), C + 36, oc, head=5, tail=11)
        before = obig.clone()
        out = oh.dwpw(xv, w_dw.cuda(), oh.pack_conv_weight(w_pw.cuda()), C, stride, scale.cuda(), shift.cuda(), in_coff=xc, out=ov, out_coff=oc)
        assert out is ov
        _within("dwpw", _nchw(ov, oc, C), ref, bound, (C, shape, stride))
        assert _untouched(obig, before, ov, oc, C), (C, shape, stride)
        # plain contiguous tensors, no scale / shift
        got = oh.dwpw(x.permute(0, 2, 3, 1).contiguous().cuda(), w_dw.cuda(), oh.pack_conv_weight(w_pw.cuda()), C, stride)
        one, zero = torch.ones(C), torch.zeros(C)
        _within("dwpw", got.permute(0, 3, 1, 2), D.dwpw_ref(x, w_dw, w_pw, one, zero, stride)[1],
                D.dwpw_bound(x, w_dw, w_pw, one, zero, stride), (C, shape, stride, "plain"))


@pytest.mark.parametrize("C", (80, 224))
def test_dwpw_same_buffer_chain(oh, C):
    """Input and output are slices of ONE buffer at different offsets (the OSA chain); everything else in it stays as it was."""
    shape = (2, 13, 19)
    x, w_dw, w_pw, scale, shift = _unit_operands(C, shape, 7 * C)
    ld = 2 * C + 24
    xc, oc = C + 16, 4
    v, big = _embed(x, ld, xc, head=3, tail=40)
    before = big.clone()
    oh.dwpw(v, w_dw.cuda(), oh.pack_conv_weight(w_pw.cuda()), C, 1, scale.cuda(), shift.cuda(), in_coff=xc, out=v, out_coff=oc)
    _within("dwpw", _nchw(v, oc, C), D.dwpw_ref(x, w_dw, w_pw, scale, shift)[1], D.dwpw_bound(x, w_dw, w_pw, scale, shift), (C, "chain"))
    assert _untouched(big, before, v, oc, C)
    assert torch.equal(_nchw(v, xc, C).cpu(), x)


@pytest.mark.parametrize("stride", (1, 2))
def test_dwpw_no_halo_across_the_batch(oh, stride):
    """Image 0 all zeros, image 1 large: image 0's output is relu(shift) exactly."""
    C = 112
    x, w_dw, w_pw, scale, shift = _unit_operands(C, (2, 6, 8), 5)
    x[0] = 0.0
    x[1] = x[1] * 1e6
    got = oh.dwpw(x.permute(0, 2, 3, 1).contiguous().cuda(), w_dw.cuda(), oh.pack_conv_weight(w_pw.cuda()), C, stride, scale.cuda(), shift.cuda())
    want = F.relu(shift).view(1, 1, C).expand(got.shape[1] * got.shape[2], 1, C).reshape(got.shape[1], got.shape[2], C)
    assert torch.equal(got[0].cpu(), want)
    assert float(got[1].abs().max()) > 1e3


def test_dwpw_planner_runs_the_composition_where_it_measured_faster(oh):
    """At stride 1 with rows * C >= 2^22 (stem_2 at 640x640; here the smallest such shape) orehip.dwpw runs k_dw3x3 + the 1x1 conv
    launch, fp32 whatever the conv precision mode is; both forms hold test 1's bound."""
    C, shape = 64, (1, 256, 256)
    assert oh.dwpw_prefers_composition(256 * 256, C, 1) and not oh.dwpw_prefers_composition(256 * 256 - 1, C, 1)
    assert not oh.dwpw_prefers_composition(1 << 20, C, 2) and not oh.dwpw_prefers_composition(160 * 160, 64, 1)
    x, w_dw, w_pw, scale, shift = _unit_operands(C, shape, 77)
    ref, bound = D.dwpw_ref(x, w_dw, w_pw, scale, shift)[1], D.dwpw_bound(x, w_dw, w_pw, scale, shift)
    xv, _ = _embed(x, C + 8, 4, head=3, tail=600)
    args = (xv, w_dw.cuda(), oh.pack_conv_weight(w_pw.cuda()), C, 1, scale.cuda(), shift.cuda())
    prev = oh.set_conv_precision("bf16")
    try:
        ov, obig = _embed(torch.full(tuple(ref.shape), NAN), C + 12, 8, head=2, tail=5)
        before = obig.clone()
        oh.flop_counter(reset=True)
        oh.dwpw(*args, in_coff=4, out=ov, out_coff=8)
        flops, calls = oh.flop_counter()
        assert calls == 2 and flops == 2.0 * 256 * 256 * C * (9 + C)                     # k_dw3x3 + the 1x1 conv launch, counted as one unit's work
        _within("dwpw_planned", _nchw(ov, 8, C), ref, bound, "composition")
        assert _untouched(obig, before, ov, 8, C)
    finally:
        oh.set_conv_precision(prev)
    oh.flop_counter(reset=True)
    fused = oh.dwpw(*args, in_coff=4, fused=True)
    assert oh.flop_counter() == (2.0 * 256 * 256 * C * (9 + C), 1)
    _within("dwpw", fused.permute(0, 3, 1, 2), ref, bound, "fused at the planner's shape")


def test_dw_c_abi_refuses_misaligned_and_overlapping(oh):
    C = 64
    buf = torch.zeros(4 * 4 * 2 * C + 8, device="cuda")
    v = buf[:4 * 4 * 2 * C].view(1, 4, 4, 2 * C)
    w9, wp = torch.zeros(C * 9, device="cuda"), torch.zeros(C * C, device="cuda")
    L = oh.lib()
    call = lambda inp, ic, out, oc: L.ore_dwpw_fwd(inp, 2 * C, ic, 1, 4, 4, C, 1, w9.data_ptr(), wp.data_ptr(), None, None, out, 2 * C, oc, None)
    assert call(v.data_ptr() + 4, 0, v.data_ptr(), C) == -22 and b"aligned" in L.ore_last_error()
    assert call(v.data_ptr(), 0, v.data_ptr(), 32) == -22 and b"overlap" in L.ore_last_error()
    assert L.ore_dw3x3_fwd(v.data_ptr(), 2 * C, 0, 1, 4, 4, C, 1, w9.data_ptr(), 0, v.data_ptr(), 2 * C, 16, 0, None) == -22
    assert call(v.data_ptr(), 0, v.data_ptr(), C) == 0                       # side by side in every row: the OSA chain
    torch.cuda.synchronize()


def test_dwpw_argument_errors(oh):
    x = torch.zeros(1, 4, 4, 72, device="cuda")
    w9, wp = torch.zeros(72 * 9, device="cuda"), torch.zeros(72 * 72, device="cuda")
    with pytest.raises(oh.OreError, match="multiple of 16"):
        oh.dwpw(x, w9, wp, 72)
    x = torch.zeros(1, 4, 4, 64, device="cuda")
    with pytest.raises(oh.OreError, match="stride"):
        oh.dwpw(x, torch.zeros(576, device="cuda"), torch.zeros(4096, device="cuda"), 64, 3, out=torch.zeros(1, 2, 2, 64, device="cuda"))


# ---------------------------------------------------------------------------------------------------------------- 2. dw3x3
@pytest.mark.parametrize("C", CS)
def test_dw3x3_forward_and_data_gradient(oh, C):
    for i, (shape, stride) in enumerate(SHAPES):
        x, w_dw, _, _, _ = _unit_operands(C, shape, 300 * C + i)
        for flip in ((False, True) if stride == 1 else (False,)):
            ref = D.dw3x3_ref(x.double(), w_dw, stride, flip)
            bound = D.dw3x3_bound(x, w_dw, stride, flip)
            xc, oc = 8, 4
            xv, _ = _embed(x, C + 20, xc, head=9, tail=2 * shape[2] + 5)
            ov, obig = _embed(torch.full(tuple(ref.shape), NAN), C + 12, oc, head=2, tail=6)
            before = obig.clone()
            oh.dw3x3(xv, w_dw.cuda(), C, stride, in_coff=xc, out=ov, out_coff=oc, dgrad=flip)
            _within("dw3x3" + ("_dgrad" if flip else ""), _nchw(ov, oc, C), ref, bound, (C, shape, stride, flip))
            assert _untouched(obig, before, ov, oc, C)
            if flip:                                                    # accumulate into what the slice holds
                g = torch.Generator().manual_seed(i)
                old = _chan_scaled(tuple(ref.shape), g)
                ov2, _ = _embed(old, C + 12, oc, head=2, tail=6)
                oh.dw3x3(xv, w_dw.cuda(), C, 1, in_coff=xc, out=ov2, out_coff=oc, dgrad=True, accumulate=True)
                _within("dw3x3_dgrad", _nchw(ov2, oc, C), ref + old.double(), bound + 2 * D.U24 * (ref.abs() + old.abs().double()),
                        (C, shape, "accumulate"))


def test_dw3x3_data_gradient_is_the_adjoint(oh):
    """<dgrad(dt), x> == <dt, dw3x3(x)> in fp64 of the device results (the flipped-tap form really is the transpose)."""
    C = 80
    x, w_dw, _, _, _ = _unit_operands(C, (2, 13, 19), 1)
    g = torch.Generator().manual_seed(2)
    dt = torch.randn(2, C, 13, 19, generator=g)
    y = oh.dw3x3(x.permute(0, 2, 3, 1).contiguous().cuda(), w_dw.cuda(), C)
    dx = oh.dw3x3(dt.permute(0, 2, 3, 1).contiguous().cuda(), w_dw.cuda(), C, dgrad=True)
    a = (dx.double().cpu().permute(0, 3, 1, 2) * x.double()).sum((0, 2, 3))
    b = (dt.double() * y.double().cpu().permute(0, 3, 1, 2)).sum((0, 2, 3))
    assert float(((a - b).abs() / b.abs().clamp(min=1e-30)).max()) < 1e-4


def test_dw3x3_data_gradient_refuses_stride_2(oh):
    x = torch.zeros(1, 6, 8, 64, device="cuda")
    with pytest.raises(oh.OreError, match="stride 1 only"):
        oh.dw3x3(x, torch.zeros(576, device="cuda"), 64, 2, dgrad=True)


# ---------------------------------------------------------------------------------------------------------------- 3. dw3x3_wgrad
@pytest.mark.parametrize("C,shape", [(c, s) for c in CS for s, st in SHAPES if st == 1] + [(96, (2, 40, 40)), (112, (1, 25, 37))])
def test_dw3x3_wgrad_vs_fp64(oh, C, shape):
    g = torch.Generator().manual_seed(C + shape[1])
    B, H, W = shape
    x = _chan_scaled((B, C, H, W), g)
    dt = _chan_scaled((B, C, H, W), g)
    ref, bound = D.dw3x3_wgrad_ref(x, dt), D.dw3x3_wgrad_bound(x, dt)
    xc, dc = 16, 4
    xv, _ = _embed(x, C + 40, xc, head=5, tail=2 * W + 30)
    dv, _ = _embed(dt, C + 8, dc, head=1, tail=3)
    got = oh.dw3x3_wgrad(xv, dv, C, x_coff=xc, dt_coff=dc)
    assert tuple(got.shape) == (C, 1, 3, 3)
    _within("dw3x3_wgrad", got, ref, bound, (C, shape))
    again = oh.dw3x3_wgrad(xv, dv, C, x_coff=xc, dt_coff=dc)
    assert torch.equal(got, again)                                          # fixed split, fixed combine order
    # beta = 0 into NaN, beta = 1 into existing values
    out = torch.full((C, 1, 3, 3), NAN, device="cuda")
    oh.dw3x3_wgrad(xv, dv, C, x_coff=xc, dt_coff=dc, out=out, beta=0.0)
    assert torch.equal(out, got)
    old = _chan_scaled((C, 1, 3, 3), g, 0) * float(ref.abs().mean())
    out = old.clone().cuda()
    oh.dw3x3_wgrad(xv, dv, C, x_coff=xc, dt_coff=dc, out=out, beta=1.0)
    _within("dw3x3_wgrad", out, ref + old.double(), bound + 2 * D.U24 * (ref.abs() + old.abs().double()), (C, shape, "beta 1"))


# ---------------------------------------------------------------------------------------------------------------- 4. the block's gradients
def _block_params(in_ch, C, out_ch, g, reduction):
    def he(co, ci, k=1, gain=2.0):
        return torch.randn(co, ci, k, k, generator=g) * (gain / (ci * k * k)) ** 0.5

    def bn(c):
        return torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.1
    red = (he(C, in_ch), *bn(C)) if reduction else None
    layers = [(torch.randn(C, 1, 3, 3, generator=g) / 3.0, he(C, C), *bn(C)) for _ in range(3)]
    concat = (he(out_ch, in_ch + 3 * C), *bn(out_ch))
    return red, layers, concat


@pytest.mark.parametrize("in_ch,C,out_ch,shape", [(256, 96, 384, (2, 9, 11)), (64, 64, 112, (1, 8, 8))])
def test_osa_block_dw_gradients(oh, monkeypatch, in_ch, C, out_ch, shape):
    from orehip import autograd as A
    g = torch.Generator().manual_seed(in_ch)
    B, H, W = shape
    red, layers, concat = _block_params(in_ch, C, out_ch, g, in_ch != C)
    x = F.relu(torch.randn(B, in_ch, H, W, generator=g))
    dy = torch.randn(B, out_ch, H, W, generator=g)

    def device_run(direct):
        dev = lambda t: t.cuda().requires_grad_(t.dim() == 4)               # conv weights need gradients, folded BN vectors do not
        xd = x.permute(0, 2, 3, 1).contiguous().cuda().requires_grad_(True)
        r = tuple(dev(t) for t in red) if red else None
        ls = [tuple(dev(t) for t in l) for l in layers]
        c = tuple(dev(t) for t in concat)
        ws = ([r[0]] if r else []) + [t for l in ls for t in l[:2]] + [c[0]]
        if direct:                                                          # kernels accumulate into .grad in place (FlatBucket's contract)
            for w in ws:
                w.grad = torch.zeros_like(w)
                w._ore_direct_grad = True
        y = A.osa_block_dw(xd, r, ls, c)
        y.backward(dy.permute(0, 2, 3, 1).contiguous().cuda())
        return y.detach(), xd.grad, [w.grad for w in ws]

    y, dx, dws = device_run(False)
    # the fp64 reference with the ReLU masks of the device forward (a pre-activation near zero cannot flip a mask)
    d = torch.float64
    to64 = lambda tup: tuple(t.to(d).requires_grad_(t.dim() == 4) for t in tup)
    r64, l64, c64 = (to64(red) if red else None), [to64(l) for l in layers], to64(concat)
    x64 = x.to(d).requires_grad_(True)
    _, pres = D.osa_block_dw_ref(x64, r64, l64, c64)
    # device masks: recompute the block's pieces on the device (bit-equal to what the block ran).  Each is checked against the fp64
    # pre-activation of ITS layer on the device's actual input of that layer: wherever that exceeds the layer's forward bound (test
    # 1's; the 1x1 form for the reduction and the concat conv) the device mask is the fp64 mask.  Nothing is carried between layers,
    # so the bound stays tight and nearly every element is compared.
    with torch.no_grad():
        nchw64 = lambda t: t.permute(0, 3, 1, 2).cpu().double()
        xn = x.permute(0, 2, 3, 1).contiguous().cuda()
        cat = torch.empty(B, H, W, in_ch + 3 * C, device="cuda")
        cat[..., :in_ch] = xn
        masks, local, r = [], [], None
        if red:                                                             # exactly the block's calls: same buffers, slices, plans
            r = oh.conv2d(cat, oh.pack_conv_weight(red[0].cuda()), C, 1, 1, 0, in_coff=0, Cin=in_ch, scale=red[1].cuda(), shift=red[2].cuda(),
                          relu_cout=C)
            masks.append(r > 0)
            local.append(D.conv1x1_pre_and_bound(nchw64(xn), *red))
        for i, (wd, wp, sc, sh) in enumerate(layers):
            src_buf, src = (r, 0) if (i == 0 and red) else (cat, in_ch + (i - 1) * C if i else 0)
            dst = in_ch + i * C
            inp = nchw64(src_buf[..., src:src + C])
            oh.dwpw(src_buf, wd.cuda(), oh.pack_conv_weight(wp.cuda()), C, 1, sc.cuda(), sh.cuda(), in_coff=src, out=cat, out_coff=dst)
            masks.append(cat[..., dst:dst + C] > 0)
            local.append((D.dwpw_ref(inp, wd, wp, sc, sh)[0], D.dwpw_bound(inp, wd, wp, sc, sh)))
        assert torch.equal(oh.conv2d(cat, oh.pack_conv_weight(concat[0].cuda()), out_ch, 1, 1, 0, scale=concat[1].cuda(), shift=concat[2].cuda(),
                                     relu_cout=out_ch), y)
        masks.append(y > 0)
        local.append(D.conv1x1_pre_and_bound(nchw64(cat), *concat))
        masks = [m.permute(0, 3, 1, 2).cpu() for m in masks]
    for m, (p, b) in zip(masks, local):
        clear = p.abs() > b
        print(f"osa_block_dw {in_ch}->{C}: {float(clear.float().mean()):.4f} of a pre-activation lies outside its forward bound")
        assert float(clear.float().mean()) > 0.99
        assert torch.equal(m[clear], (p > 0)[clear])
    y64, _ = D.osa_block_dw_ref(x64, r64, l64, c64, masks=masks)
    y64.backward(dy.to(d))
    assert rel_err(y.permute(0, 3, 1, 2).cpu().numpy(), y64.detach().numpy()) < TOL
    w64 = ([r64[0]] if r64 else []) + [t for l in l64 for t in l[:2]] + [c64[0]]
    for name, got, want in [("dX", dx.permute(0, 3, 1, 2), x64.grad)] + [(f"dW{i}", a, b.grad) for i, (a, b) in enumerate(zip(dws, w64))]:
        got, want = got.cpu().numpy(), want.numpy()
        r_, c_ = rel_err(got, want), chan_err(got, want, axis=1 if name == "dX" else 0)
        print(f"osa_block_dw {in_ch}->{C} {name}: rel_err {r_:.2e} chan_err {c_:.2e}")
        assert r_ < TOL and c_ < TOL, (name, r_, c_)
    # run-to-run bit equality, and in-place accumulation into .grad equals the returned-gradient form
    y2, dx2, dws2 = device_run(False)
    assert torch.equal(y, y2) and torch.equal(dx, dx2) and all(torch.equal(a, b) for a, b in zip(dws, dws2))
    # ... and the in-place path really ran: every weight-gradient launch was handed the parameter's .grad with beta = 1 (had
    # direct_grad() declined, autograd's own accumulation into the zeroed .grad would give the same bits)
    seen = []
    for fn in ("conv2d_wgrad", "dw3x3_wgrad"):
        real = getattr(oh, fn)
        monkeypatch.setattr(oh, fn, lambda *a, _real=real, **kw: (seen.append((kw.get("out"), kw.get("beta"))), _real(*a, **kw))[1])
    _, dx3, dws3 = device_run(True)
    assert torch.equal(dx, dx3) and all(torch.equal(a, b) for a, b in zip(dws, dws3))
    assert len(seen) == len(dws3) and all(b == 1.0 for _, b in seen)
    assert sorted(o.data_ptr() for o, _ in seen) == sorted(g.data_ptr() for g in dws3)


# ---------------------------------------------------------------------------------------------------------------- 5. backbone and engine
def _cfg(extra=()):
    from fewx.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(PKG, "configs", "fsod", "finetune_vovnet_dw.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", "cuda"] + list(extra))
    cfg.freeze()
    return cfg


def _close(got, want, what):
    got = got.detach().cpu().numpy()
    assert tuple(got.shape) == tuple(want.shape), (what, got.shape, want.shape)
    r, c = rel_err(got, want), chan_err(got, want)
    print(f"{what}: rel_err {r:.2e} chan_err {c:.2e}")
    assert r < TOL and c < TOL, (what, r, c)


@pytest.fixture(scope="module")
def backbone(oh, golden):
    from detectron2.layers import ShapeSpec
    from detectron2.modeling.backbone.vovnet import build_fcos_vovnet_fpn_backbone
    seed = int(golden("backbone_fpn_dw_96x128")["seed"])
    bb = build_fcos_vovnet_fpn_backbone(_cfg(), ShapeSpec(channels=3))
    sd = D.synth_state_dict_dw(seed, BODY)
    bb.load_state_dict({k[len("backbone."):]: v for k, v in sd.items() if k.startswith("backbone.")}, strict=True)
    return bb.cuda().eval(), sd


def test_module_path_reproduces_the_reference(oh, backbone, golden):
    bb, _ = backbone
    fx = golden("backbone_fpn_dw_96x128")
    with torch.no_grad():
        out = bb(torch.from_numpy(fx["x"]).cuda())
    for k in ("p3", "p4", "p5"):
        _close(out[k], fx[k], "module " + k)
    # the single units and stages of dw_units.npz through the same modules
    u = golden("dw_units")
    bu = bb.bottom_up
    nhwc = lambda k: torch.from_numpy(u[k]).permute(0, 2, 3, 1).contiguous().cuda()
    with torch.no_grad():
        _close(bu._unit("stem_2").hip(nhwc("stem2_x")).permute(0, 3, 1, 2), u["stem2_y"], "stem_2")
        _close(bu._unit("stem_3").hip(nhwc("stem3_x")).permute(0, 3, 1, 2), u["stem3_y"], "stem_3")
        for k in (3, 5):
            blk = getattr(bu, f"stage{k}").blocks()[0]
            pooled = oh.maxpool3x3s2(nhwc(f"stage{k}_x"))
            cat = torch.empty(*pooled.shape[:3], blk.cat_ch, device="cuda")
            cat[..., :blk.in_ch] = pooled
            y, gate = blk.hip(cat)
            _close(oh.scale_channels(y, gate).permute(0, 3, 1, 2), u[f"stage{k}_y"], f"stage{k}")


def test_engine_reproduces_the_reference(oh, backbone, golden):
    """Engine(depthwise=True) at max_batch = 2 (the engine runs whole passes: the single units of dw_units.npz are the module path's)."""
    _, sd = backbone
    fx = golden("backbone_fpn_dw_96x128")
    spec = D.DW_SPECS[BODY]
    e = oh.Engine(stem=spec["stem"], conv=spec["conv"], out=spec["out"], max_batch=2, max_h=96, max_w=128, depthwise=True)
    e.load_state_dict(sd)
    e.set_support(R.synth_support(0))
    e.finalize()
    x = (torch.from_numpy(fx["x"]) + torch.tensor(R.PIXEL_MEAN).view(1, 3, 1, 1)).contiguous().cuda()
    out = e.backbone(x)
    for k in ("p3", "p4", "p5"):
        _close(out[k], fx[k], "engine " + k)
    M = [2 * (96 >> s) * (128 >> s) for s in range(1, 6)]                  # rows at strides 2 .. 32
    want = 2.0 * M[0] * 27 * 64 + oh.lib().ore_dwpw_flops(M[0], 64) + oh.lib().ore_dwpw_flops(M[1], 64)
    cin = 64
    for s, (c, o) in enumerate(zip(spec["conv"], spec["out"])):
        m = M[s + 1]
        want += (2.0 * m * cin * c if cin != c else 0.0) + 3 * 2.0 * m * c * (9 + c) + 2.0 * m * (cin + 3 * c) * o
        cin = o
    for l, o in enumerate(spec["out"][1:]):
        want += 2.0 * M[l + 2] * o * 128 + 2.0 * M[l + 2] * 128 * 128 * 9
    assert e.last_flops() == want
    # one image through the whole pass: the graph replay equals the first call bit for bit
    img = x[1].contiguous()
    e.eval_forward(img, use_graph=True)
    torch.cuda.synchronize()
    first = [e.buffer(f"head{l}", (1, 96 >> l, 128 >> l)).clone() for l in (3, 4, 5)] + [e.buffer(f"p{l}", (1, 96 >> l, 128 >> l)).clone() for l in (3, 4, 5)]
    e.eval_forward(img, use_graph=True)
    torch.cuda.synchronize()
    second = [e.buffer(f"head{l}", (1, 96 >> l, 128 >> l)) for l in (3, 4, 5)] + [e.buffer(f"p{l}", (1, 96 >> l, 128 >> l)) for l in (3, 4, 5)]
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    e.close()


def test_engine_needs_the_dw_names_and_refuses_bf16_storage(oh, backbone):
    _, sd = backbone
    spec = D.DW_SPECS[BODY]
    e = oh.Engine(stem=spec["stem"], conv=spec["conv"], out=spec["out"], max_h=96, max_w=128, depthwise=True)
    e.load_state_dict(R.synth_state_dict(0))                                # the dense body's names
    with pytest.raises(oh.OreError, match="dw_conv3x3"):
        e.finalize()
    e.close()
    prev = oh.set_conv_precision("bf16s")
    try:
        with pytest.raises(oh.OreError, match="depthwise"):
            oh.Engine(stem=spec["stem"], conv=spec["conv"], out=spec["out"], max_h=96, max_w=128, depthwise=True)
    finally:
        oh.set_conv_precision(prev)


# ---------------------------------------------------------------------------------------------------------------- 6. end to end
def _detector(train=False, shots=4):
    from detectron2.modeling import build_model
    cfg = _cfg(["INPUT.MAX_SIZE_TEST", 128, "INPUT.FS.SUPPORT_SHOT", shots])
    torch.manual_seed(0)
    m = build_model(cfg)
    sd = R.synth_roi_state(D.synth_state_dict_dw(1, BODY), 0)
    sd["roi_heads.box_head.0.fc1.weight"] = sd["roi_heads.box_head.0.fc1.weight"] * 0.02
    sd["proposal_generator.centernet_head.agn_hm.bias"] = torch.full((1,), -2.0)
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and not missing, (missing, unexpected)
    if train:
        m.train()
        for lvl in (3, 4, 5):
            getattr(m, f"vip_p{lvl}").reweighting.drop.p = 0.0
    else:
        m.eval()
    return m, cfg


def _support_dict(ids):
    d = {k: {} for k in ("p3", "p4", "p5", "rcnn_8", "rcnn_4")}
    for j, c in enumerate(ids):
        p = R.synth_support(10 + j)
        for k in ("p3", "p4", "p5"):
            d[k][c] = p[k]
        d["rcnn_8"][c] = torch.randn(6, 128, 8, 8, generator=torch.Generator().manual_seed(40 + j)) * 0.1
        d["rcnn_4"][c] = torch.zeros(6, 128, 4, 4)
    return d


def test_detector_inference(oh):
    m, _ = _detector()
    m.set_support_dict(_support_dict([7]))
    req = {"image": R.synth_image(9, 96, 128), "height": 96, "width": 128}
    a = m([req])[0]["instances"]
    b = m.inference_many([req])[0]["instances"]
    assert len(a) > 0
    assert torch.equal(a.pred_boxes.tensor, b.pred_boxes.tensor) and torch.equal(a.scores, b.scores) and torch.equal(a.pred_classes, b.pred_classes)
    assert m._engine.depthwise
    m.set_support_dict(_support_dict([3, 5]))
    m.support_classes = "all"
    c = m([req])[0]["instances"]
    assert len(c) > 0 and set(c.pred_classes.tolist()) <= {3, 5}


def _train_items(B=1, shots=4, support_hw=96):
    """One 96x128 query with three ground-truth boxes of side 20..50 and `shots` support crops with a box of side 40..80 each."""
    from detectron2.structures import Boxes, Instances
    items = []
    for b in range(B):
        g = torch.Generator().manual_seed(500 + b)
        wh = torch.rand(3, 2, generator=g) * 30 + 20
        ctr = torch.rand(3, 2, generator=g) * (torch.tensor([128.0, 96.0]) - wh) + wh / 2
        gt = torch.cat([ctr - wh / 2, ctr + wh / 2], 1)
        sup = torch.stack([R.synth_image(20 + b + i, support_hw, support_hw).float() for i in range(shots)], 0)
        side = torch.rand(shots, 2, generator=g) * 40 + 40
        c = torch.rand(shots, 2, generator=g) * (support_hw - side) + side / 2
        sbox = torch.cat([c - side / 2, c + side / 2], 1)
        inst = Instances((96, 128))
        inst.gt_boxes, inst.gt_classes = Boxes(gt.cuda()), torch.zeros(len(gt), dtype=torch.int64).cuda()
        items.append({"image": R.synth_image(2 + b, 96, 128).cuda(), "instances": inst, "support_images": sup.cuda(), "support_bboxes": sbox.cuda()})
    return items


def test_one_training_iteration(oh):
    m, _ = _detector(train=True)
    losses = m(_train_items())
    assert all(bool(torch.isfinite(v)) for v in losses.values()), losses
    sum(losses.values()).backward()
    n_dw = 0
    for n, p in m.backbone.bottom_up.named_parameters():
        if n.startswith(("stage4.", "stage5.")) and n.endswith(("dw_conv3x3.weight", "pw_conv1x1.weight", "/conv.weight")):
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, n
            n_dw += n.endswith("dw_conv3x3.weight")
        elif n.startswith(("stem.", "stage2.", "stage3.")):
            assert p.grad is None, n
    assert n_dw == 6


def test_graphed_train_steps_equal_eager(oh, monkeypatch):
    """Two captured-and-replayed GraphedTrainStep steps (behind the two eager ones it warms up with: the packed-weight job table of the
    step is built by the second eager step) leave the parameters torch.equal to the same four steps run eagerly from the same start; a
    capture that fell back fails here with its reason."""
    from fewx.solver import GraphedTrainStep, build_optimizer
    items = _train_items()
    keys = torch.rand(1, 16384, generator=torch.Generator().manual_seed(3)).cuda()
    real_rand = torch.rand

    def fixed_rand(*shape, **kw):                           # the fg / bg subsample draws its keys here: the same for both runs
        if len(shape) == 2 and kw.get("device") is not None and torch.device(kw["device"]).type == "cuda":
            return keys[:shape[0], :shape[1]].clone()
        return real_rand(*shape, **kw)

    monkeypatch.setattr(torch, "rand", fixed_rand)
    res = {}
    for mode in ("eager", "graph"):
        m, cfg = _detector(train=True)
        opt = build_optimizer(cfg, m)
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
            assert stepper.eager_steps == 2 and stepper.replays == 2, (stepper.eager_steps, stepper.replays)
        res[mode] = opt.bucket.params.detach().clone()
    assert bool(torch.isfinite(res["eager"]).all())
    assert torch.equal(res["eager"], res["graph"]), float((res["eager"] - res["graph"]).abs().max())
