"""Every launch form of the conv weight gradient (ore_conv2d_wgrad_bias_fwd, csrc/ore_conv_wgrad.hip) against a float64 reference.

One entry point computes every conv weight gradient of the training step.  Depending on the kernel size and the precision mode it
runs k_wgrad, k_wgrad3, k_wgrad_bf<false> or k_wgrad_bf<true>.  Depending on the row split S it writes dW / db itself (S == 1) or
sums S slabs with k_wgrad_reduce<1 | 4 | 16>.  tests/wgrad_ref.py restates that plan (tests/test_wgrad_host.py checks the shape matrix
reaches every cell), computes dW and db in float64 as shifted-window GEMMs, and derives an element-wise bound
|got - ref| <= c u (|dz|^T |x| + |beta old|) with c from the plan (its docstring gives the derivation).  The operands carry
per-channel scales from 1e-3 to 1e3, so an error in a small channel fails the bound even where a max-norm measure would pass.

Covered here: the shape matrix in both modes; workspaces capped to force S = 1, 2, 3, 17 through the C ABI; channel slices and views
with NaN around them, beta = 1 into existing values and beta = 0 into NaN, db on / off, run-to-run determinism; and a replay of every
distinct call one eager 640x640 training step makes, in both modes.

ORE_WGRAD_LOG=<file>: append the largest bound ratio per (mode, kernel, reduce) form to that file (the figure of headroom in c)."""
import ctypes as C
import os

import pytest
import torch

import wgrad_ref as WR

pytestmark = pytest.mark.gpu

NAN = float("nan")
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
    lines = [f"{m:5s} {kern:18s} reduce {G:2d}  max |got-ref|/bound {r:.3e}  ({n} checks)" for (m, kern, G), (r, n) in sorted(_RATIOS.items())]
    print("\n" + "\n".join(lines))
    log = os.environ.get("ORE_WGRAD_LOG")
    if log and lines:
        with open(log, "a") as f:
            f.write("\n".join(lines) + "\n")


@pytest.fixture(params=["fp32", "bf16"])
def mode(oh, request):
    prev = oh.set_conv_precision(request.param)
    yield request.param
    oh.set_conv_precision(prev)


def _ref_device(M, Cin, Cout, k):
    return "cuda" if M * Cin * Cout * k * k > 2e7 else "cpu"


def _assert_within(ratios, plan, k, bf16, what):
    key = ("bf16" if bf16 else "fp32", WR.wgrad_kernel(k, bf16), plan[2])
    r0, n0 = _RATIOS.get(key, (0.0, 0))
    _RATIOS[key] = (max([r0] + list(ratios.values())), n0 + 1)
    assert all(v <= 1.0 for v in ratios.values()), (what, plan, ratios)


def _embed(t, ld, coff, head=0, tail=0):
    """t [B,H,W,C] as channels coff .. coff + C of a [B,H,W,ld] view that starts `head` rows into a NaN-filled allocation and
    has `tail` NaN rows behind it."""
    B, H, W, Cc = t.shape
    M = B * H * W
    big = torch.full(((head + M + tail) * ld,), NAN, device="cuda")
    v = big[head * ld:(head + M) * ld].view(B, H, W, ld)
    v[..., coff:coff + Cc] = t.cuda()
    return v


# ---- the plan restatement against the library ---------------------------------------------------------------------------------
def test_workspace_size_matches_the_plan(oh):
    """ore_conv_wgrad_workspace_floats sizes the default workspace for the split wgrad_plan starts from."""
    L = oh.lib()
    for (B, H, W, Cin, Cout, k) in WR.MATRIX + [WR.CAP_SHAPE + (1,), WR.CAP_SHAPE + (3,)]:
        M = B * H * W
        ws = L.ore_conv_wgrad_workspace_floats(M, Cin, Cout, k, k)
        assert ws == WR.slab_floats(Cin, Cout, k) * WR.wgrad_split(M, Cin, Cout, k), (B, H, W, Cin, Cout, k, ws)


# ---- the shape matrix ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,Cin,Cout,k", WR.MATRIX)
def test_wgrad_matrix(oh, mode, B, H, W, Cin, Cout, k):
    bf16 = mode == "bf16"
    M = B * H * W
    plan = WR.wgrad_plan(M, Cin, Cout, k, bf16)
    x, dz = WR.scaled_operands(B, H, W, Cin, Cout, seed=M + 7 * Cin + Cout + k)
    gw, gb = oh.conv2d_wgrad(x.cuda(), dz.cuda(), k, want_bias=True)
    ref = WR.wgrad_ref(x, dz, k, bf16=bf16, device=_ref_device(M, Cin, Cout, k))
    _assert_within(WR.wgrad_check(ref, plan, gw, gb), plan, k, bf16, "matrix")
    if H * W == 1 and k == 3:                       # single pixels: every off-centre tap reads outside its image -> exactly 0
        assert float(gw[:, :, [0, 0, 0, 1, 1, 2, 2, 2], [0, 1, 2, 0, 2, 0, 1, 2]].abs().max()) == 0.0


def test_bf16_mode_is_visible_to_the_bound(oh):
    """The bf16-mode result is within the bound of the bf16-operand reference and outside that of the fp32-operand one."""
    B, H, W, Cin, Cout, k = 2, 40, 44, 96, 96, 3
    prev = oh.set_conv_precision("bf16")
    try:
        x, dz = WR.scaled_operands(B, H, W, Cin, Cout, seed=5)
        gw = oh.conv2d_wgrad(x.cuda(), dz.cuda(), k)
    finally:
        oh.set_conv_precision(prev)
    plan = WR.wgrad_plan(B * H * W, Cin, Cout, k, True)
    assert WR.wgrad_check(WR.wgrad_ref(x, dz, k, bf16=True), plan, gw)["dw"] <= 1.0
    assert WR.wgrad_check(WR.wgrad_ref(x, dz, k), plan, gw)["dw"] > 10.0


# ---- capped workspace through the C ABI ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", WR.CAPS)
@pytest.mark.parametrize("k", [1, 3])
def test_wgrad_capped_workspace(oh, mode, k, cap):
    """A workspace of `cap` slabs (+ half a slab) makes the launch split its rows `cap` ways: S == 1 writes dW / db directly, 2 and 3
    reduce with <1>, 17 with <4> (tests/test_wgrad_host.py checks the plan)."""
    bf16 = mode == "bf16"
    B, H, W, Cin, Cout = WR.CAP_SHAPE
    M, per = B * H * W, WR.slab_floats(Cin, Cout, k)
    n = cap * per + per // 2
    plan = WR.wgrad_plan(M, Cin, Cout, k, bf16, workspace_floats=n)
    assert plan[0] == cap
    x, dz = WR.scaled_operands(B, H, W, Cin, Cout, seed=100 + cap + k, device="cuda")
    ws = torch.empty(n, device="cuda")
    dw = torch.empty(Cout, Cin, k, k, device="cuda")
    db = torch.empty(Cout, device="cuda")
    P = C.c_void_p
    rc = oh.lib().ore_conv2d_wgrad_bias_fwd(P(x.data_ptr()), Cin, 0, P(dz.data_ptr()), Cout, 0, B, H, W, Cin, Cout, k, k, k // 2,
                                            P(dw.data_ptr()), C.c_float(0.0), P(db.data_ptr()), C.c_float(0.0), P(ws.data_ptr()),
                                            C.c_size_t(n), oh._stream())
    assert rc == 0, oh.lib().ore_last_error().decode()
    ref = WR.wgrad_ref(x, dz, k, bf16=bf16)
    _assert_within(WR.wgrad_check(ref, plan, dw, db), plan, k, bf16, f"cap {cap}")


def test_wgrad_workspace_below_one_slab_is_refused(oh):
    B, H, W, Cin, Cout = WR.CAP_SHAPE
    per = WR.slab_floats(Cin, Cout, 3)
    x = torch.zeros(B, H, W, Cin, device="cuda")
    dw = torch.zeros(Cout, Cin, 3, 3, device="cuda")
    ws = torch.zeros(per, device="cuda")
    P = C.c_void_p
    rc = oh.lib().ore_conv2d_wgrad_bias_fwd(P(x.data_ptr()), Cin, 0, P(x.data_ptr()), Cout, 0, B, H, W, Cin, Cout, 3, 3, 1,
                                            P(dw.data_ptr()), C.c_float(0.0), None, C.c_float(0.0), P(ws.data_ptr()),
                                            C.c_size_t(per - 1), oh._stream())
    assert rc != 0 and "workspace too small" in oh.lib().ore_last_error().decode()
    assert float(dw.abs().max()) == 0.0


# ---- argument semantics -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,Cin,Cout,k", WR.SEMANTICS_SHAPES)
def test_wgrad_argument_semantics(oh, mode, B, H, W, Cin, Cout, k):
    """x / dz as channel slices (x_coff / dz_coff, wider ld) of views into larger allocations; every channel outside the slice and
    every row before and behind the view holds NaN, which a read outside the block's rows or channels would carry into the result.
    beta = 1 / beta_b = 1 add into existing values; beta = 0 into outputs pre-filled with NaN must not compute 0 * NaN.  The weight
    part is bitwise the same with and without the bias gradient, and two identical calls are bitwise equal."""
    bf16 = mode == "bf16"
    M = B * H * W
    plan = WR.wgrad_plan(M, Cin, Cout, k, bf16)
    x, dz = WR.scaled_operands(B, H, W, Cin, Cout, seed=3 * M + Cin + k, device="cuda")
    xc, zc = 20, 4
    xv = _embed(x, Cin + 28, xc, head=37, tail=3 * W + 70)
    zv = _embed(dz, Cout + 12, zc, head=5, tail=2 * W + 40)
    ref = WR.wgrad_ref(x, dz, k, bf16=bf16)
    kw = dict(x_coff=xc, Cin=Cin, dz_coff=zc, Cout=Cout)
    g = torch.Generator(device="cuda").manual_seed(M)
    old_w = torch.randn(Cout, Cin, k, k, generator=g, device="cuda") * ref["aw"].float().mean()
    old_b = torch.randn(Cout, generator=g, device="cuda") * ref["ab"].float().mean()
    dw, db = old_w.clone(), old_b.clone()
    oh.conv2d_wgrad(xv, zv, k, out=dw, beta=1.0, want_bias=True, db_out=db, beta_b=1.0, **kw)
    r = WR.wgrad_check(ref, plan, dw, db, old_w=old_w, beta=1.0, old_b=old_b, beta_b=1.0)
    _assert_within(r, plan, k, bf16, "beta = 1 into existing values")
    dw0 = torch.full_like(old_w, NAN)
    db0 = torch.full_like(old_b, NAN)
    oh.conv2d_wgrad(xv, zv, k, out=dw0, beta=0.0, want_bias=True, db_out=db0, beta_b=0.0, **kw)
    _assert_within(WR.wgrad_check(ref, plan, dw0, db0), plan, k, bf16, "beta = 0 into NaN")
    gw_nob = oh.conv2d_wgrad(xv, zv, k, **kw)
    assert torch.equal(gw_nob, dw0), "the bias gradient changed the weight gradient"
    gw2, gb2 = oh.conv2d_wgrad(xv, zv, k, want_bias=True, **kw)
    assert torch.equal(gw2, dw0) and torch.equal(gb2, db0), "two identical launches differ"


# ---- production replay --------------------------------------------------------------------------------------------------------
def _train_step_calls(oh, mode):
    """Every argument signature orehip.conv2d_wgrad receives during one eager training step on the `full` reference-run sample
    (640x640 query, 24 support crops of 240x240), with the flat gradient bucket in place so that direct_grad accumulates into
    parameter gradients (beta = 1) as in production."""
    from conftest import GOLDEN, PKG
    import numpy as np
    from detectron2.modeling import build_model
    from detectron2.structures import Boxes, Instances
    from fewx.config import get_cfg
    from fewx.modeling.fsod.train_forward import train_forward
    from fewx.solver.build import get_bucket
    from oracle import ref_model as R
    from oracle import ref_train as T
    g = dict(np.load(os.path.join(GOLDEN, "train_iter_ref_full.npz")))
    shots, hw = int(g["shots"]), tuple(int(v) for v in g["hw"])
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(PKG, "configs", "fsod", "finetune_vovnet.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", "cuda", "INPUT.FS.SUPPORT_SHOT", shots])
    cfg.freeze()
    torch.manual_seed(0)
    m = build_model(cfg)
    sd = R.synth_roi_state(R.synth_state_dict(0), 0)
    m.load_state_dict(sd, strict=False)
    m.train()
    get_bucket(m, cfg)
    img, gt, sup, sbox = T.synth_train_inputs(int(g["input_seed"]), hw, n_gt=int(g["n_gt"]), shots=shots, support_hw=int(g["support_hw"]))
    inst = Instances(hw)
    inst.gt_boxes, inst.gt_classes = Boxes(gt), torch.zeros(len(gt), dtype=torch.int64)
    item = {"image": img, "instances": inst, "support_images": sup, "support_bboxes": sbox.numpy()}
    over = {"boxes": torch.from_numpy(g["roi_boxes"]), "labels": torch.from_numpy(g["roi_labels"]), "gt": torch.from_numpy(g["roi_gt"])}
    calls = {}
    real = oh.conv2d_wgrad

    def spy(x, dz, k, **kw):
        B, H, W, xld = x.shape
        x_coff, dz_coff = kw.get("x_coff", 0), kw.get("dz_coff", 0)
        out, db_out, want_bias = kw.get("out"), kw.get("db_out"), kw.get("want_bias", False)
        sig = (B, H, W, xld, x_coff, kw.get("Cin") or xld - x_coff, dz.shape[-1], dz_coff, kw.get("Cout") or dz.shape[-1] - dz_coff, k,
               out is not None, float(kw.get("beta", 0.0)) if out is not None else 0.0, bool(want_bias),
               want_bias and db_out is not None, float(kw.get("beta_b", 0.0)) if want_bias and db_out is not None else 0.0)
        assert x.is_contiguous() and dz.is_contiguous()
        calls[sig] = calls.get(sig, 0) + 1
        return real(x, dz, k, **kw)

    oh.conv2d_wgrad = spy
    try:
        losses = train_forward(m, [item], roi_override=over)
        sum(losses.values()).backward()
        torch.cuda.synchronize()
    finally:
        oh.conv2d_wgrad = real
    return calls


def test_wgrad_production_replay(oh, mode):
    """Each distinct call of one eager 640x640 training step, replayed on fresh random data in the same layout (channel slices of
    the same ld with NaN in the other channels, the same beta / bias flags, existing random values under beta = 1)."""
    bf16 = mode == "bf16"
    calls = _train_step_calls(oh, mode)
    assert len(calls) >= 10, calls
    assert any(s[10] and s[11] == 1.0 for s in calls), "no in-place (direct_grad) call recorded"
    assert any(s[4] != 0 for s in calls), "no channel-slice call recorded"
    forms = set()
    for i, sig in enumerate(sorted(calls)):
        B, H, W, xld, xc, Cin, zld, zc, Cout, k, has_out, beta, want_bias, has_db, beta_b = sig
        M = B * H * W
        plan = WR.wgrad_plan(M, Cin, Cout, k, bf16, bias=want_bias)
        forms.add((WR.wgrad_kernel(k, bf16), plan[2]))
        x, dz = WR.scaled_operands(B, H, W, Cin, Cout, seed=1000 + i, device="cuda")
        xv, zv = _embed(x, xld, xc), _embed(dz, zld, zc)
        ref = WR.wgrad_ref(x, dz, k, bf16=bf16)
        g = torch.Generator(device="cuda").manual_seed(i)
        kw = dict(x_coff=xc, Cin=Cin, dz_coff=zc, Cout=Cout, want_bias=want_bias)
        old_w = old_b = None
        if has_out:
            old_w = torch.randn(Cout, Cin, k, k, generator=g, device="cuda") * ref["aw"].float().mean()
            kw.update(out=old_w.clone(), beta=beta)
        if has_db:
            old_b = torch.randn(Cout, generator=g, device="cuda") * ref["ab"].float().mean()
            kw.update(db_out=old_b.clone(), beta_b=beta_b)
        res = oh.conv2d_wgrad(xv, zv, k, **kw)
        dw, db = res if want_bias else (res, None)
        r = WR.wgrad_check(ref, plan, dw, db, old_w=old_w, beta=beta, old_b=old_b, beta_b=beta_b)
        _assert_within(r, plan, k, bf16, f"replay {sig}")
    print(f"\n{mode}: {len(calls)} distinct wgrad calls ({sum(calls.values())} launches), forms {sorted(forms)}")
