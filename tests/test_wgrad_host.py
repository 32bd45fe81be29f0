"""CPU: the weight-gradient plan restatement reaches every launch form, and the element-wise bound of tests/wgrad_ref.py has teeth.

tests/test_hip_wgrad.py holds ore_conv2d_wgrad_bias_fwd to a float64 reference with an element-wise bound derived from the launch
plan.  Here, without a GPU: the shape matrix of that module lands in every (kernel, reduce) cell; the capped-workspace cases give the
intended split; a correct fp32 emulation of the split summation passes the bound; and the bound fails on the errors it is there to
catch (a dropped slab, an ignored beta, a 1e-3 error in one tile of a small channel, a bias summed from bf16-rounded dZ)."""
import itertools

import pytest
import torch

import wgrad_ref as WR


def _M(s):
    return s[0] * s[1] * s[2]


@pytest.mark.parametrize("bf16", [False, True])
def test_matrix_reaches_every_kernel_and_reduce_form(bf16):
    cells = {}
    for s in WR.MATRIX:
        B, H, W, Cin, Cout, k = s
        S, chunk, G = WR.wgrad_plan(_M(s), Cin, Cout, k, bf16)
        assert chunk % (32 if bf16 else 16) == 0 and (S - 1) * chunk < _M(s) <= S * chunk
        cells.setdefault((WR.wgrad_kernel(k, bf16), G), []).append(s)
    kernels = WR.KERNELS[2:] if bf16 else WR.KERNELS[:2]
    want = set(itertools.product(kernels, WR.REDUCES))
    assert set(cells) == want, sorted(want - set(cells))


@pytest.mark.parametrize("bf16", [False, True])
def test_semantics_subset_covers_every_reduce_form(bf16):
    cells = {(WR.wgrad_kernel(s[5], bf16), WR.wgrad_plan(_M(s), s[3], s[4], s[5], bf16)[2]) for s in WR.SEMANTICS_SHAPES}
    kernels = WR.KERNELS[2:] if bf16 else WR.KERNELS[:2]
    assert cells == set(itertools.product(kernels, WR.REDUCES))


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("k", [1, 3])
def test_capped_workspace_gives_the_intended_split(k, bf16):
    B, H, W, Cin, Cout = WR.CAP_SHAPE
    per = WR.slab_floats(Cin, Cout, k)
    assert WR.wgrad_plan(B * H * W, Cin, Cout, k, bf16)[0] > max(WR.CAPS)         # the cap, not the default split, decides
    for cap in WR.CAPS:
        S, chunk, G = WR.wgrad_plan(B * H * W, Cin, Cout, k, bf16, workspace_floats=cap * per + per // 2)
        assert S == cap, (cap, S, chunk)
        assert G == (0 if cap == 1 else 4 if cap >= 16 else 1)
    with pytest.raises(ValueError):
        WR.wgrad_plan(B * H * W, Cin, Cout, k, bf16, workspace_floats=per - 1)


def test_plan_hand_checked_cases():
    # 2x64x64 112->112 3x3: 2 x 2 x 3 = 12 blocks per split -> 128 splits aimed at, ceil(8192 / 128) = 64 rows allow 64
    assert WR.wgrad_plan(8192, 112, 112, 3, False) == (64, 128, 16)
    # a stride-4 1x1 at 640x640: 2 blocks per split, 200 splits of 128 rows
    assert WR.wgrad_plan(25600, 64, 128, 1, True) == (200, 128, 16)
    # S >= 64 but more than 65536 quads to sum (128 x 256 x 9 / 4 = 73728): <4>
    assert WR.wgrad_plan(8192, 256, 128, 3, False) == (64, 128, 4) and WR.wgrad_tiles(256, 128, 3) == 24
    # 32-row granule of the bf16 kernel: 400 rows in 4 splits of 100 -> 112 (fp32) / 128 (bf16) rows
    assert WR.wgrad_plan(400, 128, 16, 3, False) == (4, 112, 1) and WR.wgrad_plan(400, 128, 16, 3, True) == (4, 128, 1)
    assert WR.wgrad_plan(96, 1024, 128, 1, False) == (1, 96, 0)


# ---- teeth ---------------------------------------------------------------------------------------------------------------------
SHAPE = (2, 12, 12, 32, 32, 3)     # 288 rows, 3 splits of 96 rows (k_wgrad3 + k_wgrad_reduce<1>)


def _emulate(x, dz, k, plan, drop=None, bias_dz=None):
    """An fp32 implementation of the split: per split one fp32 GEMM per tap (its own summation order), the slabs added in fp32 in
    ascending order -- what the launch computes, up to the order of the additions.  `drop`: a split whose slab is left out."""
    S, chunk, _ = plan
    B, H, W, Cin = x.shape
    Cout = dz.shape[-1]
    M, p = B * H * W, k // 2
    xp = torch.nn.functional.pad(x, (0, 0, p, p, p, p))
    z = dz.reshape(M, Cout)
    zb = (bias_dz if bias_dz is not None else dz).reshape(M, Cout)
    dw = torch.zeros(Cout, Cin, k, k)
    db = torch.zeros(Cout)
    for s in range(S):
        if s == drop:
            continue
        r = slice(s * chunk, min(M, (s + 1) * chunk))
        part = torch.empty(Cout, Cin, k, k)
        for ky in range(k):
            for kx in range(k):
                part[:, :, ky, kx] = z[r].t() @ xp[:, ky:ky + H, kx:kx + W, :].reshape(M, Cin)[r]
        dw += part
        db += zb[r].sum(0)
    return dw, db


@pytest.fixture(scope="module")
def teeth():
    B, H, W, Cin, Cout, k = SHAPE
    x, dz = WR.scaled_operands(B, H, W, Cin, Cout, seed=11)
    plan = WR.wgrad_plan(B * H * W, Cin, Cout, k, False)
    assert plan == (3, 96, 1)
    return x, dz, k, plan, WR.wgrad_ref(x, dz, k)


def test_fp32_emulation_passes_the_bound(teeth):
    x, dz, k, plan, ref = teeth
    dw, db = _emulate(x, dz, k, plan)
    r = WR.wgrad_check(ref, plan, dw, db)
    assert r["dw"] <= 1 and r["db"] <= 1, r
    # the reference itself, rounded once to fp32
    r = WR.wgrad_check(ref, plan, ref["dw"].float(), ref["db"].float())
    assert r["dw"] <= 1e-2 and r["db"] <= 1e-2, r


@pytest.mark.parametrize("drop", [0, 2])
def test_bound_fails_on_a_dropped_slab(teeth, drop):
    x, dz, k, plan, ref = teeth
    dw, db = _emulate(x, dz, k, plan, drop=drop)
    r = WR.wgrad_check(ref, plan, dw, db)
    assert r["dw"] > 1 and r["db"] > 1, r


def test_bound_fails_when_beta_is_ignored(teeth):
    x, dz, k, plan, ref = teeth
    dw, db = _emulate(x, dz, k, plan)
    g = torch.Generator().manual_seed(3)
    old_w, old_b = torch.randn(dw.shape, generator=g), torch.randn(db.shape, generator=g)
    ok = WR.wgrad_check(ref, plan, dw + old_w, db + old_b, old_w=old_w, beta=1.0, old_b=old_b, beta_b=1.0)
    assert ok["dw"] <= 1 and ok["db"] <= 1, ok
    r = WR.wgrad_check(ref, plan, dw, db, old_w=old_w, beta=1.0, old_b=old_b, beta_b=1.0)
    assert r["dw"] > 1 and r["db"] > 1, r


def test_bound_fails_on_one_perturbed_tile_of_a_small_channel(teeth):
    """One 16-wide MFMA tile (16 output channels) of the input channel with the smallest scale, 1e-3 relative off: the element-wise
    bound sees it, the max-norm measure of the end-to-end tests does not."""
    x, dz, k, plan, ref = teeth
    dw, db = _emulate(x, dz, k, plan)
    ci = int(x.abs().amax((0, 1, 2)).argmin())
    bad = dw.clone()
    bad[16:32, ci] *= 1.0 + 1e-3
    assert WR.wgrad_check(ref, plan, bad, db)["dw"] > 1
    assert float((bad.double() - ref["dw"]).abs().max() / ref["dw"].abs().max()) < 1e-6


def test_bound_fails_on_a_bias_from_rounded_dz(teeth):
    """In bf16 mode the MFMA operands are rounded, the bias gradient is not: a bias summed from the bf16-rounded dZ fails."""
    x, dz, k, _, _ = teeth
    B, H, W, Cin, Cout, _ = SHAPE
    plan = WR.wgrad_plan(B * H * W, Cin, Cout, k, True)
    ref = WR.wgrad_ref(x, dz, k, bf16=True)
    dw, db = _emulate(WR.bf16_rne(x), WR.bf16_rne(dz), k, plan, bias_dz=dz)
    ok = WR.wgrad_check(ref, plan, dw, db)
    assert ok["dw"] <= 1 and ok["db"] <= 1, ok
    _, db_bad = _emulate(WR.bf16_rne(x), WR.bf16_rne(dz), k, plan)
    assert WR.wgrad_check(ref, plan, dw, db_bad)["db"] > 1
    # and the bf16 result is outside the bound of the fp32-operand reference: the mode is visible to the check
    assert WR.wgrad_check(WR.wgrad_ref(x, dz, k), plan, dw)["dw"] > 1


def test_bf16_rne_rounds_to_nearest_even():
    v = torch.tensor([1.0, 1.0 + 2 ** -8, 1.0 + 3 * 2 ** -8, 1.0 + 2 ** -8 + 2 ** -20, -1.0 - 2 ** -8, 3.0e-3, -7.5e2])
    assert torch.equal(WR.bf16_rne(v), v.to(torch.bfloat16).float())
    assert WR.bf16_rne(v)[1] == 1.0 and WR.bf16_rne(v)[2] == 1.0 + 2 ** -6


def test_reference_is_the_conv_weight_gradient():
    """The shifted-window GEMMs are conv2d's weight gradient (float64 autograd, zero padding, per image)."""
    g = torch.Generator().manual_seed(2)
    x, dz = torch.randn(3, 5, 7, 8, generator=g), torch.randn(3, 5, 7, 12, generator=g)
    ref = WR.wgrad_ref(x, dz, 3)
    w = torch.zeros(12, 8, 3, 3, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(12, dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.conv2d(x.double().permute(0, 3, 1, 2), w, b, padding=1)
    (y * dz.double().permute(0, 3, 1, 2)).sum().backward()
    assert torch.allclose(ref["dw"], w.grad, rtol=1e-12, atol=1e-12) and torch.allclose(ref["db"], b.grad, rtol=1e-12, atol=1e-12)
