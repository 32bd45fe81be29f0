"""CPU: the float64 restatements of tests/trainops_ref.py are the ops they name, and the two bounds have teeth.

tests/trainops_ref.py restates every non-conv kernel of a training step in float64, to be held to the element-wise bound
2 d u mag and the 16 x 16 block rms bound C_S u sqrt(d) (it derives every d).  Here, without a GPU:
  * each restatement equals float64 torch.autograd of the obvious torch expression to 1e-12 relative (F.group_norm,
    F.max_pool2d(ceil_mode=True), F.adaptive_avg_pool2d, the depthwise convs of oracle.ref_model.correlation, the eSE formula);
  * an fp32 emulation of each reduction in the kernel's documented order (256-row chunks of 4 lanes x 2 accumulators; 16 lanes x 4
    accumulators x S slabs; Chan's combine over 64-row chunks; the elementwise formulas evaluated in fp32) passes both bounds at every
    production row count -- the assertion message carries the worst ratio;
  * each fault the bounds are there to catch fails at least one of them, and where the point of the fault is that it is LOCAL (one
    small channel, one small image) the old max-norm criterion of tests/test_hip_train.py passes it;
  * every orehip function orehip/autograd.py calls is either covered (TRAIN_OPS) or listed with its reason (NOT_COVERED)."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import trainops_ref as TR
from conftest import PKG

F64 = torch.float64
RTOL = 1e-12


def _same(a, b):
    a, b = a.double(), b.double()
    assert a.shape == b.shape, (a.shape, b.shape)
    assert float((a - b).abs().max()) <= RTOL * max(1.0, float(b.abs().max())), float((a - b).abs().max())


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _rand(*shape, seed=0, grad=False):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, dtype=F64, generator=g).requires_grad_(grad)


def _passes(got, ref, mag, d):
    h, r = TR.check2(got, ref, mag, d)
    return h <= 1 and r <= 1, (h, r)


# ---- the restatements are the ops ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,C,G,relu", [(2, 3, 5, 8, 2, True), (3, 1, 1, 8, 2, False), (1, 1, 7, 4, 4, True), (2, 9, 1, 16, 1, True),
                                            (2, 4, 4, 32, 8, False)])
def test_groupnorm_reference_is_group_norm(B, H, W, C, G, relu):
    x = _rand(B, H, W, C, seed=C + G, grad=True)
    x.data += 5.0
    gamma, beta = _rand(C, seed=1, grad=True), _rand(C, seed=2, grad=True)
    y = F.group_norm(_nchw(x), G, gamma, beta, eps=1e-5)
    y = F.relu(y) if relu else y
    dy = _rand(*y.shape, seed=3)
    (y * dy).sum().backward()
    xr = x.detach().reshape(B, H * W, C)
    (r, rm), (a, am) = TR.gn_stats(xr, G, 1e-5)
    assert bool((rm >= r.abs()).all()) and bool((am >= a.abs() - 1e-12).all())
    yy, ym = TR.gn_apply(xr, r, a, gamma.detach(), beta.detach(), relu)
    _same(yy.reshape(B, H, W, C), y.detach().permute(0, 2, 3, 1))
    out = TR.gn_bwd(dy.permute(0, 2, 3, 1).reshape(B, H * W, C), yy, xr, r, a, gamma.detach(), G, relu)
    _same(out["dx"][0].reshape(B, H, W, C), x.grad)
    _same(out["dbeta"][0].sum(0), beta.grad)
    _same(out["dgamma"][0].sum(0), gamma.grad)
    for k in out:
        assert bool((out[k][1] >= out[k][0].abs() * (1 - 1e-12)).all()), k


@pytest.mark.parametrize("quantised", [True, False])
@pytest.mark.parametrize("B,H,W", [(2, 5, 7), (1, 4, 6), (3, 3, 3), (2, 2, 2), (2, 9, 4), (1, 40, 3), (2, 6, 2)])
def test_maxpool_reference_is_max_pool2d(B, H, W, quantised):
    x = _rand(B, H, W, 4, seed=H * W)
    if quantised:
        x = (x * 1.5).round()                                # few distinct values: most windows hold ties
    x.requires_grad_(True)
    y = F.max_pool2d(_nchw(x), 3, 2, ceil_mode=True)
    assert tuple(y.shape[2:]) == TR.maxpool_out_hw(H, W)
    dy = _rand(*y.shape, seed=1)
    (y * dy).sum().backward()
    assert torch.equal(TR.maxpool_fwd(x.detach()), y.detach().permute(0, 2, 3, 1))
    dx, mag = TR.maxpool_bwd(x.detach(), dy.permute(0, 2, 3, 1))
    _same(dx, x.grad)
    assert bool((mag >= dx.abs()).all())
    if quantised:
        assert not torch.equal(TR.maxpool_owner(x.detach()), TR.maxpool_owner(x.detach(), last=True)), "no ties in the quantised input"


def test_maxpool_reference_below_three():
    """H or W of 1 or 2 (F.max_pool2d refuses H = 1): one window that covers the whole axis."""
    x = _rand(2, 1, 1, 4)
    assert torch.equal(TR.maxpool_fwd(x), x)
    dy = _rand(2, 1, 1, 4, seed=1)
    assert torch.equal(TR.maxpool_bwd(x, dy)[0], dy)
    x = _rand(1, 1, 6, 4, seed=2)
    want = torch.stack([x[:, :, 0:3].amax(2), x[:, :, 2:5].amax(2), x[:, :, 4:6].amax(2)], 2)
    assert torch.equal(TR.maxpool_fwd(x), want)


@pytest.mark.parametrize("B,H,W,OH,OW", [(2, 30, 30, 32, 32), (2, 7, 11, 3, 5), (1, 5, 5, 9, 12), (2, 32, 32, 1, 3), (2, 16, 16, 3, 1),
                                         (1, 8, 8, 1, 1), (2, 1, 1, 3, 3), (1, 1, 9, 1, 4), (3, 15, 15, 16, 16)])
def test_apool_reference_is_adaptive_avg_pool2d(B, H, W, OH, OW):
    x = _rand(B, H, W, 4, seed=H + OW, grad=True)
    y = F.adaptive_avg_pool2d(_nchw(x), (OH, OW))
    dy = _rand(*y.shape, seed=1)
    (y * dy).sum().backward()
    yy, ym = TR.apool_fwd(x.detach(), OH, OW)
    _same(yy, y.detach().permute(0, 2, 3, 1))
    dx, dxm = TR.apool_bwd(dy.permute(0, 2, 3, 1), H, W)
    _same(dx, x.grad)
    assert bool((ym >= yy.abs() * (1 - 1e-12)).all()) and bool((dxm >= dx.abs() * (1 - 1e-12)).all())


def _corr_torch(q, k11, k13, k31):
    """The training branch of the correlation as oracle.ref_model.correlation writes it (depthwise F.conv2d), one image at a time
    with that image's kernels; NHWC in, [attn | q] out."""
    B, H, W, C = q.shape
    outs = []
    for b in range(B):
        x = _nchw(q[b:b + 1])
        w11 = (k11[b] if k11.dim() == 2 else k11).reshape(C, 1, 1, 1)
        w13 = (k13[b] if k13.dim() == 3 else k13).reshape(C, 1, 1, 3)
        w31 = (k31[b] if k31.dim() == 3 else k31).reshape(C, 1, 3, 1)
        a = F.relu(F.conv2d(x, w11, groups=C))
        a = F.relu(F.conv2d(a, w11, groups=C))
        t = F.relu(F.conv2d(x, w13, padding=(0, 1), groups=C))
        u = F.conv2d(t, w31, padding=(1, 0), groups=C)
        outs.append(torch.cat([a + F.relu(u) + x, x], 1).permute(0, 2, 3, 1))
    return torch.cat(outs, 0)


@pytest.mark.parametrize("per_image", [False, True])
@pytest.mark.parametrize("B,H,W", [(2, 5, 7), (3, 1, 6), (2, 6, 1), (2, 1, 1), (1, 4, 4)])
def test_correlation_reference_is_the_depthwise_convs(B, H, W, per_image):
    C = 8
    q = _rand(B, H, W, C, seed=H * 7 + W, grad=True)
    ks = (B,) if per_image else ()
    k11, k13, k31 = _rand(*ks, C, seed=1, grad=True), _rand(*ks, C, 3, seed=2, grad=True), _rand(*ks, C, 3, seed=3, grad=True)
    cat = _corr_torch(q, k11, k13, k31)
    dcat = _rand(*cat.shape, seed=4)
    (cat * dcat).sum().backward()
    f = TR.corr_fwd(q.detach(), k11.detach(), k13.detach(), k31.detach())
    _same(f["cat"][0], cat.detach())
    b = TR.corr_bwd(q.detach(), k11.detach(), k13.detach(), k31.detach(), dcat, f["t"][0], f["u"][0])
    _same(b["dq"][0], q.grad)
    S = B if per_image else 1
    _same(b["dk11"][0], k11.grad.reshape(S, C))
    _same(b["dk13"][0], k13.grad.reshape(S, C, 3))
    _same(b["dk31"][0], k31.grad.reshape(S, C, 3))
    for k in b:
        assert bool((b[k][1] >= b[k][0].abs() * (1 - 1e-12)).all()), k


@pytest.mark.parametrize("B,H,W,C", [(2, 3, 5, 8), (3, 1, 1, 4), (1, 7, 1, 12)])
def test_ese_reference_is_the_ese_formula(B, H, W, C):
    x, w, b = TR.ese_inputs(B, H, W, C, seed=C)
    assert TR.ese_knee_distance(x, w, b) >= TR.ESE_KNEE_MARGIN
    x, w, b = x.double().requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)
    z = F.linear(x.mean((1, 2)), w.reshape(C, C), b)
    y = x * (F.relu6(z + 3.0) / 6.0).view(B, 1, 1, C)             # Hsigmoid as d2z:modeling/backbone/vovnet.py writes it
    dy = _rand(*y.shape, seed=1)
    (y * dy).sum().backward()
    out = TR.ese_node(x.detach(), w.detach(), b.detach(), dy)
    _same(out["y"][0], y.detach())
    _same(out["dx"][0], x.grad)
    _same(out["dW"][0], w.grad.reshape(C, C))
    _same(out["db"][0], b.grad)
    for k in ("y", "dx", "dW", "db"):
        assert bool((out[k][1] >= out[k][0].abs() * (1 - 1e-12)).all()), k


def test_small_references():
    x = _rand(2, 5, 7, 4, grad=True)
    up = x.repeat_interleave(2, 1).repeat_interleave(2, 2)[:, :9, :13]      # nearest 2x, cropped: sumpool2x2 is its backward
    dy = _rand(2, 9, 13, 4, seed=1)
    (up * dy).sum().backward()
    _same(TR.sumpool2(dy)[0], x.grad)
    p, q = _rand(3, 4, 5, 8), _rand(3, 4, 5, 8, seed=1)
    _same(TR.prod_colsum(p, q, 0.25)[0], (p * q).sum((1, 2)) * 0.25)
    _same(TR.colsum(p.reshape(-1, 8), 3, 0.5, torch.ones(3, 8))[0], p.reshape(3, -1, 8).sum(1) + 0.5)
    _same(TR.group_mean(p.reshape(6, 10, 8), 2)[0], p.reshape(2, 3, 10, 8).mean(1))
    _same(TR.group_mean_bwd(p[:2], 2, 3)[0], (p[:2] / 3).repeat_interleave(3, 0))
    _same(TR.mean_pair(p, q)[0], (p + q).mean((1, 2)))
    a0, a1 = _rand(3, 8, seed=2), _rand(3, 8, seed=3)
    _same(TR.combine2(p, q, a0, a1)[0], p * a0.view(3, 1, 1, 8) + q * a1.view(3, 1, 1, 8))
    (dw, _), (dh, _) = TR.combine2_bwd(p, a0, a1, a0)
    _same(dw, p * a0.view(3, 1, 1, 8) + a0.view(3, 1, 1, 8))
    _same(dh, p * a1.view(3, 1, 1, 8) + a0.view(3, 1, 1, 8))
    for axis in ("h", "w"):
        t = _rand(2, 4, 6, 24)
        m = TR.sm_permute(t, 2, 4, 6, 3, 8, axis, False)
        assert m.shape == ((2, 3, 6, 4, 8) if axis == "h" else (2, 3, 4, 6, 8))
        assert torch.equal(TR.sm_permute(m, 2, 4, 6, 3, 8, axis, True).reshape(t.shape), t)


def test_input_properties():
    """The 30-sigma group offsets of gn_inputs and the knee margin of ese_inputs, against float64 alone."""
    x = TR.gn_inputs(3, 400, 128, 32, seed=5).double().reshape(3, 400, 32, 4)
    ratio = (x.mean((1, 3)).abs() / x.std((1, 3))).max()
    assert 20.0 <= float(ratio) <= 1.15 * TR.GN_OFFSET_SIGMAS, float(ratio)
    v = x.var((1, 3), unbiased=False)
    onepass = (x.float() ** 2).mean((1, 3)) - x.float().mean((1, 3)) ** 2              # E x^2 - mean^2 in fp32 loses its digits
    assert float(((onepass.double() - v).abs() / v).max()) > 1e-4
    for B, H, W, C in ((1, 40, 40, 384), (24, 8, 8, 512), (16, 5, 5, 64)):
        xe, w, b = TR.ese_inputs(B, H, W, C, seed=B)
        assert TR.ese_knee_distance(xe, w, b) >= TR.ESE_KNEE_MARGIN
        z = TR.ese_node(xe, w, b)["z"]
        assert bool((z > 3).any()) and bool((z < -3).any()) and bool((z.abs() < 3).any()), "all three hard-sigmoid branches"


# ---- fp32 emulations in the kernels' documented order ------------------------------------------------------------------------------
def _lanes_sum(v, lanes, accs):
    """v [n, ...] fp32: element k goes to lane k % lanes, accumulator (k // lanes) % accs of that lane; each accumulator is one chain
    in order; accumulators added in order, then the lanes pairwise ((l0 + l1) + (l2 + l3)) for 4 lanes or in one chain."""
    n = v.shape[0]
    step = lanes * accs
    pad = -n % step
    if pad:
        v = torch.cat([v, torch.zeros(pad, *v.shape[1:])])              # adding 0.0 is exact
    v = v.reshape(-1, accs, lanes, *v.shape[1:])
    acc = torch.zeros_like(v[0])
    for i in range(v.shape[0]):
        acc = acc + v[i]
    s = acc[0]
    for a in range(1, accs):
        s = s + acc[a]
    if lanes == 4:
        return (s[0] + s[1]) + (s[2] + s[3])
    out = torch.zeros_like(s[0])
    for lane in range(lanes):
        out = out + s[lane]
    return out


def emu_colsum(x, segments=1, beta=0.0, old=None, drop=None):
    """fp32 ore_colsum_segments_fwd: k_colsum_chunks then k_colsum_final.  drop = (segment, chunk): that chunk's sums are left out."""
    x = x.float().reshape(segments, -1, x.shape[-1])
    out = []
    for s in range(segments):
        parts = []
        for c, r0 in enumerate(range(0, x.shape[1], TR.CS_ROWS)):
            p = _lanes_sum(x[s, r0:r0 + TR.CS_ROWS], 4, 2)
            parts.append(torch.zeros_like(p) if drop == (s, c) else p)
        out.append(_lanes_sum(torch.stack(parts), 4, 2))
    out = torch.stack(out)
    return beta * old.float().reshape(out.shape) + out if beta != 0.0 else out


def emu_prod_colsum(p, q, scale, S, per, drop_slab=None):
    """fp32 ore_prod_colsum_fwd with S slabs of `per` rows: k_colsum_seg (row r0 + lane + 16 j of a lane; full groups of four rows to
    the accumulators a0..a3, the remaining rows to a0; (a0 + a1) + (a2 + a3); the 16 lanes in one chain), k_colsum_seg_fin."""
    B, C = p.shape[0], p.shape[-1]
    v = p.float().reshape(B, -1, C)
    if q is not None:
        v = v * q.float().reshape(B, -1, C)
    rows = v.shape[1]
    slabs = []
    for z in range(S):
        sl = v[:, z * per:min(rows, (z + 1) * per)]
        total = torch.zeros(B, C)
        for lane in range(16):
            mine = sl[:, lane::16]
            n = mine.shape[1]
            acc = [torch.zeros(B, C) for _ in range(4)]
            for j in range(n // 4 * 4):
                acc[j % 4] = acc[j % 4] + mine[:, j]
            for j in range(n // 4 * 4, n):
                acc[0] = acc[0] + mine[:, j]
            total = total + ((acc[0] + acc[1]) + (acc[2] + acc[3]))
        slabs.append(total)
    if S == 1:
        return slabs[0] * torch.tensor(scale, dtype=torch.float32)
    out = torch.zeros(B, C)
    for z in range(S):
        if z != drop_slab:
            out = out + slabs[z]
    return out * torch.tensor(scale, dtype=torch.float32)


def emu_gn_stats(x, G, eps, full_weight_tail=False):
    """fp32 ore_groupnorm_affine_fwd with unit affine: per 64-row chunk the group mean and M2 about it in the order of the kernel
    trainops_ref.gn_stats_kernel names (k_gn_chunk_stats: per-thread row sums, then one chain over the rpar x cpg partial sums;
    k_gn_chunk_stats4: (x + y) + (z + w) per row, the rows of a thread in one chain, the 256 / G row lanes in one chain, M2 as
    (a^2 + b^2) + (c^2 + d^2) from the same values), Chan's combine in k_gn_combine's order (nsl slices of chunks sl, sl + nsl, ...,
    then the slices in order).  full_weight_tail: the last, partial chunk counted as 64 rows (a fault)."""
    x = x.float()
    B, rpi, C = x.shape
    cpg, rpar = C // G, 256 // C
    nchunk = TR._cdiv(rpi, TR.GN_ROWS)
    f = torch.float32
    recs = []
    for ch in range(nchunk):
        blk = x[:, ch * 64:min(rpi, (ch + 1) * 64)]                          # [B, n, C]
        n = blk.shape[1]

        def chain(vals):                                                    # vals [B, n, C] -> [B, G] in the kernel's order
            part = [_seq(vals[:, k::rpar]) for k in range(rpar)]
            t = torch.zeros(B, G)
            for k in range(rpar):
                pk = part[k].reshape(B, G, cpg)
                for j in range(cpg):
                    t = t + pk[:, :, j]
            return t

        def chain4(rowvals):                                                # rowvals [B, n, G]: lane rr owns rows rr, rr + 256 / G, ...
            lanes = 256 // G
            t = torch.zeros(B, G)
            for rr in range(lanes):
                t = t + _seq(rowvals[:, rr::lanes])
            return t
        if TR.gn_stats_kernel(C, G) == "k_gn_chunk_stats4":
            v = blk.reshape(B, n, G, 4)
            mu = chain4((v[..., 0] + v[..., 1]) + (v[..., 2] + v[..., 3])) / torch.tensor(float(n * 4))
            dv = v - mu.view(B, 1, G, 1)
            sq = dv * dv
            m2 = chain4((sq[..., 0] + sq[..., 1]) + (sq[..., 2] + sq[..., 3]))
        else:
            mu = chain(blk) / torch.tensor(float(n * cpg))
            dlt = blk - mu.repeat_interleave(cpg, 1).view(B, 1, C)
            m2 = chain(dlt * dlt)
        recs.append((float((64 if full_weight_tail else n) * cpg), mu, m2))
    nsl = 4 if G > 32 else 8

    def merge(state, nb, mb, qb):
        n, mean, m2 = state
        nt = n + nb
        d = mb - mean
        return nt, mean + d * (nb / nt), m2 + (qb + d * d * (n * nb / nt))
    slices = []
    for sl in range(nsl):
        st = (torch.zeros(B, G), torch.zeros(B, G), torch.zeros(B, G))
        for ch in range(sl, nchunk, nsl):
            nb, mb, qb = recs[ch]
            st = merge(st, torch.full((B, G), nb), mb, qb)
        slices.append(st)
    st = slices[0]
    for k in range(1, nsl):
        if float(slices[k][0].max()) > 0:
            st = merge(st, *slices[k])
    N, M, Q = st
    r = 1.0 / torch.sqrt(Q / N + torch.tensor(eps, dtype=f))
    return r.repeat_interleave(cpg, 1), (0.0 - M * r).repeat_interleave(cpg, 1)


def _seq(v):
    """[B, n, C] fp32 -> [B, C]: one chain over n."""
    acc = torch.zeros(v.shape[0], v.shape[2])
    for i in range(v.shape[1]):
        acc = acc + v[:, i]
    return acc


ROWS_COLSUM = [6400, 1600, 400, 1024, 256, 64]              # rows per image of the segmented column sums in production
ROWS_PROD = [(1, 1600, 384), (3, 256, 384), (1, 400, 512), (3, 64, 512), (3, 1024, 128), (1, 2047, 112), (1, 2048, 112), (2, 6400, 112),
             (1, 25600, 112)]                                # (B, rows, C): the eSE and SM_Block sums and the slab classes of the issue
ROWS_GN = [6400, 1600, 400]


@pytest.mark.parametrize("rows", ROWS_COLSUM)
def test_headroom_colsum(rows):
    x = TR.scaled_inputs((2 * rows, 80), seed=rows)
    for beta in (0.0, 0.5):
        old = TR.scaled_inputs((2, 80), seed=1)
        ref, mag = TR.colsum(x, 2, beta, old)
        ok, ratios = _passes(emu_colsum(x, 2, beta, old), ref, mag, TR.d_colsum(rows, beta != 0.0))
        assert ok, f"colsum rows {rows} beta {beta}: worst (hard, rms) ratios {ratios}"
        assert max(ratios) < 0.5, ratios


@pytest.mark.parametrize("B,rows,C", ROWS_PROD)
@pytest.mark.parametrize("has_q", [False, True])
def test_headroom_prod_colsum(B, rows, C, has_q):
    C = min(C, 64)                                            # the summation order does not depend on the channel
    p = TR.scaled_inputs((B, rows, C), seed=rows, per_image=True)
    q = TR.scaled_inputs((B, rows, C), seed=rows + 1) if has_q else None
    for ws in (10 ** 9, 3 * B * C, B * C):
        S, per = TR.prod_colsum_plan(B, rows, C, ws)
        ref, mag = TR.prod_colsum(p, q, 1.0 / rows)
        ok, ratios = _passes(emu_prod_colsum(p, q, 1.0 / rows, S, per), ref, mag, TR.d_prod_colsum(rows, S, per, has_q))
        assert ok, f"prod_colsum {B}x{rows} S {S} per {per}: worst (hard, rms) ratios {ratios}"
        assert max(ratios) < 0.5, ratios


def test_prod_colsum_plan_classes():
    big = 10 ** 9
    assert TR.prod_colsum_plan(1, 2047, 112, big) == (1, 2048)
    assert TR.prod_colsum_plan(1, 2048, 112, big) == (4, 512)
    assert TR.prod_colsum_plan(1, 25600, 112, big) == (50, 512)
    assert TR.prod_colsum_plan(16, 25600, 112, big) == (31, 832)
    assert TR.prod_colsum_plan(16, 6400, 112, big) == (12, 576)
    assert TR.prod_colsum_plan(1, 25600, 112, 7 * 112) == (7, 3712)          # capped by the workspace
    assert TR.prod_colsum_plan(16, 6400, 112, 16 * 112) == (1, 6400)         # exactly B * C floats
    assert TR.prod_colsum_plan(1, 1600, 384, big) == (1, 1600)


# GroupNorm(32, 128) at every production map; the other group shapes (cpg 1 and 16) at the smallest, which keeps the emulation short
@pytest.mark.parametrize("rpi,C,G", [(r, 128, 32) for r in ROWS_GN] + [(400, 64, 64), (400, 128, 8), (100, 256, 16), (400, 64, 16)])
def test_headroom_groupnorm(rpi, C, G):
    B = 2
    x = TR.gn_inputs(B, rpi, C, G, seed=rpi + G)
    (r, rm), (a, am) = TR.gn_stats(x, G, 1e-5)
    er, ea = emu_gn_stats(x, G, 1e-5)
    d = TR.d_gn_stats(rpi, C, G)
    for name, got, ref, mag in (("rstd", er, r, rm), ("shift", ea, a, am)):
        ok, ratios = _passes(got, ref, mag, d)
        assert ok and max(ratios) < 0.5, f"GroupNorm {name} rpi {rpi} C {C} G {G}: worst (hard, rms) ratios {ratios}"
    # apply and backward from the fp32 statistics, every elementwise formula in fp32, the column sums in the kernel's order
    g = torch.Generator().manual_seed(1)
    gamma, beta = TR.scaled_inputs((C,), seed=2, lo=-1, hi=1), TR.scaled_inputs((C,), seed=3, lo=-1, hi=1)
    dy = TR.scaled_inputs((B, rpi, C), seed=4, per_image=True)
    yref, ymag = TR.gn_apply(x, er, ea, gamma, beta, True)
    with TR.precision(torch.float32):
        y32, _ = TR.gn_apply(x, er, ea, gamma, beta, True)
        gm = dy * (y32 > 0)
        xh = x * er.view(B, 1, C) + ea.view(B, 1, C)
    ok, ratios = _passes(y32, yref, ymag, TR.D_GN_APPLY)
    assert ok, f"gn_apply: {ratios}"
    sums = emu_colsum(torch.cat([gm, gm * xh], -1).reshape(B * rpi, 2 * C), B)
    cpg = C // G
    s1 = torch.zeros(B, G)
    s2 = torch.zeros(B, G)
    for j in range(cpg):
        s1 = s1 + (gamma * sums[:, :C]).reshape(B, G, cpg)[:, :, j]
        s2 = s2 + (gamma * sums[:, C:]).reshape(B, G, cpg)[:, :, j]
    inv_n = torch.tensor(1.0) / (torch.tensor(float(rpi)) * torch.tensor(float(cpg)))
    rep = lambda t: t.repeat_interleave(cpg, 1).view(B, 1, C)           # noqa: E731
    dx32 = er.view(B, 1, C) * (gamma * gm - (rep(s1) + xh * rep(s2)) * inv_n)
    out = TR.gn_bwd(dy, y32, x, er, ea, gamma, G, True)
    dd = TR.d_gn_bwd(rpi, cpg)
    for name, got in (("dx", dx32), ("dbeta", sums[:, :C]), ("dgamma", sums[:, C:])):
        ok, ratios = _passes(got, out[name][0], out[name][1], dd[name])
        assert ok and max(ratios) < 0.5, f"GroupNorm backward {name} rpi {rpi} C {C} G {G}: worst (hard, rms) ratios {ratios}"


def _corr_operands(B, H, W, C, seed, per_image=True):
    q = TR.scaled_inputs((B, H, W, C), seed=seed, per_image=True)
    ks = (B,) if per_image else ()
    g = torch.Generator().manual_seed(seed + 1)
    sk = 10.0 ** (torch.rand(*ks, C, generator=g) * 2 - 1)
    k11 = torch.randn(*ks, C, generator=g) * sk
    k13 = torch.randn(*ks, C, 3, generator=g) * sk.unsqueeze(-1)
    k31 = torch.randn(*ks, C, 3, generator=g) * sk.unsqueeze(-1)
    dcat = TR.scaled_inputs((B, H, W, 2 * C), seed=seed + 2, per_image=True)
    return q, k11, k13, k31, dcat


def test_headroom_elementwise():
    """The elementwise kernels with their formulas evaluated in fp32 (one rounding per operation) against float64."""
    B, H, W, C = 3, 9, 11, 32
    q, k11, k13, k31, dcat = _corr_operands(B, H, W, C, 3)
    ref = TR.corr_fwd(q, k11, k13, k31)
    with TR.precision(torch.float32):
        f32 = TR.corr_fwd(q, k11, k13, k31)
    worst = {}
    for k in ("cat", "t", "u"):
        ok, worst[k] = _passes(f32[k][0], ref[k][0], ref[k][1], TR.D_CORR_FWD)
        assert ok, (k, worst[k])
    T, Us = f32["t"][0], f32["u"][0]
    rb = TR.corr_bwd(q, k11, k13, k31, dcat, T, Us)
    with TR.precision(torch.float32):
        b32 = TR.corr_bwd(q, k11, k13, k31, dcat, T, Us)
    ok, worst["dq"] = _passes(b32["dq"][0], rb["dq"][0], rb["dq"][1], TR.D_CORR_DQ)
    assert ok, worst
    x = TR.scaled_inputs((B, H * W, C), seed=5, per_image=True)
    s, v = TR.scaled_inputs((B, C), seed=6), TR.scaled_inputs((B, C), seed=7)
    for fn, args, d in ((TR.scale_add, (x, s, v), TR.D_SCALE_ADD), (TR.combine2, (x, x.flip(1), s, v), TR.D_COMBINE2),
                        (TR.sumpool2, (x.reshape(B, H, W, C),), TR.D_SUMPOOL)):
        r, m = fn(*args)
        with TR.precision(torch.float32):
            g32, _ = fn(*args)
        ok, worst[fn.__name__] = _passes(g32, r, m, d)
        assert ok, worst
    assert max(max(v) for v in worst.values()) < 1.0, worst


def emu_apool_fwd(x, OH, OW):
    """fp32 ore_adaptive_avgpool_nhwc_fwd in the order of the kernel trainops_ref.apool_kernel names: k_apool_fwd adds a bin's pixels in
    (y, x) order; k_apool_fwd_big deals pixel i of the bin to slice i % nsl, nsl = 256 / (C / 4), and adds the slices in order."""
    x = x.float()
    B, H, W, C = x.shape
    big = TR.apool_kernel(H, W, C, OH, OW) == "k_apool_fwd_big"
    nsl = 256 // (C // 4)
    out = torch.zeros(B, OH, OW, C)
    for oy, (y0, y1) in enumerate(TR.apool_bins(H, OH)):
        for ox, (x0, x1) in enumerate(TR.apool_bins(W, OW)):
            px = x[:, y0:y1, x0:x1].reshape(B, -1, C)
            if big:
                acc = _seq(px[:, 0::nsl])
                for k in range(1, nsl):
                    acc = acc + _seq(px[:, k::nsl])
            else:
                acc = _seq(px)
            out[:, oy, ox] = acc / torch.tensor(float(px.shape[1]))
    return out


def emu_apool_bwd(dy, H, W):
    """fp32 ore_adaptive_avgpool_nhwc_bwd: a pixel adds dy / |bin| of the bins that cover it in (oy, ox) order."""
    dy = dy.float()
    B, OH, OW, C = dy.shape
    out = torch.zeros(B, H, W, C)
    for oy, (y0, y1) in enumerate(TR.apool_bins(H, OH)):
        for ox, (x0, x1) in enumerate(TR.apool_bins(W, OW)):
            out[:, y0:y1, x0:x1] = out[:, y0:y1, x0:x1] + (dy[:, oy, ox] / torch.tensor(float((y1 - y0) * (x1 - x0)))).view(B, 1, 1, C)
    return out


@pytest.mark.parametrize("B,H,W,C,OH,OW", [(2, 32, 32, 128, 1, 1), (2, 32, 32, 128, 3, 1), (2, 16, 16, 128, 1, 3), (2, 8, 8, 128, 1, 1),
                                           (2, 30, 30, 16, 32, 32), (1, 5, 5, 4, 9, 12), (2, 7, 11, 20, 3, 4), (2, 31, 29, 224, 1, 1)])
def test_headroom_adaptive_pool(B, H, W, C, OH, OW):
    x = TR.scaled_inputs((B, H, W, C), seed=H + OW, per_image=True)
    ok, ratios = _passes(emu_apool_fwd(x, OH, OW), *TR.apool_fwd(x, OH, OW), TR.d_apool(H, W, C, OH, OW))
    assert ok and max(ratios) < 0.5, f"{TR.apool_kernel(H, W, C, OH, OW)} {(H, W, C, OH, OW)}: worst (hard, rms) ratios {ratios}"
    dy = TR.scaled_inputs((B, OH, OW, C), seed=H + OW + 1, per_image=True)
    ok, ratios = _passes(emu_apool_bwd(dy, H, W), *TR.apool_bwd(dy, H, W), TR.d_apool_bwd(H, W, OH, OW))
    assert ok, f"k_apool_bwd {(H, W, OH, OW)}: worst (hard, rms) ratios {ratios}"


@pytest.mark.parametrize("rps", [6400, 400, 64])
def test_headroom_correlation_dk(rps):
    """dk11 / dk13 / dk31: the per-row products in fp32, summed per image in the order of the segmented column sums."""
    B, C = 2, 16
    H, W = (80, 80) if rps == 6400 else (20, 20) if rps == 400 else (8, 8)
    q, k11, k13, k31, dcat = _corr_operands(B, H, W, C, rps)
    with TR.precision(torch.float32):
        f32 = TR.corr_fwd(q, k11, k13, k31)
    T, Us = f32["t"][0], f32["u"][0]
    ref = TR.corr_bwd(q, k11, k13, k31, dcat, T, Us)
    with TR.precision(torch.float32):
        got = TR.corr_bwd(q, k11, k13, k31, dcat, T, Us, segsum=emu_colsum)
    d = TR.d_corr_dk(rps)
    for k in ("dk11", "dk13", "dk31"):
        ok, ratios = _passes(got[k][0].reshape(B, -1), ref[k][0].reshape(B, -1), ref[k][1].reshape(B, -1), d)
        assert ok and max(ratios) < 0.5, f"{k} rows per image {rps}: worst (hard, rms) ratios {ratios}"


def test_headroom_small_ops():
    """Max-pool backward, combine2 backward, the accumulating transpose, group_mean: their formulas in fp32."""
    xq = (torch.randn(3, 16, 16, 32, generator=torch.Generator().manual_seed(2)) * 1.5).round()
    dy = TR.scaled_inputs((3, 8, 8, 32), seed=3, per_image=True)
    ref, mag = TR.maxpool_bwd(xq, dy)
    with TR.precision(torch.float32):
        got, _ = TR.maxpool_bwd(xq, dy)
    assert _passes(got, ref, mag, TR.D_MAXPOOL_BWD)[0]
    g = TR.scaled_inputs((3, 64, 32), seed=4, per_image=True)
    a0, a1, v = (TR.scaled_inputs((3, 32), seed=5 + i, lo=-1, hi=1) for i in range(3))
    want = TR.combine2_bwd(g, a0, a1, v)
    with TR.precision(torch.float32):
        got = TR.combine2_bwd(g, a0, a1, v)
    for (gr, _), (r, m) in zip(got, want):
        assert _passes(gr, r, m, TR.D_COMBINE2_BWD)[0]
    base, add = TR.scaled_inputs((64, 32), seed=8), TR.scaled_inputs((64, 32), seed=9)
    assert _passes(base + add, base.double() + add.double(), base.double().abs() + add.double().abs(), TR.D_ACCUMULATE)[0]
    for G, N in ((2, 24), (3, 5)):
        x = TR.scaled_inputs((G * N, 40, 32), seed=N, per_image=True)
        acc = torch.zeros(G, 40, 32)
        for n in range(N):
            acc = acc + x.reshape(G, N, 40, 32)[:, n]
        got = acc * (torch.tensor(1.0) / torch.tensor(float(N)))
        ok, ratios = _passes(got, *TR.group_mean(x, G), TR.d_group_mean(N))
        assert ok and max(ratios) < 0.5, (N, ratios)
        dyg = TR.scaled_inputs((G, 40, 32), seed=N + 1)
        gb = (dyg * (torch.tensor(1.0) / torch.tensor(float(N)))).repeat_interleave(N, 0)
        assert _passes(gb, *TR.group_mean_bwd(dyg, G, N), 2)[0]


@pytest.mark.parametrize("B,H,W,C", [(1, 40, 40, 96), (4, 16, 16, 96), (1, 64, 64, 32)])
def test_headroom_ese_node(B, H, W, C):
    """The eSE node in fp32: the pooled sums in k_colsum_seg's order, the [B, C] x [C, C] products as fp32 matmuls, the rest elementwise."""
    x, w, b = TR.ese_inputs(B, H, W, C, seed=H)
    dy = TR.scaled_inputs((B, H, W, C), seed=H + 1, per_image=True)
    n = H * W
    plan = TR.prod_colsum_plan(B, n, C, 10 ** 12)
    Wm = w.reshape(C, C)
    m = emu_prod_colsum(x, None, 1.0 / n, *plan)
    z = torch.addmm(b, m, Wm.t())
    g = F.hardsigmoid(z)
    y = x * g.view(B, 1, 1, C)
    dg = emu_prod_colsum(dy, x, 1.0, *plan)
    dz = torch.where(z.abs() < 3, dg / 6, torch.zeros_like(dg))
    dm = dz @ Wm
    dx = dy * g.view(B, 1, 1, C) + (dm / n).view(B, 1, 1, C)
    ref = TR.ese_node(x, w, b, dy)
    assert bool(((z.abs() < 3) == (ref["z"].abs() < 3)).all())
    d = TR.d_ese(n, C, B, plan, plan)
    for name, got in (("m", m), ("y", y), ("dx", dx), ("dW", dz.t() @ m), ("db", dz.sum(0).reshape(1, C))):
        r, mg = ref[name]
        ok, ratios = _passes(got, r.reshape(got.shape), mg.reshape(got.shape), d[name])
        assert ok and max(ratios) < 0.5, f"eSE {name} {(B, H, W, C)}: worst (hard, rms) ratios {ratios}"


# ---- faults ----------------------------------------------------------------------------------------------------------------------
def _fails(got, ref, mag, d):
    ok, ratios = _passes(got, ref, mag, d)
    return not ok


def test_fault_dropped_chunk_and_slab():
    rows = 1600
    x = TR.scaled_inputs((3 * rows, 48), seed=1)
    ref, mag = TR.colsum(x, 3)
    assert _passes(emu_colsum(x, 3), ref, mag, TR.d_colsum(rows))[0]
    assert _fails(emu_colsum(x, 3, drop=(1, 4)), ref, mag, TR.d_colsum(rows))           # a 256-row chunk of segment 1
    assert _fails(emu_colsum(x, 3, drop=(2, 6)), ref, mag, TR.d_colsum(rows))           # the last, 64-row chunk of segment 2
    p = TR.scaled_inputs((2, 6400, 32), seed=2)
    S, per = TR.prod_colsum_plan(2, 6400, 32, 10 ** 9)
    assert S > 2
    ref, mag = TR.prod_colsum(p, None, 1.0)
    d = TR.d_prod_colsum(6400, S, per, False)
    assert _passes(emu_prod_colsum(p, None, 1.0, S, per), ref, mag, d)[0]
    assert _fails(emu_prod_colsum(p, None, 1.0, S, per, drop_slab=S - 1), ref, mag, d)


def test_fault_chan_tail_weight():
    rpi = 400                                                                          # 6 chunks of 64 and one of 16
    x = TR.gn_inputs(2, rpi, 128, 32, seed=3)
    (r, rm), (a, am) = TR.gn_stats(x, 32, 1e-5)
    d = TR.d_gn_stats(rpi, 128, 32)
    er, ea = emu_gn_stats(x, 32, 1e-5, full_weight_tail=True)
    assert _fails(er, r, rm, d) or _fails(ea, a, am, d)


def test_fault_neighbouring_image():
    """Statistics / gates of image b applied to image b + 1: local to the images, the smallest of which the max-norm cannot see."""
    B, rpi, C = 3, 100, 64
    x = TR.gn_inputs(B, rpi, C, 16, seed=4)
    (r, _), (a, _) = TR.gn_stats(x, 16, 1e-5)
    r, a = r.float(), a.float()
    one, zero = torch.ones(C), torch.zeros(C)
    ref, mag = TR.gn_apply(x, r, a, one, zero, False)
    with TR.precision(torch.float32):
        bad, _ = TR.gn_apply(x, r.roll(1, 0), a.roll(1, 0), one, zero, False)
    assert _fails(bad, ref, mag, TR.D_GN_APPLY)
    xs = TR.scaled_inputs((B, rpi, C), seed=5)
    xs[1] *= 1e-6                                                                        # one image far below the others
    s = torch.rand(B, C) + 0.5
    ref, mag = TR.scale_add(xs, s)
    wrong = s.clone()
    wrong[1] = s[0]                                                                      # image 1 gets the gate of image 0
    with TR.precision(torch.float32):
        bad, _ = TR.scale_add(xs, wrong)
        good, _ = TR.scale_add(xs, s)
    assert _passes(good, ref, mag, TR.D_SCALE_ADD)[0]
    assert _fails(bad, ref, mag, TR.D_SCALE_ADD)
    assert TR.close_old(bad, ref), "the max-norm criterion was expected to miss the small image"


def test_fault_correlation_seams_and_taps():
    q, k11, k13, k31, dcat = _corr_operands(3, 5, 6, 16, 6)
    ref = TR.corr_fwd(q, k11, k13, k31)
    for wrap in ("image", "row"):
        bad = TR.corr_fwd(q, k11, k13, k31, wrap=wrap)
        assert any(_fails(bad[k][0], ref[k][0], ref[k][1], TR.D_CORR_FWD) for k in ("cat", "t", "u")), wrap
    T, Us = ref["t"][0].float(), ref["u"][0].float()
    rb = TR.corr_bwd(q, k11, k13, k31, dcat, T, Us)
    bad = TR.corr_bwd(q, k11, k13, k31, dcat, T, Us, reverse_taps=True)
    d = TR.d_corr_dk(30)
    assert _fails(bad["dk13"][0], rb["dk13"][0], rb["dk13"][1], d) and _fails(bad["dk31"][0], rb["dk31"][0], rb["dk31"][1], d)
    assert _passes(bad["dk11"][0], rb["dk11"][0], rb["dk11"][1], d)[0]


def test_fault_groupnorm_n_and_slice():
    B, rpi, C, G = 2, 100, 64, 16
    x = TR.gn_inputs(B, rpi, C, G, seed=7)
    (r, _), (a, _) = TR.gn_stats(x, G, 1e-5)
    r, a = r.float(), a.float()
    gamma = torch.rand(C) + 0.5
    dy = TR.scaled_inputs((B, rpi, C), seed=8)
    y, _ = TR.gn_apply(x, r, a, gamma, torch.zeros(C), True)
    ref = TR.gn_bwd(dy, y, x, r, a, gamma, G, True)
    d = TR.d_gn_bwd(rpi, C // G)
    bad = TR.gn_bwd(dy, y, x, r, a, gamma, G, True, n_wrong=True)                       # n = rpi instead of rpi * cpg
    assert _fails(bad["dx"][0], *ref["dx"], d["dx"])
    # coff on the wrong operand: x is the slice [coff, coff + C) of rows of ld floats with NaN around it.  The kernel's two reads are
    # dy + row * C and x + row * ld + coff; the fault reads dy + row * C + coff and x + row * ld.
    coff, ld = 8, C + 24
    buf = torch.full((B, rpi, ld), float("nan"))
    buf[..., coff:coff + C] = x
    dy_shift = torch.cat([dy.reshape(-1)[coff:], torch.zeros(coff)]).reshape(dy.shape)
    good = TR.gn_bwd(dy, y, buf[..., coff:coff + C], r, a, gamma, G, True)
    assert all(_passes(good[k][0], *ref[k], d[k])[0] for k in ("dx", "dbeta", "dgamma"))
    bad = TR.gn_bwd(dy, y, buf[..., :C], r, a, gamma, G, True)                          # x without its offset: reads the NaN border
    assert all(_fails(bad[k][0], *ref[k], d[k]) for k in ("dx", "dgamma"))
    bad = TR.gn_bwd(dy_shift, y, buf[..., coff:coff + C], r, a, gamma, G, True)         # the offset on dy instead
    assert all(_fails(bad[k][0], *ref[k], d[k]) for k in ("dx", "dbeta", "dgamma"))


def test_fault_apool_edge_and_maxpool_tie():
    x = TR.scaled_inputs((2, 7, 11, 8), seed=9)
    assert [b - a for a, b in TR.apool_bins(11, 4)] == [3, 4, 4, 3]                      # the edge bins are the smaller ones
    ref, mag = TR.apool_fwd(x, 3, 4)
    bad, _ = TR.apool_fwd(x, 3, 4, interior_count=True)
    assert _fails(bad, ref, mag, TR.d_apool(7, 11, 8, 3, 4))
    assert _passes(bad[:, :, 1:3], ref[:, :, 1:3], mag[:, :, 1:3], TR.d_apool(7, 11, 8, 3, 4))[0]      # the interior bins are right
    xq = (torch.randn(2, 9, 7, 4, generator=torch.Generator().manual_seed(1)) * 1.5).round()
    dy = TR.scaled_inputs((2, 4, 3, 4), seed=10)
    ref, mag = TR.maxpool_bwd(xq, dy)
    bad, _ = TR.maxpool_bwd(xq, dy, last=True)
    assert _fails(bad, ref, mag, TR.D_MAXPOOL_BWD)


def test_fault_small_channel_block():
    """A 1e-3 relative error confined to the smallest-scale channel of one 16-row block: both bounds see it, the max-norm does not."""
    x = TR.scaled_inputs((4, 64, 48), seed=11)
    s = torch.rand(4, 48) + 0.5
    ref, mag = TR.scale_add(x, s)
    with TR.precision(torch.float32):
        got, _ = TR.scale_add(x, s)
    assert _passes(got, ref, mag, TR.D_SCALE_ADD)[0]
    c = int(x.double().pow(2).mean((0, 1)).argmin())
    bad = got.clone()
    bad[2, 16:32, c] *= 1.0 + 1e-3
    h, r = TR.check2(bad, ref, mag, TR.D_SCALE_ADD)
    assert h > 1 and r > 1, (h, r)
    assert TR.close_old(bad, ref)


# ---- coverage --------------------------------------------------------------------------------------------------------------------
def test_every_autograd_call_is_covered_or_listed():
    with open(os.path.join(PKG, "orehip", "autograd.py")) as f:
        called = set(re.findall(r"\borehip\.(\w+)\(", f.read()))
    assert called, "no orehip calls found in orehip/autograd.py"
    covered = TR.covered_functions()
    both = covered & set(TR.NOT_COVERED)
    assert not both, f"both covered and listed as left out: {sorted(both)}"
    missing = called - covered - set(TR.NOT_COVERED)
    assert not missing, f"orehip functions on the training path neither covered nor listed: {sorted(missing)}"
    stale = (covered | set(TR.NOT_COVERED)) - called
    assert stale <= {"colsum_segments"}, f"listed but not called from orehip/autograd.py: {sorted(stale)}"      # (a C-level helper's wrapper)
    for op, (fns, classes) in TR.TRAIN_OPS.items():
        assert len(set(classes)) == len(classes), op
        for cls in classes:
            big = TR.batch16(op, cls)
            assert big[0] == 16 * cls[0] and big[1:] == tuple(cls[1:]), (op, cls, big)
