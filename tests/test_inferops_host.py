"""CPU: the float64 restatements of tests/inferops_ref.py and their two bounds have teeth, and the coverage table is complete.

tests/inferops_ref.py restates the inference-only non-conv kernels in float64, to be held to the element-wise bound 2 d u mag and the
16 x 16 block rms bound C_S u sqrt(d) (it derives every d).  Here, without a GPU:
  * an fp32 emulation of each kernel in its documented order (the stem's 28-step fma chain; the head's 36-step fma chain per quad, four
    chains of 8 quads, (s0 + s1) + (s2 + s3); the eSE partial sums over row lanes, slices and the 64-lane dot product with its
    shuffle butterfly; the support kernels' lane chains; ROIAlign with fp32 coordinates, weights and sample chain; the correlation
    evaluated in fp32) passes both bounds at every edge class of the GPU file -- the assertion message carries the worst ratio;
  * each fault the bounds are there to catch fails at least one of them;
  * the ROI box generator keeps its margins for every seed the GPU file uses, and fp32 and float64 agree on every discrete
    decision of the generated and of the exact boxes;
  * every __global__ of csrc/ore_misc.hip and csrc/ore_roi.hip is in INFER_OPS or, with the test that pins it, in NOT_COVERED (the
    training forward partners in ore_misc.hip -- the GroupNorm statistics, the max-pool -- are kernels the inference path runs too, so
    they are in INFER_OPS as well as behind trainops_ref.TRAIN_OPS)."""
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import inferops_ref as IR
import trainops_ref as TR
from conftest import PKG

F32, F64 = torch.float32, torch.float64
BOX_SEEDS = (0, 1)                  # the seeds tests/test_hip_inferops.py draws its 64 boxes from, per pyramid


def _ratios(got, ref, mag, d):
    return TR.check2(got, ref, mag, d)


def _passes(got, ref, mag, d):
    h, r = _ratios(got, ref, mag, d)
    return h <= 1 and r <= 1


def _fma(a, b, c):
    """fp32 fma: the product of two fp32 values is exact in float64; one rounding of the sum (the float64 addition's own rounding is
    2^-29 of that)."""
    return (a.double() * b.double() + c.double()).float()


def _butterfly(s):
    """acc += shfl_xor(acc, d) for d = 32 .. 1 over the last axis of 64 lanes; every lane ends with the same value, lane 0 returned."""
    lanes = torch.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        s = s + s[..., lanes ^ d]
    return s[..., 0]


def _block_error(ref, mag, rel=1e-3):
    """ref with a relative error `rel` (of mag) in the first 16 x 16 block of the channel group that holds the smallest-magnitude
    channel."""
    r2, m2 = ref.reshape(-1, ref.shape[-1]), mag.reshape(-1, ref.shape[-1])
    c = int(m2.mean(0).argmin()) // 16 * 16
    got = r2.clone()
    got[:16, c:c + 16] += rel * m2[:16, c:c + 16]
    return got.reshape(ref.shape)


# ---- stem ------------------------------------------------------------------------------------------------------------------------
def stem_emulation(img, Hp, Wp, mean, std, w, scale, shift):
    """k_stem1 in fp32: a = (x - mean) / std (two roundings), 0 outside the image; acc = fma chain over k = c * 9 + ky * 3 + kx =
    0 .. 26 (tap 27 is the zero pad); relu(acc * scale + shift)."""
    B, _, H, W = img.shape
    m, s = torch.tensor(mean, dtype=F32).view(1, 3, 1, 1), torch.tensor(std, dtype=F32).view(1, 3, 1, 1)
    a = F.pad((img.float() - m) / s, (0, Wp - W, 0, Hp - H))
    cols = F.unfold(a, 3, padding=1, stride=2)                            # [B, 27, Ho * Wo], k = c * 9 + ky * 3 + kx
    Cout = w.shape[0]
    wk = w.reshape(Cout, 27)
    acc = torch.zeros(B, Cout, cols.shape[-1], dtype=F32)
    for k in range(27):
        acc = _fma(wk[:, k].view(1, Cout, 1), cols[:, k].unsqueeze(1), acc)
    v = (acc * scale.view(1, Cout, 1) + shift.view(1, Cout, 1)).clamp(min=0)
    return v.permute(0, 2, 1).reshape(B, Hp // 2, Wp // 2, Cout)


@pytest.mark.parametrize("u8", [True, False])
@pytest.mark.parametrize("case", IR.STEM_CASES, ids=str)
def test_stem_emulation_within_bounds(case, u8):
    B, H, W, Hp, Wp, Cout = case
    img, mean, std, w, scale, shift = IR.stem_inputs(B, H, W, Cout, u8, seed=H + W)
    ref, mag = IR.stem_ref(img, Hp, Wp, mean, std, w, scale, shift)
    h, r = _ratios(stem_emulation(img, Hp, Wp, mean, std, w, scale, shift), ref, mag, IR.D_STEM)
    assert h <= 1 and r <= 1, (case, u8, h, r)
    assert bool((mag >= ref.abs() * (1 - 1e-12)).all())


_STEM_FAULT_CASES = [(1, 75, 100, 76, 100, 64), (2, 1, 37, 2, 38, 64), (1, 3, 3, 4, 4, 64), (1, 20, 24, 64, 64, 64)]


@pytest.mark.parametrize("case,fault", [(c, f) for c in _STEM_FAULT_CASES for f in ("tap26", "channel", "pad")
                                        if not (f == "tap26" and c[1] == 1)], ids=str)         # one image row: tap (2, 2) is always padding
def test_stem_faults_fail(case, fault):
    B, H, W, Hp, Wp, Cout = case
    img, mean, std, w, scale, shift = IR.stem_inputs(B, H, W, Cout, True, seed=1)
    ref, mag = IR.stem_ref(img, Hp, Wp, mean, std, w, scale, shift)
    bad, _ = IR.stem_ref(img, Hp, Wp, mean, std, w, scale, shift, fault=fault)
    assert not _passes(bad, ref, mag, IR.D_STEM), (case, fault)


def test_stem_block_error_fails():
    img, mean, std, w, scale, shift = IR.stem_inputs(1, 33, 31, 64, True, seed=2)
    ref, mag = IR.stem_ref(img, 34, 32, mean, std, w, scale, shift)
    assert _passes(ref, ref, mag, IR.D_STEM) and not _passes(_block_error(ref, mag), ref, mag, IR.D_STEM)


# ---- head ------------------------------------------------------------------------------------------------------------------------
def head_emulation(tower, B, levels, mul, add, w5, scale, shift, drop_quad=None):
    """k_head_pred in fp32: t = relu(x * mul + add) staged once, zero halo; per (pixel, output, quad) one fma chain over the taps
    (dy, dx) with the quad's channels in the order w, z, y, x; the 32 quads into s0..s3 (quad k goes to s[k % 4], ascending k);
    (s0 + s1) + (s2 + s3); * scale + shift; relu on outputs 0..3.  drop_quad: that quad's partial sum is left out (a fault)."""
    C, outs, r0 = 128, [], 0
    for l, (H, W) in enumerate(levels):
        n = B * H * W
        x = tower[r0:r0 + n].reshape(B, H * W, C)
        t = (x * mul[l * B:(l + 1) * B].view(B, 1, C) + add[l * B:(l + 1) * B].view(B, 1, C)).clamp(min=0)
        tp = F.pad(t.reshape(B, H, W, C), (0, 0, 1, 1, 1, 1))
        acc = torch.zeros(B, H, W, 5, 32, dtype=F32)
        for dy in range(3):
            for dx in range(3):
                v = tp[:, dy:dy + H, dx:dx + W].reshape(B, H, W, 1, 32, 4)
                wq = w5[:, :, dy, dx].reshape(1, 1, 1, 5, 32, 4)
                for ch in (3, 2, 1, 0):
                    acc = _fma(v[..., ch], wq[..., ch], acc)
        if drop_quad is not None:
            acc[..., drop_quad] = 0.0
        a8 = acc.reshape(B, H, W, 5, 8, 4)
        s = torch.zeros(B, H, W, 5, 4, dtype=F32)
        for i in range(8):
            s = s + a8[..., i, :]
        v = (s[..., 0] + s[..., 1]) + (s[..., 2] + s[..., 3])
        v = v * scale[l, :5] + shift[l, :5]
        v = torch.cat([v[..., :4].clamp(min=0), v[..., 4:]], -1)
        outs.append(v.reshape(n, 5))
        r0 += n
    return torch.cat(outs)


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("levels", IR.HEAD_LEVELS, ids=str)
def test_head_emulation_within_bounds(levels, B):
    args = IR.head_inputs(B, levels, seed=len(levels) + B)
    tower, mul, add, w5, scale, shift = args
    ref, mag = IR.head_ref(tower, B, levels, *args[1:])
    h, r = _ratios(head_emulation(tower, B, levels, *args[1:]), ref, mag, IR.D_HEAD)
    assert h <= 1 and r <= 1, (levels, B, h, r)
    assert bool((mag >= ref.abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("levels", [[(9, 7)], [(1, 1)], [(10, 12), (5, 6), (3, 3)]], ids=str)
def test_head_faults_fail(levels):
    args = IR.head_inputs(2, levels, seed=3)
    tower = args[0]
    ref, mag = IR.head_ref(tower, 2, levels, *args[1:])
    assert not _passes(IR.head_ref(tower, 2, levels, *args[1:], fault="halo")[0], ref, mag, IR.D_HEAD), "un-zeroed halo"
    for quad in (0, 7, 31):
        assert not _passes(head_emulation(tower, 2, levels, *args[1:], drop_quad=quad), ref, mag, IR.D_HEAD), ("missing quad", quad)
    if len(levels) > 1:
        bad = IR.head_ref(tower, 2, levels, *args[1:], fault="stride5")[0]
        assert not _passes(bad, ref, mag, IR.D_HEAD), "epilogue stride 5"          # (NaN columns of the table reach level >= 1)
    assert not _passes(_block_error(ref, mag), ref, mag, IR.D_HEAD)


# ---- eSE -------------------------------------------------------------------------------------------------------------------------
def colsum_partial_emulation(x, P):
    """k_colsum_partial in fp32: x [B,HW,C] -> part [B,P,C]; part p holds the rows [p rows_per, (p + 1) rows_per); row lane rr adds
    the rows r0 + rr, r0 + rr + rpar, ...; lane 0 then adds the lanes 1 .. rpar - 1."""
    B, HW, C = x.shape
    cpb = min(C // 4, 256)
    rpar, rows_per = 256 // cpb, TR._cdiv(HW, P)
    part = torch.zeros(B, P, C, dtype=F32)
    for p in range(P):
        r0, r1 = p * rows_per, min((p + 1) * rows_per, HW)
        lanes = torch.zeros(rpar, B, C, dtype=F32)
        for rr in range(rpar):
            for r in range(r0 + rr, r1, rpar):
                lanes[rr] = lanes[rr] + x[:, r]
        acc = lanes[0]
        for k in range(1, rpar):
            acc = acc + lanes[k]
        part[:, p] = acc
    return part


def ese_gate_emulation(part, HW, fc_w, fc_b):
    """ese_gate16 in fp32: slices of parts, the slice chain, * fl(1 / HW); per wave the 64-lane dot product (lane k: terms k, k + 64,
    ... as product then addition), the butterfly, + bias + 3, clamp, / 6."""
    B, P, C = part.shape
    nsl = IR.ESE_T // (C // 4)
    sl = torch.zeros(nsl, B, C, dtype=F32)
    for p in range(P):
        sl[p % nsl] = sl[p % nsl] + part[:, p]
    m = sl[0]
    for k in range(1, nsl):
        m = m + sl[k]
    mean = m * (torch.tensor(1.0, dtype=F32) / torch.tensor(float(HW), dtype=F32))
    Cp = TR._cdiv(C, 64) * 64
    Wm = F.pad(fc_w.reshape(C, C), (0, Cp - C)).reshape(1, C, Cp // 64, 64)
    mp = F.pad(mean, (0, Cp - C)).reshape(B, 1, Cp // 64, 64)
    s = torch.zeros(B, C, 64, dtype=F32)
    for j in range(Cp // 64):
        s = s + Wm[:, :, j] * mp[:, :, j]
    v = _butterfly(s) + fc_b + 3.0
    return v.clamp(0, 6) / 6.0


ESE_P = IR.ESE_P


def test_ese_P_table_reaches_every_loop_count():
    """Per C: a P below 8 NSL (the unrolled loop runs zero times), one in [8 NSL, 16 NSL) and, where the table has a third, one in
    [16 NSL, 24 NSL), none of them a multiple of NSL (a remainder)."""
    for C, Ps in ESE_P.items():
        nsl = IR.ESE_T // (C // 4)
        runs = {(P - 1 - 7 * nsl) // (8 * nsl) + 1 if P > 7 * nsl else 0 for P in Ps}       # iterations of slice 0's unrolled loop
        assert {0, 1} <= runs, (C, runs)
        assert any(P % nsl for P in Ps)
    assert {IR.ESE_T % (C // 4) != 0 for C in IR.ESE_C} == {True, False}


@pytest.mark.parametrize("C", IR.ESE_C)
def test_ese_gate_emulation_within_bounds(C):
    worst = (0.0, 0.0)
    for B in (1, 3):
        for P in ESE_P[C] if C < 2048 or B == 1 else ESE_P[C][:2]:
            for HW, empty in ((400, None), (max(P - 2, 1), max(P - 2, 1))):                  # the second: P > HW, the last parts empty
                if P > 600 and HW != 400:
                    continue
                part, w, b = IR.ese_parts_inputs(B, P, HW, C, seed=C + P, empty_from=empty)
                ref, mag, z = IR.ese_gate_from_parts_ref(part, HW, w, b)
                assert float((z.abs() - 3.0).abs().min()) >= TR.ESE_KNEE_MARGIN
                h, r = _ratios(ese_gate_emulation(part, HW, w, b), ref, mag, IR.d_ese_gate(HW, C, P))
                worst = (max(worst[0], h), max(worst[1], r))
    assert worst[0] <= 1 and worst[1] <= 1, (C, worst)


@pytest.mark.parametrize("C,HW,B", [(16, 1, 1), (20, 15, 3), (112, 400, 1), (384, 15, 3), (528, 400, 1), (2048, 15, 1)])
def test_ese_gate_from_map_emulation_within_bounds(C, HW, B):
    x, w, b = TR.ese_inputs(B, 1, HW, C, seed=C + HW)
    x = x.reshape(B, HW, C)
    ref, mag, z = IR.ese_gate_ref(x, w, b)
    assert float((z.abs() - 3.0).abs().min()) >= TR.ESE_KNEE_MARGIN
    P = IR.ese_plan_P(HW)
    got = ese_gate_emulation(colsum_partial_emulation(x, P), HW, w.reshape(C, C), b)
    h, r = _ratios(got, ref, mag, IR.d_ese_colsum(HW, C, P) + IR.d_ese_gate(HW, C, P))
    assert h <= 1 and r <= 1, (C, HW, B, h, r)


@pytest.mark.parametrize("C,P,HW", [(20, 4, 15), (112, 13, 400), (512, 7, 400), (528, 23, 15)])
def test_ese_faults_fail(C, P, HW):
    part, w, b = IR.ese_parts_inputs(3, P, HW, C, seed=5)
    ref, mag, _ = IR.ese_gate_from_parts_ref(part, HW, w, b)
    d = IR.d_ese_gate(HW, C, P)
    rows_per = TR._cdiv(HW, P)
    assert P * rows_per != HW
    assert not _passes(IR.ese_gate_from_parts_ref(part, HW, w, b, HW_div=P * rows_per)[0], ref, mag, d), "mean over P * rows_per"
    twice = list(range(P)) + [P - 1]                                # an empty part that repeats the last real one
    assert not _passes(IR.ese_gate_from_parts_ref(part, HW, w, b, parts=twice)[0], ref, mag, d), "an empty part counted"
    assert not _passes(_block_error(ref, mag), ref, mag, d)


# ---- correlation -------------------------------------------------------------------------------------------------------------------
def _corr_inputs(B, H, W, C, seed):
    q = TR.scaled_inputs((B, H, W, C), seed, per_image=True)
    g = torch.Generator().manual_seed(seed + 1)
    sk = 10.0 ** (torch.rand(C, generator=g) * 2 - 1)
    return q, torch.randn(C, generator=g) * sk, torch.randn(C, 3, generator=g) * sk.view(C, 1), torch.randn(C, 3, generator=g) * sk.view(C, 1)


@pytest.mark.parametrize("C", [4, 128])
@pytest.mark.parametrize("B,H,W", IR.CORR_MAPS + [(2, 6, 7), (2, 2, 2)])
def test_correlation_emulation_within_bounds(B, H, W, C):
    q, k11, k13, k31 = _corr_inputs(B, H, W, C, seed=H * W + C)
    ref, mag = IR.corr_infer_ref(q, k11, k13, k31)
    with TR.precision(F32):
        got, _ = IR.corr_infer_ref(q, k11, k13, k31)
    h, r = _ratios(got, ref, mag, IR.D_CORR_FWD)
    assert h <= 1 and r <= 1, (B, H, W, C, h, r)


@pytest.mark.parametrize("B,H,W", [(2, 1, 7), (3, 5, 6), (2, 2, 2)])
def test_correlation_faults_fail(B, H, W):
    """Without the zero rows of the 1 x 3 result at y = -1 and y = H the 3 x 1 conv reads the neighbouring image's rows."""
    q, k11, k13, k31 = _corr_inputs(B, H, W, 128, seed=7)
    ref, mag = IR.corr_infer_ref(q, k11, k13, k31)
    assert not _passes(IR.corr_infer_ref(q, k11, k13, k31, wrap="image")[0], ref, mag, IR.D_CORR_FWD)
    if W > 1 and H > 1:
        assert not _passes(IR.corr_infer_ref(q, k11, k13, k31, wrap="row")[0], ref, mag, IR.D_CORR_FWD)
    assert not _passes(_block_error(ref, mag), ref, mag, IR.D_CORR_FWD)


# ---- support kernels -----------------------------------------------------------------------------------------------------------------
def support_emulation(proto, floor_end=False):
    """k_support_kernels in fp32: lane i adds the pixels i, i + 64, ... of each window in one chain, the butterfly, the division.
    floor_end: the window end floor((j + 1) s / 3) instead of ceil (a fault)."""
    C, s, _ = proto.shape
    n = s * s
    npad = TR._cdiv(n, 64) * 64
    idx = torch.arange(npad)
    y, x = idx // s, idx % s
    lo = [(j * s) // 3 for j in range(3)]
    hi = [((j + 1) * s) // 3 if floor_end else ((j + 1) * s + 2) // 3 for j in range(3)]
    masks = [idx < n] + [(idx < n) & (x >= lo[j]) & (x < hi[j]) for j in range(3)] + [(idx < n) & (y >= lo[j]) & (y < hi[j]) for j in range(3)]
    p = F.pad(proto.reshape(C, n), (0, npad - n)).reshape(C, npad // 64, 64)
    sums = []
    for m in masks:
        mk = m.reshape(npad // 64, 64)
        acc = torch.zeros(C, 64, dtype=F32)
        for j in range(npad // 64):
            acc = acc + p[:, j] * mk[j]
        sums.append(_butterfly(acc))
    den = [float(s * max(hi[j] - lo[j], 0)) for j in range(3)]
    k13 = torch.stack([sums[1 + j] / den[j] if den[j] else sums[1 + j] * 0 for j in range(3)], 1)
    k31 = torch.stack([sums[4 + j] / den[j] if den[j] else sums[4 + j] * 0 for j in range(3)], 1)
    return {"k11": sums[0] / float(n), "k13": k13, "k31": k31}


@pytest.mark.parametrize("C", IR.SUPPORT_C)
@pytest.mark.parametrize("s", IR.SUPPORT_S)
def test_support_kernels_emulation_within_bounds(s, C):
    proto = TR.scaled_inputs((s, s, C), s + C).permute(2, 0, 1).contiguous() + TR.scaled_inputs((1, 1, C), 99).permute(2, 0, 1)
    ref = IR.support_kernels_ref(proto)
    got = support_emulation(proto)
    for k in ("k11", "k13", "k31"):
        h, r = _ratios(got[k].reshape(C, -1), ref[k][0].reshape(C, -1), ref[k][1].reshape(C, -1), IR.d_support(s))
        assert h <= 1 and r <= 1, (s, C, k, h, r)


@pytest.mark.parametrize("s", [s for s in IR.SUPPORT_S if s % 3])
def test_support_kernels_floor_fault_fails(s):
    proto = TR.scaled_inputs((s, s, 5), s).permute(2, 0, 1).contiguous() + 1.0
    ref = IR.support_kernels_ref(proto)
    bad = support_emulation(proto, floor_end=True)
    assert any(not _passes(bad[k].reshape(5, -1), ref[k][0].reshape(5, -1), ref[k][1].reshape(5, -1), IR.d_support(s)) for k in ("k13", "k31"))


def test_support_kernels_reference_is_adaptive_avg_pool():
    for s in (2, 5, 8):
        proto = torch.randn(6, s, s, dtype=F64)
        ref = IR.support_kernels_ref(proto)
        assert torch.allclose(ref["k11"][0], F.adaptive_avg_pool2d(proto, 1).reshape(6), rtol=1e-12, atol=0)
        assert torch.allclose(ref["k13"][0], F.adaptive_avg_pool2d(proto, (1, 3)).reshape(6, 3), rtol=1e-12, atol=0)
        assert torch.allclose(ref["k31"][0], F.adaptive_avg_pool2d(proto, (3, 1)).reshape(6, 3), rtol=1e-12, atol=0)


# ---- ROIAlign ------------------------------------------------------------------------------------------------------------------------
def _roi_feats(pyramid, C, B, seed):
    _, _, HWs = IR.roi_pyramid(pyramid)
    return [TR.scaled_inputs((B, h, w, C), seed + l, per_image=B > 1) for l, (h, w) in enumerate(HWs)]


@pytest.mark.parametrize("pyramid", list(IR.ROI_PYRAMIDS))
@pytest.mark.parametrize("seed", BOX_SEEDS)
def test_roi_box_margins(pyramid, seed):
    """Every generated box keeps ROI_MARGIN at every pooled size, and numpy float32 (correctly rounded +, -, *, /, sqrt; the level by
    comparisons with exact powers of two, no log2) takes the decisions float64 takes.  All levels are drawn."""
    scales, ml, HWs = IR.roi_pyramid(pyramid)
    boxes, seeds = IR.roi_boxes(64, seed, pyramid)
    assert boxes.shape == (64, 4) and len(set(seeds)) == 64
    levels = set()
    for b in boxes:
        for P in IR.ROI_POOLED:
            assert IR.roi_margins(b, scales, ml, P, HWs) >= IR.ROI_MARGIN
            a, c = IR.roi_decisions(b, scales, ml, P, HWs, np.float32), IR.roi_decisions(b, scales, ml, P, HWs, np.float64)
            assert (a["level"], a["gh"], a["gw"]) == (c["level"], c["gh"], c["gw"])
            assert bool((a["vy"] == c["vy"]).all()) and bool((a["vx"] == c["vx"]).all())
            levels.add(c["level"])
    assert levels == set(range(len(scales)))


@pytest.mark.parametrize("pyramid", list(IR.ROI_PYRAMIDS))
def test_roi_exact_boxes_are_exact(pyramid):
    """Coordinates in 1/8 px; sqrt(area) / 224 a power of two computed without rounding (or a degenerate area); fp32 and float64
    agree on every decision at every pooled size; the list holds boxes ON a level threshold, ON an integer of rh / P, with a sample
    ON y == H, with gh <= 0 and with no valid sample."""
    scales, ml, HWs = IR.roi_pyramid(pyramid)
    on_level = on_grid = on_H = empty = outside = 0
    for b in IR.ROI_EXACT_BOXES:
        assert all(float(v * 8).is_integer() for v in b)
        area = (np.float64(b[2]) - b[0]) * (np.float64(b[3]) - b[1])
        if area > 0:
            ratio = math.sqrt(area) / 224.0
            assert math.log2(ratio).is_integer() and np.float32(np.sqrt(np.float32(area))) == math.sqrt(area), b
            on_level += any(ratio == 2.0 ** (k - 4) for k in range(ml + 1, ml + len(scales)))
        for P in IR.ROI_POOLED:
            a, c = IR.roi_decisions(b, scales, ml, P, HWs, np.float32), IR.roi_decisions(b, scales, ml, P, HWs, np.float64)
            assert (a["level"], a["gh"], a["gw"]) == (c["level"], c["gh"], c["gw"]), (b, P)
            assert bool((a["vy"] == c["vy"]).all()) and bool((a["vx"] == c["vx"]).all()), (b, P)
            on_grid += c["gh"] > 0 and float(c["rhP"]).is_integer()
            on_H += c["gh"] > 0 and bool((c["ys"] == c["H"]).any())
            empty += c["gh"] <= 0 or c["gw"] <= 0
            outside += c["gh"] > 0 and c["gw"] > 0 and not (c["vy"].any() and c["vx"].any())
    assert on_level and on_grid and on_H and empty and outside, (on_level, on_grid, on_H, empty, outside)


def test_roi_reference_is_the_oracle_roi_pooler():
    """roi_align_ref in float64 equals oracle.ref_model.roi_align (the published algorithm as a Python loop) on double maps, with the levels of
    oracle.ref_model.assign_levels."""
    from oracle import ref_model as R
    scales, ml, HWs = IR.roi_pyramid("p3-5")
    feats = [f.double() for f in _roi_feats("p3-5", 4, 1, 0)]
    boxes = np.concatenate([IR.roi_boxes(9, 3, "p3-5")[0], np.array(IR.ROI_EXACT_BOXES[:6], dtype=np.float32)])
    for P in (1, 7):
        ref, mag, _ = IR.roi_align_ref(feats, scales, ml, P, boxes)
        lv = [IR.roi_decisions(b, scales, ml, P, HWs)["level"] for b in boxes]
        want = torch.stack([R.roi_align(feats[l][0].permute(2, 0, 1), torch.from_numpy(boxes[i:i + 1]).double(), scales[l], P)[0]
                            for i, l in enumerate(lv)])                                                         # [n, C, P, P]
        assert lv == [int(v) for v in R.assign_levels(torch.from_numpy(boxes), ml, ml + len(scales) - 1)]
        want = want.permute(0, 2, 3, 1).reshape(len(boxes), -1)
        assert float((ref - want).abs().max()) <= 1e-12 * float(want.abs().max()), P
        assert bool((mag >= ref.abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("pyramid,C,P", [("p3-5", 4, 1), ("p3-5", 16, 7), ("p2-5", 4, 4), ("p2-5", 16, 8), ("p3-5", 4, 14)])
def test_roi_emulation_within_bounds(pyramid, C, P):
    scales, ml, HWs = IR.roi_pyramid(pyramid)
    feats = _roi_feats(pyramid, C, 1, 1)
    boxes = np.concatenate([IR.roi_boxes(64, BOX_SEEDS[0], pyramid)[0][:24], np.array(IR.ROI_EXACT_BOXES, dtype=np.float32)])
    ref, mag, d = IR.roi_align_ref(feats, scales, ml, P, boxes)
    got, _, _ = IR.roi_align_ref(feats, scales, ml, P, boxes, emulate=True)
    h, r = _ratios(got, ref, mag, d)
    assert h <= 1 and r <= 1, (pyramid, C, P, h, r, d)


@pytest.mark.parametrize("fault", ["grid", "level", "yH"])
def test_roi_faults_fail(fault):
    scales, ml, HWs = IR.roi_pyramid("p3-5")
    feats = _roi_feats("p3-5", 16, 1, 2)
    gen = IR.roi_boxes(64, BOX_SEEDS[0], "p3-5")[0][:12]
    exact = np.array(IR.ROI_EXACT_BOXES, dtype=np.float32)
    for P in (1, 7):
        hit = False
        for boxes in (gen, exact):
            ref, mag, d = IR.roi_align_ref(feats, scales, ml, P, boxes)
            bad, _, _ = IR.roi_align_ref(feats, scales, ml, P, boxes, fault=fault)
            hit |= not _passes(bad, ref, mag, d)
            if fault != "yH":
                assert not _passes(bad, ref, mag, d), (fault, P)
        assert hit or P != 1, (fault, P)                 # the exact list has a sample ON y == H at P = 1
    ref, mag, d = IR.roi_align_ref(feats, scales, ml, 7, gen)
    assert not _passes(_block_error(ref, mag), ref, mag, d)


# ---- coverage --------------------------------------------------------------------------------------------------------------------
def test_every_kernel_is_accounted_for():
    names = set()
    for f in ("ore_misc.hip", "ore_roi.hip"):
        src = open(os.path.join(PKG, "csrc", f)).read()
        names |= set(re.findall(r"__global__[^;{]*?void\s+(\w+)\s*\(", src))
    assert len(names) > 20 and "k_head_pred" in names and "k_roi_align" in names
    covered = IR.covered_kernels()
    assert not (covered & set(IR.NOT_COVERED)), covered & set(IR.NOT_COVERED)
    missing = sorted(n for n in names if n not in covered and n not in IR.NOT_COVERED)
    assert not missing, f"kernels without a test: {missing}"
    stale = sorted(n for n in covered | set(IR.NOT_COVERED) if n not in names)
    assert not stale, f"the table names kernels that do not exist: {stale}"


def test_entry_points_exist_in_the_header():
    hdr = open(os.path.join(os.path.dirname(PKG), "include", "ore_hip.h")).read()
    for op, (entries, _, edges) in IR.INFER_OPS.items():
        assert edges, op
        for e in entries:
            assert re.search(r"\b%s\s*\(" % e, hdr), (op, e)
