"""float64 restatements of the inference-only non-conv kernels (csrc/ore_misc.hip, the forward of csrc/ore_roi.hip), the chain depths
of those kernels, the operands the tests feed them, and the coverage table.

As in trainops_ref.py every restatement works on NHWC tensors and returns (ref, mag): `ref` the float64 value, `mag` the SAME
expression with every operand, product and sum term replaced by its modulus (padding contributes 0 to both).  A kernel output is held
to the two checks of dgrad_ref.check with the kernel's depth d, u = 2^-24, C_S = 1:
    every element                     |got - ref| <= 2 d u mag              (an element with mag == 0 must be exact)
    every 16-row x 16-channel block   rms((got - ref) / mag) <= C_S u sqrt(d)
d is the longest chain of fp32 roundings behind one output element, read off the kernel's own summation order.

Chain depths (constant or function, kernel, derivation):
  D_STEM = 32                 k_stem1: the preprocess (x - mean) / std (2); the GEMM over K = 27 padded to 28 is 7 k-steps of
                              v_mfma_f32_16x16x4_f32, each a chain of 4 products into the accumulator (28); acc * scale + shift (2);
                              the ReLU is 1-Lipschitz.  A tap outside the H x W image is 0 AFTER the normalisation (also between H x W
                              and the padded Hp x Wp that fixes the output size), never (0 - mean) / std.
  d_ese_colsum(HW, C, P)      k_colsum_partial: part p holds rows_per = ceil(HW / P) rows (the last parts fewer or none); the 256 threads
                              are cpb = min(C / 4, 256) channel quads x rpar = 256 / cpb row lanes; a lane adds ceil(rows_per / rpar)
                              rows in one chain, lane 0 then adds the other rpar - 1 lanes in one chain.
  d_ese_gate(HW, C, P)        ese_gate16 on the P partial sums: the 1024 threads are Q4 = C / 4 quads x NSL = 1024 / Q4 slices; slice sl
                              adds the parts sl, sl + NSL, ... in one chain (the 8-way unrolled loop and its remainder loop add in the
                              same ascending order): ceil(P / NSL); the slices in one chain: min(NSL, P) (a slice beyond P holds an
                              exact 0); * (1 / HW) with the reciprocal itself rounded (2).  The dot product over C terms: lane k of
                              the wave multiplies (1) and adds ceil(C / 64) terms in one chain (the register part and the tail loop
                              past ESE_FP x 64 = 512 in the same ascending order), then 6 shuffle steps; + bias, + 3 (2); the clamp is
                              1-Lipschitz; / 6 (1).  d = ceil(P / NSL) + min(NSL, P) + 2 + 1 + ceil(C / 64) + 6 + 3.
                              ore_ese_gate_fwd (its own P = min(ceil(HW / 32), 512)): d_ese_colsum + d_ese_gate.
                              The scaled weight columns (ese_scale_columns) and k_scale_channels are single products: bit for bit
                              against the fp32 product with the kernel's own gate.
  d_support(s)                k_support_kernels: lane i of the 64 adds the pixels i, i + 64, ... of its windows in one chain,
                              ceil(s^2 / 64); 6 shuffle steps; the division (1).
  D_CORR_FWD (trainops_ref)   k_correlation computes, expression for expression, the attention half of k_corr_fwd_train:
                              a + relu(conv3x1(relu(conv1x3(q)))) + q with a = relu(k11 relu(k11 q)); the restatement is
                              trainops_ref.corr_fwd, its first C channels.
  d_gn_stats (trainops_ref)   the multi-level statistics run k_gn_chunk_stats / k_gn_chunk_stats4 and k_gn_combine per (level, image)
                              segment; the depth is trainops_ref.d_gn_stats with the segment's own row count.
  D_HEAD = 50                 k_head_pred: the staged value x * mul + add (2), the ReLU is 1-Lipschitz, zero padding is applied AFTER
                              it; thread (quad q, row r) runs ONE fma chain per (pixel, output) over its 9 taps x 4 channels (36);
                              the 32 quads go into four chains s0..s3 of 8 additions (8), (s0 + s1) + (s2 + s3) (2);
                              * scale + shift (2).  The ReLU applies to outputs 0..3 only.
  d_roi(gh, gw)               k_roi_align, per sample: hy = 1 - ly (1; ly = y - floor(y) is exact), a weight product such as
                              hy * hx (1), the weighted value (1), three additions (3): 6; the gh * gw samples of a bin in one chain
                              (gh * gw), / cnt (1).  d = 6 + gh * gw + 1 with the largest grid among the boxes.
  C_ROI_COORD = 8             the coordinate term of ROIAlign.  y = y0 + ph * bh + (iy + 0.5) * bh / gh with y0 = b.y * sc - 0.5
                              (sc a power of two: the product is exact; the subtraction rounds: 1, likewise y1), rh = y1 - y0 (1),
                              bh = rh / P (1), ph * bh (1), (iy + 0.5) * bh (1), / gh (1), two additions (2).  y = (1 - f) y0 + f y1
                              with f in [0, 1], so the roundings of y0 and y1 contribute at most u (|y| + 1) (every box the tests
                              compare starts at y0 >= -1, so the partial sums grow from y0 to y, or it has no valid sample); the
                              roundings on the way to f * rh are 4 relative roundings (rh, bh, the product, / gh) of a term of at
                              most |y| + 1, the two additions 2 more: 7 u (|y| + 1),
                              stated as c = 8 with the second-order terms (contracting the products to fma removes roundings, it adds
                              none).  Bilinear interpolation is continuous and piecewise linear in (y, x): across a cell border and into
                              the border clamp alike, with slope at most the sum of absolute differences of the four corner values.
                              A sample's value is therefore off by at most  E = c u (|y| + |x| + 1) * D,  D = |v1 - v2| + |v3 - v4| +
                              |v1 - v3| + |v2 - v4|, on top of the roundings counted in d.  Both checks are relative to mag times a
                              multiple of u (2 d u and C_S u sqrt(d)), so E enters mag divided by the SMALLER of those factors:
                                  mag gains  c (|y| + |x| + 1) D / sqrt(d)  per sample,
                              which admits exactly E in the rms check (coordinate errors are shared by the channels and bins of a
                              block, they do not average out) and at most 2 sqrt(d) E in the element check.  (Adding c u (..) D to
                              mag itself would make the term second order in u: at |y| ~ 40 the coordinate error is ~50 times the
                              value roundings, and the fp32 emulation of tests/test_inferops_host.py then exceeds both bounds 7 to
                              16 times at pooled 7, 8 and 14.)
Exact ops (torch.equal): k_maxpool against the float64 max (trainops_ref.maxpool_fwd); with the gate, against the fp32 product of
that max with the gate (the gate is >= 0 and fl(x * s) is monotone in x, so max fl(x_i s) == fl(max(x_i) s)).

bf16 storage.  ld4 / st4 of ore_common.h: ld4(ore_bf16_t*) widens by shifting the 16 bits into the top of an fp32 (exact),
st4(ore_bf16_t*) goes through to_bf16x4 = __builtin_convertvector(f32x2 -> bf16x2), the hardware's round-to-nearest-even conversion.
k_stem1<T, NT, TO>, k_maxpool<TS>, k_correlation<TS>, k_head_pred<TS>, k_roi_align<TS> and k_gn_chunk_stats4<8, TS> differ from their
fp32 builds in these two helpers only, so a bf16 build must equal the fp32 build on the up-cast values bit for bit (after bf16_rne of
the result where the output is bf16); the fp32 build is what the float64 bound pins.

ROIAlign's discrete decisions (the level: floor(4 + log2(sqrt(area) / 224 + 1e-8)); the grid: ceil(rh / P), ceil(rw / P); validity:
y < -1 or y > H) are taken in float64 from the fp32 box values; roi_boxes() only hands out boxes that keep a relative margin of
ROI_MARGIN = 1e-4 from every level threshold, every integer of rh / P and rw / P and both validity limits at every sample
(roi_margins(); a box that fails is re-drawn from the next seed), so that fp32 and float64 agree on them; ROI_EXACT_BOXES have
coordinates in 1/8 px and power-of-two size ratios, so their decisions are exact in fp32 and sit on the boundaries.

Test infrastructure (used by tests/ only)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import trainops_ref as TR
from trainops_ref import (C_S, D_CORR_FWD, U, bf16_rne, check, check2, d_gn_stats, gn_inputs, gn_stats,  # noqa: F401  (re-exported)
                          gn_stats_kernel, scaled_inputs)

F64 = torch.float64
_cdiv = TR._cdiv

# ---- chain depths ----------------------------------------------------------------------------------------------------------------
D_STEM, D_HEAD, C_ROI_COORD = 32, 50, 8
ESE_T, ESE_PARTS = 1024, 512


def ese_plan_P(HW):
    """P of ore_ese_gate_fwd."""
    return min(_cdiv(HW, 32), ESE_PARTS)


def d_ese_colsum(HW, C, P):
    cpb = min(C // 4, 256)
    rpar = 256 // cpb
    return _cdiv(_cdiv(HW, P), rpar) + rpar - 1


def d_ese_gate(HW, C, P):
    nsl = ESE_T // (C // 4)
    return _cdiv(P, nsl) + min(nsl, P) + 2 + 1 + _cdiv(C, 64) + 6 + 3


def d_support(s):
    return _cdiv(s * s, 64) + 6 + 1


def d_roi(gh, gw):
    return 6 + max(gh * gw, 1) + 1


def _conv(x, w, stride=1, padding=0):
    """F.conv2d as im2col + matmul (float64 on any device): x [B,Ci,H,W], w [Co,Ci,k,k] -> [B,Co,Ho,Wo]."""
    B, _, H, W = x.shape
    Co, _, k, _ = w.shape
    Ho, Wo = (H + 2 * padding - k) // stride + 1, (W + 2 * padding - k) // stride + 1
    cols = F.unfold(x, k, padding=padding, stride=stride)                  # [B, Ci * k * k, Ho * Wo]
    return (w.reshape(1, Co, -1) @ cols).reshape(B, Co, Ho, Wo)


# ---- stem ------------------------------------------------------------------------------------------------------------------------
def stem_inputs(B, H, W, Cout, u8, seed, device="cpu"):
    """(img [B,3,H,W] u8 or fp32 planar, mean3, std3 (python floats), w [Cout,3,3,3], scale, shift [Cout]): pixel values in
    [0, 255], the detector's BGR statistics, weights with per-output-channel scales 10^U(-3, 3), FrozenBN scale / shift of mixed sign
    (roughly half of the outputs survive the ReLU)."""
    g = torch.Generator(device=device).manual_seed(seed)
    f64 = dict(generator=g, dtype=F64, device=device)
    img = torch.rand(B, 3, H, W, **f64) * 255.0
    img = img.round().to(torch.uint8) if u8 else img.float()
    mean, std = [103.53, 116.28, 123.675], [57.375, 57.12, 58.395]
    sc = 10.0 ** (torch.rand(Cout, **f64) * 6 - 3)
    w = (torch.randn(Cout, 3, 3, 3, **f64) * sc.view(-1, 1, 1, 1) / math.sqrt(27.0)).float()
    scale = (torch.randn(Cout, **f64) * 10.0 ** (torch.rand(Cout, **f64) * 2 - 1)).float()
    shift = (torch.randn(Cout, **f64) * sc * 0.3).float()
    return img.contiguous(), mean, std, w.contiguous(), scale, shift


def stem_ref(img, Hp, Wp, mean, std, w, scale, shift, device=None, images=None, fault=None):
    """ore_stem1_fwd (d2z:modeling/backbone/vovnet.py stem_1 behind the model's normaliser): relu(conv3x3 s2 p1 over the zero-padded
    (x - mean) / std, * scale + shift) -> [B, Hp / 2, Wp / 2, Cout].  images: these batch indices only.
    fault (tests/test_inferops_host.py): "tap26" drops the last tap, "channel" normalises tap (c = 1, ky = 1, kx = 1) with channel 0's
    mean / std, "pad" pads with (0 - mean) / std."""
    dev = device or img.device
    x = (img if images is None else img[images]).to(dev).double()
    B, _, H, W = x.shape
    f32 = lambda v: torch.tensor(v, dtype=torch.float32, device=dev).double().view(1, 3, 1, 1)      # noqa: E731  (the kernel's fp32 arguments)
    m, s = f32(mean), f32(std)
    wd, sc, sh = w.to(dev).double(), scale.to(dev).double().view(1, -1, 1, 1), shift.to(dev).double().view(1, -1, 1, 1)
    a, am = (x - m) / s, (x.abs() + m.abs()) / s.abs()
    pad = lambda t, v: F.pad(t, (0, Wp - W, 0, Hp - H), value=v)                                      # noqa: E731
    if fault == "pad":
        full = ((torch.zeros(B, 3, Hp + 2, Wp + 2, dtype=F64, device=dev) - m) / s)
        full[:, :, 1:1 + H, 1:1 + W] = a
        acc = _conv(full, wd, stride=2)
    else:
        acc = _conv(pad(a, 0.0), wd, stride=2, padding=1)
        if fault == "tap26":
            w1 = torch.zeros_like(wd)
            w1[:, 2, 2, 2] = wd[:, 2, 2, 2]
            acc = acc - _conv(pad(a, 0.0), w1, stride=2, padding=1)
        if fault == "channel":
            w1 = torch.zeros_like(wd)
            w1[:, 1, 1, 1] = wd[:, 1, 1, 1]
            wrong = a.clone()
            wrong[:, 1] = (x[:, 1] - m[0, 0]) / s[0, 0]
            acc = acc + _conv(pad(wrong - a, 0.0), w1, stride=2, padding=1)
    mag = _conv(pad(am, 0.0), wd.abs(), stride=2, padding=1) * sc.abs() + sh.abs()
    ref = (acc * sc + sh).clamp(min=0)
    return ref.permute(0, 2, 3, 1).contiguous(), mag.permute(0, 2, 3, 1).contiguous()


# ---- eSE -------------------------------------------------------------------------------------------------------------------------
def ese_gate_ref(x, fc_w, fc_b, device=None):
    """ore_ese_gate_fwd (d2z:modeling/backbone/vovnet.py:238-260): x [B,HW,C] -> gate = relu6(fc(mean_hw(x)) + 3) / 6, [B, C];
    -> (ref, mag, z) with z the float64 pre-activations (for the knee margin)."""
    B, HW, C = x.shape
    o = TR.ese_node(x.reshape(B, 1, HW, C), fc_w, fc_b, device=device)
    z = o["z"]
    zm = TR._d(fc_b, device).abs() + o["m"][1] @ TR._d(fc_w, device).reshape(C, C).abs().t()
    return (z / 6 + 0.5).clamp(0, 1), zm / 6 + 0.5, z


def ese_gate_from_parts_ref(part, HW, fc_w, fc_b, device=None, HW_div=None, parts=None):
    """ore_ese_gate_from_colsum_fwd and the scaled-weight / pool forms: part [B,P,C] fp32 partial column sums (given inputs) ->
    (ref, mag, z).  HW_div: divide by this instead of HW; parts: count these parts only (faults for tests/test_inferops_host.py)."""
    p = TR._d(part, device)
    if parts is not None:
        p = p[:, parts]
    C = p.shape[-1]
    Wm, b = TR._d(fc_w, device).reshape(C, C), TR._d(fc_b, device)
    n = float(HW_div or HW)
    m, mm = p.sum(1) / n, p.abs().sum(1) / n
    z, zm = b + m @ Wm.t(), b.abs() + mm @ Wm.abs().t()
    return (z / 6 + 0.5).clamp(0, 1), zm / 6 + 0.5, z


def ese_parts_inputs(B, P, HW, C, seed, device="cpu", empty_from=None):
    """(part [B,P,C], fc_w [C,C], fc_b [C]) fp32: partial sums of a map with per-channel scales 10^U(-3, 3) and per-image scales, a mean
    offset of one standard deviation, parts from `empty_from` on exactly 0 (P > HW: the parts beyond the rows hold nothing); fc_w
    undoes the channel scales so that every pre-activation is O(1), and the bias is nudged off the hard-sigmoid knees as in
    trainops_ref.ese_inputs."""
    g = torch.Generator(device=device).manual_seed(seed)
    f64 = dict(generator=g, dtype=F64, device=device)
    sc = 10.0 ** (torch.rand(C, **f64) * 6 - 3)
    si = 10.0 ** (torch.rand(B, **f64) * 2 - 1)
    rows = max(HW / P, 1.0)
    part = ((torch.randn(B, P, C, **f64) * math.sqrt(rows) + rows) * sc * si.view(B, 1, 1)).float()
    if empty_from is not None:
        part[:, empty_from:] = 0.0
    w = (2.0 * torch.randn(C, C, **f64) / (math.sqrt(C) * sc.view(1, C))).float()
    b = (torch.rand(C, **f64) * 6 - 3).float()
    for _ in range(200):
        z = ese_gate_from_parts_ref(part, HW, w, b)[2]
        bad = ((z.abs() - 3.0).abs() < 2 * TR.ESE_KNEE_MARGIN).any(0)
        if not bool(bad.any()):
            break
        b = torch.where(bad, b + 5 * TR.ESE_KNEE_MARGIN, b)
    return part, w, b


# ---- correlation, support kernels ---------------------------------------------------------------------------------------------------
def corr_infer_ref(q, k11, k13, k31, device=None, wrap=None):
    """ore_correlation_fwd (ref:fewx/modeling/fsod/fsod_cen.py:229-245, the attention): q [B,H,W,C], k11 [C], k13 / k31 [C,3] ->
    a + relu(conv3x1(relu(conv1x3(q)))) + q.  The expression is the training forward's: its restatement, first C channels."""
    C = q.shape[-1]
    ref, mag = TR.corr_fwd(q, k11, k13, k31, device=device, wrap=wrap)["cat"]
    return ref[..., :C], mag[..., :C]


def corr_levels_ref(q_rows, B, levels, k11, k13, k31, device=None):
    """ore_correlation_levels_fwd: q_rows [sum_l B H_l W_l, C] level-major, k11 [L,C], k13 / k31 [L,C,3] -> rows of the same layout."""
    C = q_rows.shape[-1]
    refs, mags, r0 = [], [], 0
    for l, (H, W) in enumerate(levels):
        n = B * H * W
        r, m = corr_infer_ref(q_rows[r0:r0 + n].reshape(B, H, W, C), k11[l], k13[l], k31[l], device=device)
        refs.append(r.reshape(n, C)); mags.append(m.reshape(n, C))
        r0 += n
    return torch.cat(refs), torch.cat(mags)


def support_kernels_ref(proto, device=None):
    """ore_support_kernels_fwd (ref fsod_cen.py:214-231): proto [C,s,s] -> k11 [C], k13 [C,3] (adaptive pool to 1 x 3: column windows
    over all rows), k31 [C,3] (3 x 1: row windows); window j of an axis of length s is [floor(j s / 3), ceil((j + 1) s / 3)).
    -> {"k11", "k13", "k31"}: (ref, mag) each, in the kernel's output layouts."""
    C, s, _ = proto.shape
    x = proto.permute(1, 2, 0).unsqueeze(0)                               # [1, s, s, C]
    out = {}
    for name, (oh, ow) in (("k11", (1, 1)), ("k13", (1, 3)), ("k31", (3, 1))):
        r, m = TR.apool_fwd(x, oh, ow, device=device)                     # [1, oh, ow, C]
        out[name] = tuple(t.reshape(oh * ow, C).t().reshape(C) if oh * ow == 1 else t.reshape(oh * ow, C).t().contiguous() for t in (r, m))
    return out


# ---- GroupNorm statistics of several levels ----------------------------------------------------------------------------------------
def gn_levels_ref(x_rows, B, HWs, G, eps, gamma, beta, device=None):
    """ore_groupnorm_affine_levels_fwd: x_rows [sum_l B HW_l, C] level-major -> mul, add [L * B, C] (segment = level * B + image):
    mul = rstd * gamma, add = beta - mean * mul.  -> (mul_ref, mul_mag), (add_ref, add_mag)."""
    C = x_rows.shape[-1]
    ga, be = TR._d(gamma, device), TR._d(beta, device)
    mr, mm, ar, am, r0 = [], [], [], [], 0
    for hw in HWs:
        (r, rm), (a, amag) = gn_stats(x_rows[r0:r0 + B * hw].reshape(B, hw, C), G, eps, device=device)
        mr.append(r * ga); mm.append(rm * ga.abs())
        ar.append(be + a * ga); am.append(be.abs() + amag * ga.abs())
        r0 += B * hw
    return (torch.cat(mr), torch.cat(mm)), (torch.cat(ar), torch.cat(am))


# ---- CenterNet head, last step -----------------------------------------------------------------------------------------------------
def head_inputs(B, levels, seed, device="cpu", ep_stride=16):
    """(tower [rows,128] level-major, mul, add [L * B,128], w5 [5,128,3,3], scale, shift [L, ep_stride]): the tower with per-channel
    and per-image scales, mul undoing the channel scale up to 10^U(-1, 1) and add of the staged value's size and mixed sign (so that
    relu(add) != 0: a halo left un-zeroed shows), so the staged values are O(1) to O(10) in every channel as behind a GroupNorm;
    weights with per-OUTPUT scales 10^U(-3, 3) and mild per-input scales 10^U(-0.5, 0.5) (every quad of input channels carries a
    visible share of every output); distinct per-level epilogue rows, the columns from 5 on NaN."""
    g = torch.Generator(device=device).manual_seed(seed)
    f64 = dict(generator=g, dtype=F64, device=device)
    C, L = 128, len(levels)
    rows = sum(B * h * w for h, w in levels)
    sc = 10.0 ** (torch.rand(C, **f64) * 6 - 3)
    seg = 10.0 ** (torch.rand(L * B, 1, **f64) * 2 - 1)
    tower = torch.empty(rows, C, dtype=F64, device=device)
    r0 = 0
    for l, (h, w) in enumerate(levels):
        for b in range(B):
            tower[r0:r0 + h * w] = torch.randn(h * w, C, **f64) * sc * seg[l * B + b]
            r0 += h * w
    mul = 10.0 ** (torch.rand(L * B, C, **f64) * 2 - 1) / (sc * seg) * torch.where(torch.rand(L * B, C, **f64) < 0.5, -1.0, 1.0)
    add = torch.randn(L * B, C, **f64) * 10.0 ** (torch.rand(L * B, C, **f64) * 2 - 1)
    so, si = 10.0 ** (torch.rand(5, **f64) * 6 - 3), 10.0 ** (torch.rand(C, **f64) - 0.5)
    w5 = torch.randn(5, C, 3, 3, **f64) * so.view(5, 1, 1, 1) * si.view(1, C, 1, 1) / math.sqrt(9.0 * C)
    scale = torch.full((L, ep_stride), float("nan"), dtype=F64, device=device)
    shift = torch.full((L, ep_stride), float("nan"), dtype=F64, device=device)
    scale[:, :5] = torch.randn(L, 5, **f64) * 10.0 ** (torch.rand(L, 5, **f64) * 2 - 1)
    shift[:, :5] = torch.randn(L, 5, **f64) * so * 3.0
    return tuple(t.float().contiguous() for t in (tower, mul, add, w5, scale, shift))


def head_ref(tower, B, levels, mul, add, w5, scale, shift, device=None, fault=None):
    """ore_head_pred_fwd (ref:CenterNet2/centernet/modeling/dense_heads/centernet_head.py:150-159 on the folded GroupNorm affine):
    t = relu(x * mul + add), zero-padded; v = conv3x3_{128 -> 5}(t) * scale_l + shift_l; relu on outputs 0..3 -> [rows, 5].
    fault (tests/test_inferops_host.py): "halo": the padding is relu(add) instead of 0; "stride5": level l reads its epilogue at
    l * 5 of the flattened table."""
    C = tower.shape[-1]
    wd = TR._d(w5, device)
    refs, mags, r0 = [], [], 0
    scf, shf = TR._d(scale, device).reshape(-1), TR._d(shift, device).reshape(-1)
    eps_ = scale.shape[1]
    for l, (H, W) in enumerate(levels):
        n = B * H * W
        x = TR._d(tower[r0:r0 + n], device).reshape(B, H * W, C)
        m, a = TR._d(mul[l * B:(l + 1) * B], device).view(B, 1, C), TR._d(add[l * B:(l + 1) * B], device).view(B, 1, C)
        t, tm = (x * m + a).clamp(min=0), (x * m).abs() + a.abs()
        nchw = lambda v: v.reshape(B, H, W, C).permute(0, 3, 1, 2)                     # noqa: E731
        if fault == "halo":
            tp = a.clamp(min=0).view(B, C, 1, 1).expand(B, C, H + 2, W + 2).clone()
            tp[:, :, 1:-1, 1:-1] = nchw(t)
            acc = _conv(tp, wd)
        else:
            acc = _conv(nchw(t), wd, padding=1)
        am = _conv(nchw(tm), wd.abs(), padding=1)
        e0 = l * (5 if fault == "stride5" else eps_)
        sc, sh = scf[e0:e0 + 5].view(1, 5, 1, 1), shf[e0:e0 + 5].view(1, 5, 1, 1)
        v, vm = acc * sc + sh, am * sc.abs() + sh.abs()
        v = torch.cat([v[:, :4].clamp(min=0), v[:, 4:]], 1)
        refs.append(v.permute(0, 2, 3, 1).reshape(n, 5)); mags.append(vm.permute(0, 2, 3, 1).reshape(n, 5))
        r0 += n
    return torch.cat(refs), torch.cat(mags)


# ---- ROIAlign ------------------------------------------------------------------------------------------------------------------------
ROI_MARGIN = 1e-4
CANONICAL_SIZE, CANONICAL_LEVEL = 224.0, 4


def roi_decisions(box, scales, min_level, P, HWs, dtype=np.float64):
    """The discrete decisions of k_roi_align for one box (4 values, taken as given fp32 numbers) evaluated in `dtype` arithmetic with
    correctly rounded operations (numpy float32 / float64: +, -, *, /, sqrt; log2 is only ever needed at the thresholds, see
    roi_margins) -> dict(level, gh, gw, valid [gh*P] / [gw*P] bools per sample coordinate, ys, xs sample coordinates, and the
    quantities the margins are measured on)."""
    t = dtype
    b = [t(v) for v in np.asarray(box, dtype=np.float32)]
    with np.errstate(invalid="ignore"):
        size = np.sqrt((b[2] - b[0]) * (b[3] - b[1]))
    ratio = size / t(CANONICAL_SIZE) + t(np.float32(1e-8))
    L = len(scales)
    # floor(4 + log2(ratio)) clamped == the number of thresholds 2^(k - 4), k = min_level + 1 .. min_level + L - 1, at or below ratio
    # (2^(k-4) is exact in either type, and so is the comparison: no log2 is evaluated)
    lvl = sum(1 for k in range(min_level + 1, min_level + L) if ratio >= t(2.0 ** (k - CANONICAL_LEVEL)))
    if not np.isfinite(ratio):
        lvl = 0                                                # sqrt of a negative area: NaN -> fmaxf / fminf pick the lower clamp
    sc = t(np.float32(scales[lvl]))
    H, W = HWs[lvl]
    x0, y0, x1, y1 = b[0] * sc - t(0.5), b[1] * sc - t(0.5), b[2] * sc - t(0.5), b[3] * sc - t(0.5)
    rw, rh = x1 - x0, y1 - y0
    bw, bh = rw / t(P), rh / t(P)
    gh, gw = int(np.ceil(rh / t(P))), int(np.ceil(rw / t(P)))
    ys = np.array([y0 + t(ph) * bh + (t(iy) + t(0.5)) * bh / t(gh) for ph in range(P) for iy in range(max(gh, 0))], dtype=t)
    xs = np.array([x0 + t(pw) * bw + (t(ix) + t(0.5)) * bw / t(gw) for pw in range(P) for ix in range(max(gw, 0))], dtype=t)
    return dict(level=lvl, gh=gh, gw=gw, ys=ys, xs=xs, vy=~((ys < -1) | (ys > H)), vx=~((xs < -1) | (xs > W)), ratio=ratio,
                rhP=rh / t(P), rwP=rw / t(P), H=H, W=W)


def roi_margins(box, scales, min_level, P, HWs):
    """The smallest relative distance of the float64 decisions of `box` from a discontinuity: level thresholds (on the size ratio),
    integers of rh / P and rw / P, the validity limits -1 and H (W) at every sample coordinate (relative to max(|limit|, 1))."""
    d = roi_decisions(box, scales, min_level, P, HWs)
    L = len(scales)
    m = min([abs(d["ratio"] / 2.0 ** (k - CANONICAL_LEVEL) - 1.0) for k in range(min_level + 1, min_level + L)] or [1.0])
    for v in (d["rhP"], d["rwP"]):
        n = round(float(v))
        m = min(m, abs(float(v) - n) / max(abs(n), 1.0))
    for vs, lim in ((d["ys"], d["H"]), (d["xs"], d["W"])):
        if len(vs):
            m = min(m, float(np.abs(vs + 1.0).min()), float(np.abs(vs - lim).min()) / lim)
    return float(m)


ROI_POOLED = (1, 4, 7, 8, 14)
ROI_PYRAMIDS = {"p3-5": dict(strides=(8, 16, 32), min_level=3), "p2-5": dict(strides=(4, 8, 16, 32), min_level=2)}
ROI_IMAGE = 320


def roi_pyramid(name):
    p = ROI_PYRAMIDS[name]
    return [1.0 / s for s in p["strides"]], p["min_level"], [(ROI_IMAGE // s, ROI_IMAGE // s) for s in p["strides"]]


def roi_boxes(n, seed, pyramid):
    """n fp32 boxes, box i aimed at level i % L of the pyramid (sizes log-uniform within the level's range, aspect ratios in
    [1/2, 2]): inside the ROI_IMAGE square, except that the top level takes sqrt(area) >= 448, so its boxes start inside the image
    and end beyond it (some of their samples are invalid).  Every box starts at x0, y0 >= 0.  Each keeps ROI_MARGIN at EVERY pooled size of ROI_POOLED; a box that fails a margin is
    re-drawn from the next seed (never dropped): -> (boxes [n,4] float32 numpy, the seeds used)."""
    scales, min_level, HWs = roi_pyramid(pyramid)
    L = len(scales)
    out, seeds = [], []
    s = seed * 100003
    for i in range(n):
        lvl = i % L
        while True:
            rng = np.random.default_rng(s)
            s += 1
            top = lvl == L - 1
            lo = 8.0 if lvl == 0 else CANONICAL_SIZE * 2.0 ** (min_level + lvl - CANONICAL_LEVEL)
            hi = 640.0 if top else min(300.0, CANONICAL_SIZE * 2.0 ** (min_level + lvl + 1 - CANONICAL_LEVEL))
            size = math.exp(rng.uniform(math.log(lo), math.log(hi)))
            ar = 2.0 ** rng.uniform(-1, 1)
            w, h = size * math.sqrt(ar), size / math.sqrt(ar)
            if top:                                              # larger than the image: starts inside it, ends beyond
                x0, y0 = rng.uniform(0, 40), rng.uniform(0, 40)
            else:
                w, h = min(w, ROI_IMAGE), min(h, ROI_IMAGE)
                x0, y0 = rng.uniform(0, ROI_IMAGE - w), rng.uniform(0, ROI_IMAGE - h)
            box = np.array([x0, y0, x0 + w, y0 + h], dtype=np.float32)
            if all(roi_margins(box, scales, min_level, P, HWs) >= ROI_MARGIN for P in ROI_POOLED):
                break
        out.append(box); seeds.append(s - 1)
    return np.stack(out), seeds


# coordinates in 1/8 px, size ratios sqrt(area) / 224 in {1/4, 1/2, 1, 2}: sqrt, the division, the level thresholds and (for the
# power-of-two pooled sizes) the grid are exact in fp32 and sit ON their boundaries
ROI_EXACT_BOXES = [
    (0.0, 0.0, 448.0, 448.0),           # ratio 2: exactly the top threshold -> top level; reaches beyond the image
    (0.0, 0.0, 224.0, 224.0),           # ratio 1: threshold of level 4 -> level 4
    (48.0, 100.0, 272.0, 156.0),        # 224 x 56: ratio 1/2, threshold of level 3
    (16.0, 16.0, 128.0, 128.0),         # 112 x 112: ratio 1/2 again, rh / P integer at P in {1, 7, 14} (stride 8: 14 cells)
    (60.0, 312.0, 256.0, 328.0),        # 196 x 16: ratio 1/4; at stride 8 and P = 1 the second sample row is y == H exactly (valid)
    (32.0, 64.0, 81.0, 128.0),          # 49 x 64: ratio 1/4; rh / P = 8 / P exactly integer at P in {1, 4, 8} (stride 8)
    (100.0, 100.0, 100.0, 180.0),       # zero width: gw = 0, count 1, output 0
    (100.0, 100.0, 180.0, 100.0),       # zero height
    (200.0, 200.0, 144.0, 144.0),       # inverted in both axes (positive area, negative extents): gh, gw <= 0, output 0
    (200.0, 40.0, 120.0, 120.0),        # inverted in x only: negative area, the level falls to the lowest; output 0
    (400.0, 400.0, 456.0, 456.0),       # wholly outside the image, beyond the validity limit: output 0
    (-120.0, -120.0, -64.0, -64.0),     # wholly outside on the other side
    (-4.0, 8.0, 60.0, 57.0),            # 64 x 49: ratio 1/4; x0 = -1 at stride 8: samples between -1 and 0 clamp to column 0
]


def roi_align_ref(feats, scales, min_level, P, boxes, bidx=None, device=None, fault=None, emulate=False):
    """ore_roi_align_fwd (ROIPooler + ROIAlignV2, d2z:modeling/poolers.py:47-58, layers/roi_align.py aligned=True, sampling_ratio 0):
    feats[l] [B,H_l,W_l,C], boxes [n,4] fp32, bidx [n] image per box -> (ref, mag, d) with ref / mag [n, P * P * C] and d the depth for
    the largest sample grid among the boxes.  The decisions come from roi_decisions in float64.
    fault (tests/test_inferops_host.py): "grid": gh + 1 sample rows; "level": the level one too high where there is one;
    "yH": a sample at y == H (x == W) counts as invalid.  emulate: the same expressions in the kernel's order with fp32 decisions,
    coordinates, weights and sums (the fp32 emulation of tests/test_inferops_host.py; mag is not meaningful then)."""
    dev = device or feats[0].device
    T, npT = (torch.float32, np.float32) if emulate else (F64, np.float64)
    C = feats[0].shape[-1]
    HWs = [(f.shape[1], f.shape[2]) for f in feats]
    fd = [f.to(dev, T) for f in feats]
    bx = np.asarray(boxes.detach().cpu().numpy() if torch.is_tensor(boxes) else boxes, dtype=np.float32)
    n = bx.shape[0]
    ref = torch.zeros(n, P * P, C, dtype=T, device=dev)
    mag, magc = torch.zeros_like(ref), torch.zeros_like(ref)
    dmax = d_roi(1, 1)
    for r in range(n):
        if fault == "level":
            d0 = roi_decisions(bx[r], scales, min_level, P, HWs, npT)
            lv = min(d0["level"] + 1, len(scales) - 1)
            d = roi_decisions(bx[r], [scales[lv]] * len(scales), min_level, P, [HWs[lv]] * len(scales), npT)
            d["level"] = lv
        else:
            d = roi_decisions(bx[r], scales, min_level, P, HWs, npT)
        gh, gw = d["gh"], d["gw"]
        cnt = float(max(gh * gw, 1))
        if fault == "grid":
            b = [np.float64(v) for v in bx[r]]
            sc = np.float64(np.float32(scales[d["level"]]))
            y0, bh = b[1] * sc - 0.5, (b[3] - b[1]) * sc / P
            gh = gh + 1
            d["ys"] = np.array([y0 + ph * bh + (iy + 0.5) * bh / gh for ph in range(P) for iy in range(max(gh, 0))])
            H = d["H"]
            d["vy"] = ~((d["ys"] < -1) | (d["ys"] > H))
            cnt = float(max(gh * gw, 1))
        if gh <= 0 or gw <= 0:
            continue
        dmax = max(dmax, d_roi(gh, gw))
        H, W = d["H"], d["W"]
        f = fd[d["level"]][int(bidx[r]) if bidx is not None else 0]                     # [H, W, C]

        def axis(vs, valid, Ln, g):
            v = torch.tensor(np.asarray(vs, dtype=npT), device=dev)
            ok = torch.tensor(np.asarray(valid), device=dev)
            if fault == "yH":
                ok = ok & (v != Ln)
            raw = v.abs()
            v = v.clamp(min=0)
            lo = v.floor().clamp(max=Ln - 1).long()
            hi = (lo + 1).clamp(max=Ln - 1)
            v = torch.where(lo >= Ln - 1, lo.to(T), v)
            fr = v - lo.to(T)
            return lo.view(P, g), hi.view(P, g), fr.view(P, g), ok.view(P, g), raw.view(P, g)
        yl, yh, ly, oky, ya = axis(d["ys"], d["vy"], H, gh)
        xl, xh, lx, okx, xa = axis(d["xs"], d["vx"], W, gw)
        if not emulate:                                         # all samples of all bins at once (the order of a float64 sum is immaterial)
            fy = lambda t: t.reshape(P * gh, 1, 1)              # noqa: E731
            fx = lambda t: t.reshape(1, P * gw, 1)              # noqa: E731
            ok = (fy(oky) & fx(okx)).to(T)
            a_, b_ = fy(ly), fx(lx)
            yl_, yh_, xl_, xh_ = yl.reshape(-1), yh.reshape(-1), xl.reshape(-1), xh.reshape(-1)
            v1, v2, v3, v4 = f[yl_][:, xl_], f[yl_][:, xh_], f[yh_][:, xl_], f[yh_][:, xh_]
            w1, w2, w3, w4 = (1 - a_) * (1 - b_), (1 - a_) * b_, a_ * (1 - b_), a_ * b_
            bins = lambda t: t.reshape(P, gh, P, gw, C).sum((1, 3))      # noqa: E731
            acc = bins(ok * (w1 * v1 + w2 * v2 + w3 * v3 + w4 * v4))
            am = bins(ok * (w1 * v1.abs() + w2 * v2.abs() + w3 * v3.abs() + w4 * v4.abs()))
            coord = C_ROI_COORD * (fy(ya) + fx(xa) + 1.0)
            amc = bins(ok * coord * ((v1 - v2).abs() + (v3 - v4).abs() + (v1 - v3).abs() + (v2 - v4).abs()))
            ref[r], mag[r], magc[r] = (acc / cnt).reshape(P * P, C), (am / cnt).reshape(P * P, C), (amc / cnt).reshape(P * P, C)
            continue
        acc = torch.zeros(P, P, C, dtype=T, device=dev)
        am, amc = torch.zeros_like(acc), torch.zeros_like(acc)
        for iy in range(gh):
            for ix in range(gw):
                ok = (oky[:, iy].view(P, 1) & okx[:, ix].view(1, P)).to(T).unsqueeze(-1)
                a_, b_ = ly[:, iy].view(P, 1, 1), lx[:, ix].view(1, P, 1)
                v1 = f[yl[:, iy]][:, xl[:, ix]]; v2 = f[yl[:, iy]][:, xh[:, ix]]
                v3 = f[yh[:, iy]][:, xl[:, ix]]; v4 = f[yh[:, iy]][:, xh[:, ix]]
                w1, w2, w3, w4 = (1 - a_) * (1 - b_), (1 - a_) * b_, a_ * (1 - b_), a_ * b_
                acc += ok * (w1 * v1 + w2 * v2 + w3 * v3 + w4 * v4)
                coord = C_ROI_COORD * (ya[:, iy].view(P, 1, 1) + xa[:, ix].view(1, P, 1) + 1.0)
                diffs = (v1 - v2).abs() + (v3 - v4).abs() + (v1 - v3).abs() + (v2 - v4).abs()
                am += ok * (w1 * v1.abs() + w2 * v2.abs() + w3 * v3.abs() + w4 * v4.abs())
                amc += ok * coord * diffs
        ref[r], mag[r], magc[r] = (acc / cnt).reshape(P * P, C), (am / cnt).reshape(P * P, C), (amc / cnt).reshape(P * P, C)
    mag = mag + magc / math.sqrt(dmax)
    return ref.reshape(n, P * P * C), mag.reshape(n, P * P * C), dmax


# ---- coverage --------------------------------------------------------------------------------------------------------------------
# op -> (C-ABI entry points, kernels, edge classes); tests/test_hip_inferops.py runs every entry point at every edge class and
# tests/test_inferops_host.py accounts for every __global__ of csrc/ore_misc.hip and every forward kernel of csrc/ore_roi.hip
STEM_CASES = [  # (B, H, W, Hp, Wp, Cout)
    (1, 75, 100, 76, 100, 16), (1, 75, 100, 76, 100, 32), (1, 75, 100, 76, 100, 64), (1, 75, 100, 76, 100, 128),
    (2, 1, 37, 2, 38, 64), (3, 5, 1, 6, 2, 64), (1, 33, 31, 34, 32, 64), (1, 3, 3, 4, 4, 64), (1, 5, 13, 6, 14, 64),
    (1, 20, 24, 64, 64, 64), (2, 9, 661, 10, 662, 64), (1, 5, 5, 6, 6, 64),
]   # output widths Wo: 50, 19, 1, 16, 2, 7, 32, 331, 3
MAXPOOL_CASES = [(2, 1, 9, 16), (2, 9, 1, 16), (1, 2, 2, 4), (3, 7, 5, 20)]
ESE_C = (16, 20, 112, 384, 512, 528, 2048)
ESE_HW = (1, 15, 400)
# P of the from-colsum forms per C: slice 0's 8-way unrolled loop runs zero, one and (where listed) two times, with a remainder
ESE_P = {16: (1, 255, 256 * 8 + 3, 256 * 16 + 5), 20: (3, 204 * 8 + 1), 112: (5, 36 * 8 + 7, 36 * 16 + 9), 384: (7, 10 * 8 + 3, 10 * 16 + 3),
         512: (7, 8 * 8 + 3, 8 * 16 + 3), 528: (6, 7 * 8 + 2, 7 * 16 + 5), 2048: (1, 15, 2 * 8 + 1, 2 * 16 + 1)}
CORR_MAPS = [(1, 1, 1), (2, 1, 7), (2, 7, 1), (3, 5, 6)]
CORR_LEVELS = [[(6, 7), (3, 4), (2, 2)], [(5, 5), (3, 3), (2, 1), (1, 1)]]
SUPPORT_S = (1, 2, 3, 4, 5, 7, 8, 16, 32)
SUPPORT_C = (1, 5, 128)
GN_LEVELS = [[100, 30, 7], [65, 64, 63, 1]]
GN_CG = [(128, 32), (64, 16), (32, 32), (256, 32)]
HEAD_LEVELS = [[(8, 8)], [(9, 7)], [(1, 1)], [(1, 13), (13, 1)], [(10, 12), (5, 6), (3, 3)], [(16, 8), (8, 4), (4, 2), (2, 1)]]
INFER_OPS = {
    "stem": (("ore_stem1_fwd", "ore_stem1_bf16_fwd"), ("k_stem1",),
             ["NT 1 / 2 / 4 / 8", "u8 and f32 images", "bf16 output", "M % 16 != 0", "M < 16", "one row", "one column", "Hp, Wp >> H, W",
              "two groups per wave", "M >= 2^22", "out_ld > Cout with an offset", "Wo off powers of two"]),
    "maxpool": (("ore_maxpool3x3s2_fwd", "ore_maxpool3x3s2_bf16_fwd"), ("k_maxpool",),
                ["one row", "one column", "2 x 2", "C = 20", "gate", "sliced in and out"]),
    "ese_gate": (("ore_ese_gate_fwd", "ore_ese_gate_bf16_fwd", "ore_ese_gate_pool_bf16_fwd", "ore_ese_gate_from_colsum_fwd", "ore_ese_gate_scaled_weight_fwd", "ore_ese_gate_scaled_weight_bf16_fwd",
                  "ore_scale_channels_fwd", "ore_ese_gate_pool_fwd"),
                 ("k_colsum_partial", "k_ese_gate_fused", "k_ese_gate_pool", "k_scale_channels"),
                 ["C > 512", "1024 / (C / 4) not an integer", "unrolled loop 0, 1, 2 times with a remainder", "P > HW", "C % 16 != 0",
                  "lrows 1 / 16 / 128", "pool (1, 9), (9, 1), (2, 2)", "pool with a short last pixel block"]),
    "correlation": (("ore_correlation_fwd", "ore_correlation_levels_fwd", "ore_correlation_levels_bf16_fwd"), ("k_correlation",),
                    ["H = 1", "W = 1", "single pixel", "four levels", "B > 1 with bf16", "in place", "per-level kernels (the C ABI fixes kstride = C)"]),
    "support_kernels": (("ore_support_kernels_fwd",), ("k_support_kernels",), ["s % 3 != 0", "s in {1, 2}", "s * s > 64", "C = 1"]),
    "groupnorm_levels": (("ore_groupnorm_affine_levels_fwd", "ore_groupnorm_affine_levels_bf16_fwd"),
                         ("k_gn_chunk_stats", "k_gn_chunk_stats4", "k_gn_combine"),
                         ["HW off multiples of 64", "HW = 1", "four levels", "both statistics kernels", "RPT 4 and 8", "bf16"]),
    "head_pred": (("ore_head_pred_fwd", "ore_head_pred_bf16_fwd", "ore_head_pred_gn_fwd", "ore_head_pred_gn_bf16_fwd"), ("k_head_pred",),
                  ["partial tiles", "H or W below 8", "single pixel", "one row / one column", "four levels", "ld 256", "out_ld 8",
                   "ep_stride 16", "B = 2"]),
    "roi_align": (("ore_roi_align_fwd", "ore_roi_align_batched_fwd", "ore_roi_align_bf16_fwd"), ("k_roi_align",),
                  ["three and four levels", "pooled 1 / 4 / 7 / 8 / 14", "C 4 / 16 / 128", "exact boxes on the decision boundaries",
                   "zero-area and inverted boxes", "boxes outside the image", "device count below / at / above cap", "batched, interleaved",
                   "ld > C"]),
}
# every other __global__ of csrc/ore_misc.hip and every other kernel of csrc/ore_roi.hip, and where it is pinned
NOT_COVERED = {
    "k_correlation_classes": "internal N-way fan-out: bit-identical per class to k_correlation in tests/test_hip_nway.py",
    "k_copy_cols": "plain copy of a channel slice, part of the N-way pass: bitwise in tests/test_hip_nway.py",
    "k_roi_predict": "bit-exact against the C twin (oracle/ref_decode.c): the GENERAL form of tests/test_hip_roitail.py (tests/roitail_ref.py)",
    "k_roi_predict_mb": "bit-exact against the C twin: the FUSED64 and FUSED8 (K-split partials) forms of tests/test_hip_roitail.py",
    "k_roi_finalize": "bit-exact against the C twin: the GENERAL form of tests/test_hip_roitail.py",
    "k_roi_tail": "bit-exact against the C twin: both fused forms of tests/test_hip_roitail.py, every hard decision a case class of its own",
    "k_roi_merge_classes": "bit-exact against the C twin (tests/test_hip_nway.py)",
    "k_roi_align_bwd": "training: held to float64 in tests/test_hip_trainloss.py (tests/trainloss_ref.py roi_align_bwd_ref)",
    "k_roi_align_bwd_col": "training: held to float64 in tests/test_hip_trainloss.py (tests/trainloss_ref.py roi_align_bwd_ref)",
    "k_roi_align_bwd_tile": "training: held to float64 in tests/test_hip_trainloss.py (tests/trainloss_ref.py roi_align_bwd_ref)",
    "k_roi_bwd_finalize": "training: tests/test_hip_train.py, tests/test_hip_properties.py",
}


def covered_kernels():
    return {k for _, ks, _ in INFER_OPS.values() for k in ks}
