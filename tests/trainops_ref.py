"""float64 restatements of the non-conv kernels a training step launches (csrc/ore_bwd.hip and their forward partners in
csrc/ore_misc.hip), the chain depths of those kernels, and the operands the tests feed them.

Every restatement works on NHWC tensors ([B, H, W, C] or [B, rows, C]) and returns (ref, mag) per output: `ref` the float64 value,
`mag` the SAME expression with every operand, product and sum term replaced by its modulus (subtractions become additions; a mask
stays the mask).  A kernel output is then held to the two checks of dgrad_ref.check with the kernel's depth d, u = 2^-24, C_S = 1:
    every element                     |got - ref| <= 2 d u mag              (an element with mag == 0 must be exact)
    every 16-row x 16-channel block   rms((got - ref) / mag) <= C_S u sqrt(d)
d is the longest chain of fp32 roundings behind one output element, read off the kernel's documented summation order; any
summation with that chain length satisfies |got - ref| <= ((1 + u)^d - 1) sum |terms| <= 2 d u mag.

Chain depths (function, kernel, derivation):
  d_colsum(rows, beta)        k_colsum_chunks: a 256-row chunk is dealt to 4 row lanes x 2 accumulators, <= 32 rows each (32
                              additions), s0 + s1 (1), the lanes as (l0 + l1) + (l2 + l3) (2).  k_colsum_final: the cps chunk sums
                              go to 4 lanes x 2 accumulators again, ceil(cps / 8) additions, then 1 + 2, and beta * old + s (2).
                              d = min(32, ceil(rows / 8)) + 3 + ceil(cps / 8) + 3 + (2 if beta).
  d_prod_colsum(rows, S, per, q)  k_colsum_seg: a slab of R rows goes to 16 row lanes; a lane with n rows (ceil or floor of R / 16) adds its
                              n // 4 full groups of four rows to the accumulators a0..a3 and its n % 4 leftover rows to a0 again, so
                              the a0 chain has n // 4 + n % 4 additions (+ 1 for the product p * q); (a0 + a1) + (a2 + a3) (2), the
                              16 lanes in one chain (16), then k_colsum_seg_fin's chain over the S slabs (S, 0 when S == 1) and
                              * scale (1).  d = max over slabs and lanes of (n // 4 + n % 4) + q + 2 + 16 + (S if S > 1) + 1, with
                              (S, per) = prod_colsum_plan(...); the slabs have `per` rows, the last one the remainder.
  d_gn_stats(rpi, C, G)       one 64-row chunk, then Chan's combine.  k_gn_chunk_stats (generic): a thread sums 64 * C / 256 values,
                              the rpar * cpg partial sums (rpar = 256 / C) go in one chain, one division: the chunk mean; x - mu, the
                              square, and the same two chains for M2: 2 * (64 * C / 256 + rpar * cpg + 2).  k_gn_chunk_stats4
                              (cpg == 4, RPT = 64 G / 256 in {4, 8} rows per thread, 256 / G row lanes): a row's group sum is
                              (x + y) + (z + w) (2), the RPT rows of a thread in one chain (RPT), the lanes in one chain (256 / G),
                              the division (1); M2 from the same registers: v - mu (1), the square (1), (a^2 + b^2) + (c^2 + d^2)
                              (2), RPT, 256 / G: 2 * (RPT + 256 / G) + 7.  Chan's combine (k_gn_combine): nsl = 4 or 8 slices of
                              ceil(nchunk / nsl) records, six roundings per record (nt, d, nb / nt, mean, d * d * (n nb / nt), m2),
                              then nsl - 1 more records.  Then Q / N + eps, sqrt, 1 / ., * gamma, beta - mean * m (6).
                              d = chunk part + 6 * (ceil(nchunk / nsl) + nsl) + 6.
                              The relative error of rstd is half that of the variance; the check uses the full d for both outputs.
  D_GN_APPLY = 4              k_gn_apply: x * r + a (2), * gamma + beta (2); ReLU is 1-Lipschitz.
  d_gn_bwd(rpi, cpg)          k_gn_bwd_prod: xhat = x * r + a (2), dy' * xhat (1); the per-image column sums
                              (d_colsum(rpi)); k_gn_bwd_dx: S1 / S2 as chains of cpg products (2 cpg), xhat * S2, + S1, * inv_n
                              (1 / (rpi * cpg) itself rounded: 2), gamma * dy', the difference, * r (3):
                              dx: d = 3 + d_colsum(rpi) + 2 cpg + 8;  dbeta: d_colsum(rpi);  dgamma: 3 + d_colsum(rpi).
  D_SCALE_ADD = 2, D_COMBINE2 = 3, D_COMBINE2_BWD = 2, D_SUMPOOL = 3 (four terms), D_ACCUMULATE = 1   literal counts.
  D_CORR_FWD = 12             k_corr_fwd_train: t = relu(3 products, 2 additions) (5), u = 3 products of t, 2 additions (5 more),
                              attn = a2 + relu(u) + q (2); a2 = relu(k11 * relu(k11 * q)) is the shorter branch.
  D_CORR_DT = 6, D_CORR_DQ = 15   k_corr_bwd_a: dT = [t > 0] (3 products of dU, 2 additions) (5, + 1 for the mask product being a
                              select: kept as slack); k_corr_bwd_b: 3 products of dT + 2 additions on top (5), da1 * k11 with
                              da1 = da2 * k11 (2), and g + g2 + . + . (3).
  d_corr_dk(rps)              the per-row products (dT * q: D_CORR_DT + 1; dU * t: 1; da2 * a1 + da1 * q: 5) column-summed per
                              segment: D_CORR_DT + 1 + d_colsum(rps).
  d_apool(H, W, C, OH, OW)    k_apool_fwd: a bin of n pixels in one chain (n) and the division (1).  k_apool_fwd_big (bin >= 64):
                              the n pixels dealt to nsl = 256 / (C / 4) slices, ceil(n / nsl) additions each, the slices in one
                              chain (nsl), the division (1).  n is the largest bin.
  d_apool_bwd(H, W, OH, OW)   k_apool_bwd: input pixel (y, x) gathers dy / |bin| (the division rounds, the bin area is exact) from every
                              bin that covers it, in one chain: ny * nx terms, ny / nx the most bins of an axis that share a pixel
                              (1 when pooling down to disjoint bins, 2 with overlapping bins, more when up-sampling: 4 for 5 -> 12).
                              d = ny * nx + 1.
  D_MAXPOOL_BWD = 4           k_maxpool_bwd: a pixel owns at most 4 windows (2 per axis): 4 additions.
  d_group_mean(N)             k_group_sum: N additions, * (1 / N) with 1 / N rounded (2).  Backward: dy * (1 / N), 2 (exact when N
                              is a power of two: compared with torch.equal).
  d_ese_*                     the eSE node: the kernels above plus torch's [B, C] x [C, C] products, chains of at most C terms.
Exact ops (no rounding, torch.equal): granule transposes without accumulate, group_mean backward for N a power of two, max-pool
forward, the ownership pattern of max-pool backward.

Masks.  A backward that selects on the sign of a SAVED tensor takes that tensor from the product's own forward output: y of
GroupNorm+ReLU, t and u of the correlation (they are arguments of the backward entry points, so the restatements simply read the
mask from the argument).  The correlation's inner masks, [k11 q > 0] and [k11 relu(k11 q) > 0], are signs of products of the
kernel's fp32 inputs; the sign of an fp32 product is exact (no underflow at these scales), so float64 sees the same masks.

Test infrastructure (used by tests/ only)."""
import contextlib
import math

import torch

from dgrad_ref import C_S, U, bf16_rne, c16, check  # noqa: F401  (re-exported: the project's unit roundoff, C_S = 1 and the two checks)

F64 = torch.float64


def _cdiv(a, b):
    return -(-a // b)


_DT = [F64]


def _d(t, device=None):
    return t.to(device or t.device, _DT[0])


@contextlib.contextmanager
def precision(dtype):
    """Evaluate the restatements in `dtype` instead of float64: with torch.float32 every elementwise operation rounds once, which
    is the fp32 emulation of the elementwise kernels in tests/test_trainops_host.py."""
    _DT[0] = dtype
    try:
        yield
    finally:
        _DT[0] = F64


# ---- chain depths ----------------------------------------------------------------------------------------------------------------
CS_ROWS = 256          # k_colsum_chunks
GN_ROWS = 64           # k_gn_chunk_stats
D_GN_APPLY, D_SCALE_ADD, D_COMBINE2, D_COMBINE2_BWD, D_SUMPOOL, D_ACCUMULATE = 4, 2, 3, 2, 3, 1
D_CORR_FWD, D_CORR_DT, D_CORR_DQ, D_MAXPOOL_BWD = 12, 6, 15, 4


def d_colsum(rows, beta=False):
    cps = _cdiv(rows, CS_ROWS)
    return min(32, _cdiv(rows, 8)) + 3 + _cdiv(cps, 8) + 3 + (2 if beta else 0)


def prod_colsum_plan(B, rows, C, workspace_floats):
    """(S, per) of ore_prod_colsum_fwd: S row slabs of `per` rows (the last one shorter).  Slabs only from 2048 rows on: enough to
    reach 1024 blocks over the ceil(C / 64) x B grid, at least 512 rows each, as many as the workspace holds [B][C] partial sums for;
    then evened out to whole multiples of 64 rows."""
    S = 1
    if rows >= 2048:
        S = min(_cdiv(1024, _cdiv(C, 64) * B), rows // 512)
        S = max(1, min(S, workspace_floats // (B * C)))
    per = _cdiv(_cdiv(rows, S), 64) * 64
    return _cdiv(rows, per), per


def d_prod_colsum(rows, S, per, has_q):
    chain = 0
    for R in {min(per, rows), rows - (S - 1) * per}:          # the full slabs and the last one
        for n in {_cdiv(R, 16), R // 16}:                     # rows of a lane
            chain = max(chain, n // 4 + n % 4)
    return chain + int(bool(has_q)) + 2 + 16 + (S if S > 1 else 0) + 1


def gn_stats_kernel(C, G):
    """The statistics kernel ore_groupnorm_affine_fwd picks (16-byte aligned x, ld and coff multiples of 4)."""
    if C == 4 * G and 256 % G == 0 and GN_ROWS * G % 256 == 0 and GN_ROWS * G // 256 in (4, 8):
        return "k_gn_chunk_stats4"
    return "k_gn_chunk_stats"


def d_gn_stats(rpi, C, G):
    cpg, nchunk, nsl = C // G, _cdiv(rpi, GN_ROWS), (4 if G > 32 else 8)
    if gn_stats_kernel(C, G) == "k_gn_chunk_stats4":
        chunk = 2 * (GN_ROWS * G // 256 + 256 // G) + 7
    else:
        chunk = 2 * (GN_ROWS * C // 256 + (256 // C) * cpg + 2)
    return chunk + 6 * (_cdiv(nchunk, nsl) + nsl) + 6


def d_gn_bwd(rpi, cpg):
    cs = d_colsum(rpi)
    return {"dx": 3 + cs + 2 * cpg + 8, "dbeta": cs, "dgamma": 3 + cs}


def d_corr_dk(rps):
    return D_CORR_DT + 1 + d_colsum(rps)


def apool_bins(L, S):
    return [((i * L) // S, _cdiv((i + 1) * L, S)) for i in range(S)]


def apool_kernel(H, W, C, OH, OW):
    """The forward kernel ore_adaptive_avgpool_nhwc_fwd picks."""
    return "k_apool_fwd_big" if (_cdiv(H, OH) + 1) * (_cdiv(W, OW) + 1) >= 64 and C <= 1024 else "k_apool_fwd"


def d_apool(H, W, C, OH, OW):
    n = max(b - a for a, b in apool_bins(H, OH)) * max(b - a for a, b in apool_bins(W, OW))
    if apool_kernel(H, W, C, OH, OW) == "k_apool_fwd_big":
        nsl = 256 // (C // 4)
        return _cdiv(n, nsl) + nsl + 1
    return n + 1


def d_apool_bwd(H, W, OH, OW):
    cover = lambda L, S: max(sum(a <= i < b for a, b in apool_bins(L, S)) for i in range(L))      # noqa: E731
    return cover(H, OH) * cover(W, OW) + 1


def d_group_mean(N):
    return N + 2


def d_ese(rows, C, B, plan, plan_q):
    """Depths of the outputs of the eSE node (orehip/autograd.py EseFn): the pooled mean (ore_prod_colsum_fwd, scale 1 / HW), torch's
    addmm over C terms and hard-sigmoid (3), x * gate; backward: sum dy * x, / 6, the C-term products with W, / HW, dy * gate + c."""
    dm = d_prod_colsum(rows, *plan, False)
    dg = d_prod_colsum(rows, *plan_q, True)
    y = dm + C + 1 + 3 + 1
    return {"m": dm, "y": y, "dx": y + dg + 1 + C + 1 + D_SCALE_ADD, "dW": dg + 1 + B + dm + 1, "db": dg + 1 + B}


# ---- operands --------------------------------------------------------------------------------------------------------------------
def scaled_inputs(shape, seed, device="cpu", lo=-3.0, hi=3.0, per_image=False, image_decades=1.0):
    """fp32 tensor of `shape` = [B, ..., C]: unit normals times per-channel scales 10^U(lo, hi) (as dgrad_ref.scaled_operands), and
    with per_image also times per-image scales 10^U(-image_decades, image_decades).  An error confined to a small channel or image
    is then visible to the element-wise bound while a max-norm over the tensor would not see it."""
    g = torch.Generator(device=device).manual_seed(seed)
    f64 = dict(generator=g, dtype=F64, device=device)
    sc = 10.0 ** (torch.rand(shape[-1], **f64) * (hi - lo) + lo)
    x = torch.randn(*shape, **f64) * sc
    if per_image:
        si = 10.0 ** (torch.rand(shape[0], **f64) * 2 * image_decades - image_decades)
        x = x * si.view(-1, *([1] * (len(shape) - 1)))
    return x.float()


GN_OFFSET_SIGMAS = 30.0


def gn_inputs(B, rpi, C, G, seed, device="cpu"):
    """x [B, rpi, C] fp32 for GroupNorm(G, C): every group has its own scale s_g = 10^U(-3, 3), its channels mild relative factors
    f_c in [0.5, 2], and every (image, group) a mean offset of U(-30, 30) group standard deviations -- what the tower conv's bias
    produces, and what makes a one-pass variance (E x^2 - mean^2) lose its digits."""
    g = torch.Generator(device=device).manual_seed(seed)
    f64 = dict(generator=g, dtype=F64, device=device)
    cpg = C // G
    sg = 10.0 ** (torch.rand(G, **f64) * 6 - 3)
    fc = 2.0 ** (torch.rand(G, cpg, **f64) * 2 - 1)
    sigma = (fc ** 2).mean(1).sqrt()                                        # std of a group's unit-scale values
    off = (torch.rand(B, G, **f64) * 2 - 1) * GN_OFFSET_SIGMAS * sigma
    if B * G > 1:
        off.view(-1)[0] = GN_OFFSET_SIGMAS * sigma[0]                       # the extreme is present in every draw
    x = torch.randn(B, rpi, G, cpg, **f64) * fc + off.view(B, 1, G, 1)
    return (x * sg.view(1, 1, G, 1)).reshape(B, rpi, C).float()


ESE_KNEE_MARGIN = 1e-3


def ese_inputs(B, H, W, C, seed, device="cpu"):
    """(x [B,H,W,C], fc_w [C,C,1,1], fc_b [C]) fp32 for the eSE node: x = s_c * (N(0,1) + 1) with per-channel and per-image scales,
    fc_w[o, i] ~ 2 N(0,1) / (sqrt(C) s_i) so that every pre-activation z = fc(mean(x)) is O(1) whatever the channel scales, fc_b in
    U(-3, 3): gates on both knees and in between.  The bias is then nudged until every z of the float64 reference is at least twice
    ESE_KNEE_MARGIN away from +-3 (tests assert the margin itself): no element's hard-sigmoid branch depends on fp32 rounding."""
    g = torch.Generator(device=device).manual_seed(seed)
    f64 = dict(generator=g, dtype=F64, device=device)
    sc = 10.0 ** (torch.rand(C, **f64) * 6 - 3)
    si = 10.0 ** (torch.rand(B, **f64) * 2 - 1)
    x = ((torch.randn(B, H, W, C, **f64) + 1.0) * sc * si.view(B, 1, 1, 1)).float()
    w = (2.0 * torch.randn(C, C, **f64) / (math.sqrt(C) * sc.view(1, C))).float()
    b = (torch.rand(C, **f64) * 6 - 3).float()
    m = x.double().mean((1, 2))
    for _ in range(200):
        z = b.double() + m @ w.double().t()
        bad = (((z.abs() - 3.0).abs() < 2 * ESE_KNEE_MARGIN).any(0))
        if not bool(bad.any()):
            break
        b = torch.where(bad, b + 5 * ESE_KNEE_MARGIN, b)
    return x, w.reshape(C, C, 1, 1), b


def ese_knee_distance(x, fc_w, fc_b):
    """min over (image, channel) of | |z| - 3 | for the float64 pre-activations z of the eSE gate."""
    C = x.shape[-1]
    z = fc_b.double() + x.double().mean((1, 2)) @ fc_w.double().reshape(C, C).t()
    return float((z.abs() - 3.0).abs().min())


# ---- sums ------------------------------------------------------------------------------------------------------------------------
def colsum(x, segments=1, beta=0.0, old=None, device=None):
    """ore_colsum_fwd / ore_colsum_segments_fwd (the bias gradient, d2z:layers/wrappers.py Conv2d bias; the per-image sums of
    GroupNorm and the correlation): x [rows, C] in `segments` equal runs -> [segments, C]; beta * old + sums."""
    x = _d(x, device)
    x = x.reshape(segments, -1, x.shape[-1])
    ref, mag = x.sum(1), x.abs().sum(1)
    if beta != 0.0:
        o = beta * _d(old, device).reshape(ref.shape)
        ref, mag = ref + o, mag + o.abs()
    return ref, mag


def prod_colsum(p, q=None, scale=1.0, device=None):
    """ore_prod_colsum_fwd (the eSE pool and gate gradient, d2z:modeling/backbone/vovnet.py:238-260; the SM_Block's pooled mean,
    fsod_cen.py:612): p (, q) [B, ..., C] -> scale * sum over pixels of p (* q), [B, C]."""
    B, C = p.shape[0], p.shape[-1]
    v = _d(p, device).reshape(B, -1, C)
    if q is not None:
        v = v * _d(q, device).reshape(B, -1, C)
    return v.sum(1) * scale, v.abs().sum(1) * abs(scale)


def scale_add(x, s, v=None, device=None):
    """ore_scale_add_channels_fwd: x [B, ..., C] * s [B, C] + v [B, C] (eSE's x * gate and its backward dy * gate + dm / HW)."""
    B, C = x.shape[0], x.shape[-1]
    xs = _d(x, device).reshape(B, -1, C) * _d(s, device).reshape(B, 1, C)
    ref, mag = xs, xs.abs()
    if v is not None:
        vv = _d(v, device).reshape(B, 1, C)
        ref, mag = ref + vv, mag + vv.abs()
    return ref.reshape(x.shape), mag.reshape(x.shape)


def group_mean(x, groups, device=None):
    """ore_group_mean_fwd (the prototype = mean over an image's shots, fsod_cen.py:228): [groups * N, ...] -> [groups, ...]."""
    x = _d(x, device)
    v = x.reshape(groups, x.shape[0] // groups, -1)
    return v.mean(1).reshape(groups, *x.shape[1:]), v.abs().mean(1).reshape(groups, *x.shape[1:])


def group_mean_bwd(dy, groups, N, device=None):
    dy = _d(dy, device)
    r = (dy / N).repeat_interleave(N, 0)
    return r, r.abs()


def mean_pair(h, w, device=None):
    """A.mean_pair (fsod_cen.py:612): mean over pixels of (h + w), [B, C]."""
    n = h.numel() // (h.shape[0] * h.shape[-1])
    a, am = prod_colsum(h, None, 1.0 / n, device)
    b, bm = prod_colsum(w, None, 1.0 / n, device)
    return a + b, am + bm


# ---- GroupNorm -------------------------------------------------------------------------------------------------------------------
def gn_stats(x, G, eps, device=None):
    """ore_groupnorm_affine_fwd with unit affine (ref:CenterNet2/centernet/modeling/dense_heads/centernet_head.py:141-149,
    GroupNorm(32, 128)): x [B, rpi, C] -> r = rstd of the channel's group, a = -mean * rstd, both [B, C].  mag: r itself (the variance
    is a sum of non-negative terms), mean|x| * r for a."""
    x = _d(x, device)
    B, rpi, C = x.shape
    xg = x.reshape(B, rpi, G, C // G)
    mean = xg.mean((1, 3))
    var = ((xg - mean.view(B, 1, G, 1)) ** 2).mean((1, 3))
    r = 1.0 / (var + eps).sqrt()
    rep = lambda t: t.repeat_interleave(C // G, 1)          # noqa: E731
    return (rep(r), rep(r)), (rep(-mean * r), rep(xg.abs().mean((1, 3)) * r))


def gn_apply(x, r, a, gamma, beta, relu, device=None):
    """ore_groupnorm_apply_fwd: relu?((x * r + a) * gamma + beta), r / a [B, C] per image."""
    x, r, a, gamma, beta = (_d(t, device) for t in (x, r, a, gamma, beta))
    B, rpi, C = x.shape
    xr = x * r.view(B, 1, C)
    ref = (xr + a.view(B, 1, C)) * gamma + beta
    mag = (xr.abs() + a.abs().view(B, 1, C)) * gamma.abs() + beta.abs()
    return (ref.clamp(min=0) if relu else ref), mag


def gn_bwd(dy, y, x, r, a, gamma, G, relu, device=None, n_wrong=False):
    """ore_groupnorm_bwd (the backward of F.group_norm (+ReLU) given the saved statistics): dy, y, x [B, rpi, C]; r, a [B, C].
        dy' = dy [y > 0 or no ReLU];  xhat = x r + a;  dbeta = sum_rows dy';  dgamma = sum_rows dy' xhat   (per image)
        dx = r (gamma dy' - (S1 + xhat S2) / n),  S1 = sum_{c in g} gamma dbeta, S2 = sum_{c in g} gamma dgamma, n = rpi * cpg
    -> {"dx": (ref, mag), "dbeta": ..., "dgamma": ...}.  n_wrong: n = rpi (a fault for tests/test_trainops_host.py)."""
    dy, y, x, r, a, gamma = (_d(t, device) for t in (dy, y, x, r, a, gamma))
    B, rpi, C = x.shape
    cpg = C // G
    g = dy * (y > 0) if relu else dy
    rv, av = r.view(B, 1, C), a.view(B, 1, C)
    xh, xhm = x * rv + av, (x * rv).abs() + av.abs()
    db, dbm = g.sum(1), g.abs().sum(1)
    dg, dgm = (g * xh).sum(1), (g.abs() * xhm).sum(1)
    grp = lambda t: t.reshape(B, G, cpg).sum(2).repeat_interleave(cpg, 1).view(B, 1, C)      # noqa: E731
    s1, s1m, s2, s2m = grp(gamma * db), grp(gamma.abs() * dbm), grp(gamma * dg), grp(gamma.abs() * dgm)
    n = float(rpi if n_wrong else rpi * cpg)
    dx = rv * (gamma * g - (s1 + xh * s2) / n)
    dxm = rv.abs() * (gamma.abs() * g.abs() + (s1m + xhm * s2m) / n)
    return {"dx": (dx, dxm), "dbeta": (db, dbm), "dgamma": (dg, dgm)}


# ---- eSE -------------------------------------------------------------------------------------------------------------------------
def ese_node(x, fc_w, fc_b, dy=None, device=None):
    """eSE (d2z:modeling/backbone/vovnet.py:238-260): y = x * hsigmoid(fc(mean_hw(x))), hsigmoid(z) = relu6(z + 3) / 6, and its
    gradients.  -> {"m", "z", "y", "dx", "dW", "db"}: (ref, mag) each (z: the float64 pre-activations, no mag)."""
    x, b = _d(x, device), _d(fc_b, device)
    B, H, W, C = x.shape
    Wm = _d(fc_w, device).reshape(C, C)
    n = H * W
    m, mm = x.mean((1, 2)), x.abs().mean((1, 2))
    z, zm = b + m @ Wm.t(), b.abs() + mm @ Wm.abs().t()
    g, gm = (z / 6 + 0.5).clamp(0, 1), zm / 6 + 0.5
    out = {"m": (m, mm), "z": z, "y": (x * g.view(B, 1, 1, C), x.abs() * gm.view(B, 1, 1, C))}
    if dy is None:
        return out
    dy = _d(dy, device)
    dg, dgm = (dy * x).sum((1, 2)), (dy * x).abs().sum((1, 2))
    act = (z.abs() < 3).to(z.dtype)
    dz, dzm = dg / 6 * act, dgm / 6 * act
    dm, dmm = dz @ Wm, dzm @ Wm.abs()
    out["dx"] = (dy * g.view(B, 1, 1, C) + (dm / n).view(B, 1, 1, C), dy.abs() * gm.view(B, 1, 1, C) + (dmm / n).view(B, 1, 1, C))
    out["dW"] = (dz.t() @ m, dzm.t() @ mm)
    out["db"] = (dz.sum(0), dzm.sum(0))
    return out


# ---- correlation -----------------------------------------------------------------------------------------------------------------
def _taps(k, B, C):
    """k [C, 3] (shared) or [B, C, 3] -> three [B or 1, 1, 1, C] tap tensors."""
    k = k.reshape(-1, C, 3)
    return [k[:, :, j].reshape(-1, 1, 1, C) for j in range(3)]


def _shift(t, dy, dx, wrap=None):
    """t[b, y + dy, x + dx, c] with zeros outside the image.  wrap (faults for tests/test_trainops_host.py): "row" reads x + dx across
    the row end into the neighbouring row, "image" reads y + dy across the image seam into the neighbouring image."""
    B, H, W, C = t.shape
    s = dy * W + dx
    if s != 0 and ((wrap == "row" and dx != 0) or (wrap == "image" and dy != 0)):
        flat = t.reshape(1, B * H * W, C) if wrap == "image" else t.reshape(B, H * W, C)
        z = torch.zeros_like(flat)
        n = flat.shape[1]
        if s > 0:
            z[:, :n - s] = flat[:, s:]
        else:
            z[:, -s:] = flat[:, :n + s]
        return z.reshape(B, H, W, C)
    p = torch.nn.functional.pad(t, (0, 0, 1, 1, 1, 1))
    return p[:, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W, :]


def corr_fwd(q, k11, k13, k31, device=None, wrap=None):
    """ore_correlation_train_fwd (ref:fewx/modeling/fsod/fsod_cen.py:229-245, training branch), q [B,H,W,C]; k11 [C] / k13, k31 [C,3]
    shared or [B,C] / [B,C,3] per image:
        a2 = relu(k11 relu(k11 q));  t = relu(conv1x3(q, k13));  u = conv3x1(t, k31);  attn = a2 + relu(u) + q;  cat = [attn | q]
    -> {"cat": (ref, mag) [B,H,W,2C], "t": ..., "u": ...}."""
    q = _d(q, device)
    B, H, W, C = q.shape
    w11 = _d(k11, device).reshape(-1, 1, 1, C)
    w13, w31 = _taps(_d(k13, device), B, C), _taps(_d(k31, device), B, C)
    qa = q.abs()
    a2 = (w11 * (w11 * q).clamp(min=0)).clamp(min=0)
    a2m = w11.abs() * w11.abs() * qa
    tp = sum(w13[j] * _shift(q, 0, j - 1, wrap) for j in range(3))
    tm = sum(w13[j].abs() * _shift(qa, 0, j - 1, wrap) for j in range(3))
    t = tp.clamp(min=0)
    u = sum(w31[j] * _shift(t, j - 1, 0, wrap) for j in range(3))
    um = sum(w31[j].abs() * _shift(tm, j - 1, 0, wrap) for j in range(3))
    attn, attnm = a2 + u.clamp(min=0) + q, a2m + um + qa
    return {"cat": (torch.cat([attn, q], -1), torch.cat([attnm, qa], -1)), "t": (t, tm), "u": (u, um)}


def corr_bwd(q, k11, k13, k31, dcat, T, Us, device=None, reverse_taps=False, segsum=None):
    """ore_correlation_train_bwd: the gradient of corr_fwd given dcat [B,H,W,2C] and the SAVED t, u (the masks [t > 0], [u > 0] and
    the values of t in dk31 come from them).  dk per image when the kernels are per image, else summed over the batch.
    -> {"dq", "dk11" [S,C], "dk13" [S,C,3], "dk31" [S,C,3]}: (ref, mag) each, S = B or 1.  reverse_taps: dk13 / dk31 with their
    taps in reverse order (a fault for tests/test_trainops_host.py).  segsum(rows [S * rps, C], S) -> [S, C]: the per-segment
    column sum of the per-row products, for an emulation that sums them in the kernel's order."""
    q, dcat, T, Us = (_d(t, device) for t in (q, dcat, T, Us))
    B, H, W, C = q.shape
    per_image = k11.dim() == 2
    w11 = _d(k11, device).reshape(-1, 1, 1, C)
    w13, w31 = _taps(_d(k13, device), B, C), _taps(_d(k31, device), B, C)
    g, g2 = dcat[..., :C], dcat[..., C:]
    ga, qa, Ta = g.abs(), q.abs(), T.abs()
    du, dum = g * (Us > 0), ga * (Us > 0)
    tmask = (T > 0)
    dt = tmask * sum(w31[j] * _shift(du, 1 - j, 0) for j in range(3))
    dtm = tmask * sum(w31[j].abs() * _shift(dum, 1 - j, 0) for j in range(3))
    s1 = w11 * q
    a1, a1m = s1.clamp(min=0), (s1 > 0) * s1.abs()
    m2 = (w11 * a1 > 0)
    da2, da2m = g * m2, ga * m2
    da1, da1m = (s1 > 0) * da2 * w11, (s1 > 0) * da2m * w11.abs()
    dq = g + g2 + da1 * w11 + sum(w13[j] * _shift(dt, 0, 1 - j) for j in range(3))
    dqm = ga + g2.abs() + da1m * w11.abs() + sum(w13[j].abs() * _shift(dtm, 0, 1 - j) for j in range(3))
    S = B if per_image else 1
    seg = (lambda t: t.reshape(S, -1, C).sum(1)) if segsum is None else (lambda t: segsum(t.reshape(-1, C), S))       # noqa: E731
    order = (2, 1, 0) if reverse_taps else (0, 1, 2)
    d11, d11m = seg(da2 * a1 + da1 * q), seg(da2m * a1m + da1m * qa)
    d13 = torch.stack([seg(dt * _shift(q, 0, j - 1)) for j in order], -1)
    d13m = torch.stack([seg(dtm * _shift(qa, 0, j - 1)) for j in order], -1)
    d31 = torch.stack([seg(du * _shift(T, j - 1, 0)) for j in order], -1)
    d31m = torch.stack([seg(dum * _shift(Ta, j - 1, 0)) for j in order], -1)
    return {"dq": (dq, dqm), "dk11": (d11, d11m), "dk13": (d13, d13m), "dk31": (d31, d31m)}


# ---- pools -----------------------------------------------------------------------------------------------------------------------
def maxpool_out_hw(H, W):
    """MaxPool2d(3, 2, ceil_mode=True): ceil((n - 3) / 2) + 1 windows, the last one starting inside the input; 1 below 3."""
    def osz(n):
        o = _cdiv(n - 3, 2) + 1 if n >= 3 else 1
        return o - 1 if (o - 1) * 2 >= n else o
    return osz(H), osz(W)


def _windows(x, Ho, Wo):
    """x [B,H,W,C] -> its 3x3 / stride 2 windows [B,Ho,Wo,C,9] in (ky, kx) scan order, -inf outside the input."""
    B, H, W, C = x.shape
    xp = torch.nn.functional.pad(x, (0, 0, 0, 2 * Wo + 1 - W, 0, 2 * Ho + 1 - H), value=-math.inf)
    return xp.unfold(1, 3, 2).unfold(2, 3, 2).reshape(B, Ho, Wo, C, 9)


def maxpool_fwd(x, device=None):
    """ore_maxpool3x3s2_fwd (d2z:modeling/backbone/vovnet.py stage pooling): exact, compared with torch.equal."""
    x = x.to(device or x.device)
    Ho, Wo = maxpool_out_hw(x.shape[1], x.shape[2])
    return _windows(x, Ho, Wo).max(-1).values


def maxpool_owner(x, last=False):
    """[B,Ho,Wo,C] int64: the flat input pixel (y * W + x) that owns each window -- its first maximum in (ky, kx) scan order (ATen's
    max_pool2d rule).  last: the last maximum instead (a fault for tests/test_trainops_host.py)."""
    B, H, W, C = x.shape
    Ho, Wo = maxpool_out_hw(H, W)
    win = _windows(x, Ho, Wo)
    rank = torch.arange(1, 10, device=x.device) if last else torch.arange(9, 0, -1, device=x.device)
    k = ((win == win.max(-1, keepdim=True).values) * rank).argmax(-1)
    oy = torch.arange(Ho, device=x.device).view(1, Ho, 1, 1)
    ox = torch.arange(Wo, device=x.device).view(1, 1, Wo, 1)
    return (2 * oy + k // 3) * W + 2 * ox + k % 3


def maxpool_bwd(x, dy, device=None, last=False):
    """ore_maxpool3x3s2_bwd: every window's dy goes to its owner; a pixel that owns several windows sums them."""
    x = x.to(device or x.device)
    dy = _d(dy, x.device)
    B, H, W, C = x.shape
    own = maxpool_owner(x, last)
    idx = (own + torch.arange(B, device=x.device).view(B, 1, 1, 1) * H * W) * C + torch.arange(C, device=x.device)
    out = []
    for v in (dy, dy.abs()):
        o = torch.zeros(B * H * W * C, dtype=dy.dtype, device=x.device)
        o.index_add_(0, idx.reshape(-1), v.reshape(-1))
        out.append(o.reshape(B, H, W, C))
    return out[0], out[1]


def sumpool2(x, device=None):
    """ore_sumpool2x2_fwd: the backward of the FPN's nearest-2x top-down add (d2z:modeling/backbone/fpn.py:143-150), cropped sums of
    2x2 blocks: [B,H,W,C] -> [B,ceil(H/2),ceil(W/2),C]."""
    x = _d(x, device)
    B, H, W, C = x.shape
    xp = torch.nn.functional.pad(x, (0, 0, 0, W % 2, 0, H % 2))
    f = lambda t: t.reshape(B, (H + 1) // 2, 2, (W + 1) // 2, 2, C).sum((2, 4))     # noqa: E731
    return f(xp), f(xp.abs())


def _bin_matrix(L, S, device):
    m = torch.zeros(S, L, dtype=_DT[0], device=device)
    for i, (a, b) in enumerate(apool_bins(L, S)):
        m[i, a:b] = 1.0
    return m


def apool_fwd(x, OH, OW, device=None, interior_count=False):
    """ore_adaptive_avgpool_nhwc_fwd (F.adaptive_avg_pool2d: bin i of an axis of length L pooled to S covers [floor(i L / S),
    ceil((i + 1) L / S)); ref fsod_cen.py:214-231).  interior_count: every bin divided by the largest bin's size (a fault)."""
    x = _d(x, device)
    B, H, W, C = x.shape
    Iy, Ix = _bin_matrix(H, OH, x.device), _bin_matrix(W, OW, x.device)
    cnt = (Iy.sum(1).view(OH, 1) * Ix.sum(1).view(1, OW)).view(1, OH, OW, 1)
    if interior_count:
        cnt = cnt.max().expand_as(cnt)
    f = lambda t: torch.einsum("oh,bhwc,pw->bopc", Iy, t, Ix) / cnt            # noqa: E731
    return f(x), f(x.abs())


def apool_bwd(dy, H, W, device=None):
    """ore_adaptive_avgpool_nhwc_bwd: input pixel (y, x) collects dy / |bin| from every bin that covers it."""
    dy = _d(dy, device)
    B, OH, OW, C = dy.shape
    Iy, Ix = _bin_matrix(H, OH, dy.device), _bin_matrix(W, OW, dy.device)
    cnt = (Iy.sum(1).view(OH, 1) * Ix.sum(1).view(1, OW)).view(1, OH, OW, 1)
    f = lambda t: torch.einsum("oh,bopc,pw->bhwc", Iy, t / cnt, Ix)            # noqa: E731
    return f(dy), f(dy.abs())


# ---- SM_Block glue ---------------------------------------------------------------------------------------------------------------
def sm_permute(x, B, H, W, G, S, axis, inverse):
    """ore_granule_transpose_fwd as orehip.sm_permute drives it (ref fsod_cen.py:602-611): axis 'h': [B,H,W,G,S] <-> [B,G,W,H,S];
    axis 'w': [B,H,W,G,S] <-> [B,G,H,W,S].  Pure data movement: exact."""
    if axis == "h":
        return x.reshape(B, G, W, H, S).permute(0, 3, 2, 1, 4).contiguous() if inverse else x.reshape(B, H, W, G, S).permute(0, 3, 2, 1, 4).contiguous()
    return x.reshape(B, G, H, W, S).permute(0, 2, 3, 1, 4).contiguous() if inverse else x.reshape(B, H, W, G, S).permute(0, 3, 1, 2, 4).contiguous()


def combine2(w, h, a0, a1, device=None):
    """ore_combine2_fwd (ref fsod_cen.py:614-615): y = w a0[b, c] + h a1[b, c]."""
    w, h, a0, a1 = (_d(t, device) for t in (w, h, a0, a1))
    B, C = w.shape[0], w.shape[-1]
    sh = (B,) + (1,) * (w.dim() - 2) + (C,)
    p0, p1 = w * a0.view(sh), h * a1.view(sh)
    return p0 + p1, p0.abs() + p1.abs()


def combine2_bwd(dy, a0, a1, v=None, device=None):
    """ore_combine2_bwd: dw = dy a0 + v, dh = dy a1 + v with the optional per-(image, channel) constant v."""
    dy, a0, a1 = (_d(t, device) for t in (dy, a0, a1))
    B, C = dy.shape[0], dy.shape[-1]
    sh = (B,) + (1,) * (dy.dim() - 2) + (C,)
    out = []
    for a in (a0, a1):
        r = dy * a.view(sh)
        m = r.abs()
        if v is not None:
            vv = _d(v, device).view(sh)
            r, m = r + vv, m + vv.abs()
        out.append((r, m))
    return out


# ---- the two checks on tensors of any rank ---------------------------------------------------------------------------------------
def check2(got, ref, mag, d):
    """dgrad_ref.check on [..., C] tensors flattened to rows x C: (hard ratio, rms ratio), <= 1 passes."""
    Cc = ref.shape[-1]
    return check(got.reshape(-1, Cc), ref.reshape(-1, Cc), mag.reshape(-1, Cc), d)


def close_old(got, ref, tol=2e-5):
    """The criterion of tests/test_hip_train.py::_close: max |got - ref| <= tol * max |ref| over the whole tensor."""
    return float((got.double() - ref.double()).abs().max()) <= tol * max(float(ref.abs().max()), 1e-6)


# ---- coverage --------------------------------------------------------------------------------------------------------------------
# The non-conv ops of one training step of configs/fsod/finetune_vovnet.yaml at batch 1 (a 640 x 640 query, 24 support crops padded to
# 256 x 256): op -> the orehip functions it goes through and its call classes at batch 1.  A class is the tuple a spy on those functions
# records (image counts first); tests/test_hip_trainops.py::test_production_replay asserts that the recorded set equals this table.
# At batch 16 every image count is 16 times larger (group_mean: 16 groups of 24; the per-image pools of the prototypes: 16 images).
# A function stands for both of its directions: adaptive_avgpool_nhwc and group_mean run forward and (grad_of / backward=True)
# backward, sm_permute both axes, both directions and the accumulating form.
_Q = [(1, 80, 80), (1, 40, 40), (1, 20, 20)]          # query pyramid p3..p5
_S = [(24, 32, 32), (24, 16, 16), (24, 8, 8)]         # support pyramid
TRAIN_OPS = {
    # GroupNorm(32, 128) + ReLU of the head tower, per level: (B, rows per image, C, groups, relu)
    "group_norm_relu": (("groupnorm_affine", "groupnorm_apply", "groupnorm_bwd"), [(b, h * w, 128, 32, True) for b, h, w in _Q]),
    # eSE of the trained stages 4 and 5, query and support: (B, rows per image, C)
    "ese": (("prod_colsum", "scale_add_channels"), [(1, 1600, 384), (24, 256, 384), (1, 400, 512), (24, 64, 512)]),
    # the stage-5 pool over the stage-4 output: (B, H, W, C)
    "maxpool": (("maxpool3x3s2", "maxpool3x3s2_bwd"), [(1, 40, 40, 384), (24, 16, 16, 384)]),
    # backward of the FPN top-down add: (B, H, W, C) of the finer map
    "sumpool2x2": (("sumpool2x2",), [(1, 80, 80, 128), (1, 40, 40, 128), (24, 32, 32, 128), (24, 16, 16, 128)]),
    # SM_Block over the support maps: (B, H, W, G, S)
    "sm_permute": (("sm_permute",), [(24, 32, 32, 32, 4), (24, 16, 16, 16, 8), (24, 8, 8, 8, 16)]),
    # (B, rows per image, C)
    "mean_pair": (("prod_colsum",), [(24, 1024, 128), (24, 256, 128), (24, 64, 128)]),
    "combine2": (("combine2", "combine2_bwd", "prod_colsum"), [(24, 1024, 128), (24, 256, 128), (24, 64, 128)]),
    # prototype over the 24 shots: (groups, N, M)
    "group_mean": (("group_mean",), [(1, 24, 32 * 32 * 128), (1, 24, 16 * 16 * 128), (1, 24, 8 * 8 * 128)]),
    # support kernels, 1x1 / 3x1 / 1x3 pools of the prototype: (B, H, W, C, OH, OW)
    "adaptive_avg_pool": (("adaptive_avgpool_nhwc",), [(1, s, s, 128, oh, ow) for s in (32, 16, 8) for oh, ow in ((1, 1), (3, 1), (1, 3))]),
    # per-image support kernels: (B, H, W, C, per_image)
    "correlation_cat": (("correlation_train_fwd", "correlation_train_bwd"), [(b, h, w, 128, 1) for b, h, w in _Q]),
    # ReLU / FrozenBN masks (bitwise-tested in tests/test_hip_dgrad.py; replayed only, no class of its own)
    "relu_affine_bwd": (("relu_affine_bwd",), []),
    # ore_colsum_fwd (beta, coff, Cc) and ore_colsum_segments_fwd: on this config's training path only inside ore_groupnorm_bwd and
    # ore_correlation_train_bwd (a conv bias gradient rides in the weight-gradient launch), so no call class of their own; covered at the
    # production rows per image and at edge shapes
    "colsum": (("colsum", "colsum_segments"), []),
}
# training-path calls of orehip/autograd.py that this work leaves out, and why
NOT_COVERED = {
    "conv2d": "the conv data gradient and forward: tests/dgrad_ref.py, tests/test_hip_dgrad.py",
    "conv2d_wgrad": "the conv weight gradient: tests/wgrad_ref.py, tests/test_hip_wgrad.py",
    "pack_conv_weight_dev": "weight layouts, bitwise: test_hip_dgrad.py::test_dgrad_pack_layout",
    "pack_conv_weights_multi": "weight layouts, bitwise: test_hip_dgrad.py::test_dgrad_pack_layout",
    "winograd_covers": "a host predicate of the conv plan: tests/test_conv_plan_host.py",
    "winograd_weight": "the Winograd weight transform: pinned with the launches that use it in tests/test_hip_dgrad.py",
    "roi_align": "ROIAlign forward: held to float64 in tests/test_hip_inferops.py (tests/inferops_ref.py roi_align_ref)",
    "roi_align_batched": "ROIAlign forward, batched: held to float64 in tests/test_hip_inferops.py::test_roi_align_batched",
    "roi_align_bwd": "ROIAlign backward, all three launch forms: held to float64 in tests/test_hip_trainloss.py (tests/trainloss_ref.py roi_align_bwd_ref)",
    "roi_losses": "loss kernels of ore_train.hip: held to float64 in tests/test_hip_trainloss.py (tests/trainloss_ref.py)",
    "centernet_loss_sums": "loss kernels of ore_train.hip: held to float64 in tests/test_hip_trainloss.py (tests/trainloss_ref.py)",
    "centernet_loss_grad": "loss kernels of ore_train.hip: held to float64 in tests/test_hip_trainloss.py (tests/trainloss_ref.py)",
}


def covered_functions():
    return {f for fns, _ in TRAIN_OPS.values() for f in fns}


def batch16(op, cls):
    """The call class of `op` at batch 16 for its batch-1 class."""
    if op == "group_mean":
        return (16,) + tuple(cls[1:])
    return (cls[0] * 16,) + tuple(cls[1:])
