"""Restatement of the conv weight-gradient launch (csrc/ore_conv_wgrad.hip, ore_conv2d_wgrad_bias_fwd) and its float64 reference.

`wgrad_plan` mirrors the host dispatch: how many row splits S the launch uses, how many rows each split owns, and which reduce
(`k_wgrad_reduce<G>`) sums the slabs.  `wgrad_ref` computes dW and db in float64 as GEMMs over shifted windows, and `wgrad_check`
holds a result to an element-wise bound derived from the plan.

The bound.  Every output element is a sum of products dz[row][co] * x[row shifted by tap][ci].  Each product is exact in fp32 in
bf16 mode (two 8-bit significands) and rounded at most once in fp32 mode.  The launch adds the products of one split in fp32,
chunk rows deep (MFMA steps of 4 or 32 rows, however the matrix core orders the additions inside one instruction, add at most one
rounding per row).  The reduce then adds ceil(S / G) slabs per group and the G group sums in sequence, and `beta * old + s`
adds two more roundings.  Any summation whose longest chain of roundings is d satisfies
    |got - ref| <= ((1 + u)^d - 1) * (sum |terms|)  ~=  d * u * (|dz|^T |x| + |beta * old|),     u = 2^-24,
so d = chunk + ceil(S / G) + G + 3 bounds every form (the +3 is the product rounding and `beta * old + s`).  The check uses
c = 2 d: the factor 2 covers a matrix core that truncates instead of rounding to nearest, and the second-order term.  With S and
chunk taken from the plan, c is a few hundred at the shapes production uses, so c * u stays near 1e-5 of sum |terms|.  That is far
below the error of a dropped slab, a wrong tap, or a 1e-3 change in one channel, each of which moves an element by about
sqrt(rows) / rows of sum |terms| or more.  The bias is the column sum of the UNROUNDED dz in both modes, so its bound
uses the same d over sum |dz|.

Test infrastructure (used by tests/ only)."""
import math

import torch

WG_BLOCKS = 1536        # the build-time target of blocks per launch (ORE_WG_BLOCKS in ore_conv_wgrad.hip)
WG_T = 64               # block tile: 64 output x 64 input channels of one tap
U = 2.0 ** -24          # unit roundoff of fp32

KERNELS = ("k_wgrad", "k_wgrad3", "k_wgrad_bf<false>", "k_wgrad_bf<true>")
REDUCES = (0, 1, 4, 16)     # 0: S == 1, the kernel writes dW / db itself; else the G of k_wgrad_reduce<G>


# ---- the shape matrix of tests/test_hip_wgrad.py, (B, H, W, Cin, Cout, k); tests/test_wgrad_host.py checks that it reaches every
# (kernel, reduce) form in both modes
# the 13 classes of test_hip_train.py::test_wgrad_with_fused_bias_gradient: every mix of full / half / quarter / empty 32 x 32 wave
# parts of the 64 x 64 block tile (wg_live), unsplit and split
TILE_SHAPES = [(1, 6, 9, 32, 16, 3), (2, 40, 44, 96, 96, 3), (1, 64, 64, 128, 128, 1), (4, 30, 30, 256, 112, 1), (1, 20, 20, 128, 16, 3),
               (3, 8, 8, 112, 112, 3), (2, 8, 8, 384, 112, 3), (1, 7, 9, 20, 36, 3), (1, 7, 9, 68, 100, 1), (1, 1, 2048, 128, 4, 1),
               (2, 16, 16, 544, 384, 1), (1, 16, 16, 80, 48, 3), (1, 12, 12, 36, 20, 1)]
# 3x3 edges of the image walk: one image row, one image column, single pixels, and chunks that straddle image boundaries
# (H * W not a multiple of the chunk, B > 1)
EDGE_SHAPES = [(2, 1, 37, 64, 48, 3), (2, 29, 1, 48, 64, 3), (5, 1, 1, 32, 32, 3), (3, 13, 11, 64, 64, 3), (4, 15, 17, 96, 64, 3)]
# enough rows for k_wgrad_reduce<16> (S >= 64), and the Linear-over-rows class (1x1, Cin 1024)
LARGE_SHAPES = [(2, 64, 64, 112, 112, 3), (1, 160, 160, 64, 128, 1), (1, 1, 96, 1024, 128, 1), (2, 30, 40, 1024, 128, 1)]
MATRIX = TILE_SHAPES + EDGE_SHAPES + LARGE_SHAPES
# capped workspace: workspace_floats = cap slabs (+ half a slab, the division floors) forces S = cap in both modes on this shape
# (ceil(M / 17) = 512 rows is a multiple of both chunk granules, so the rounding to 16 / 32 rows keeps S = 17)
CAP_SHAPE = (1, 68, 128, 112, 112)
CAPS = (1, 2, 3, 17)
# argument semantics (channel slices, NaN around the views, beta, db on / off, determinism): every reduce form of every kernel
SEMANTICS_SHAPES = [(1, 6, 9, 32, 16, 3), (1, 20, 20, 128, 16, 3), (2, 40, 44, 96, 96, 3), (2, 64, 64, 112, 112, 3),
                    (1, 1, 96, 1024, 128, 1), (1, 12, 12, 36, 20, 1), (1, 64, 64, 128, 128, 1), (1, 160, 160, 64, 128, 1)]


def _cdiv(a, b):
    return -(-a // b)


def wgrad_kernel(k, bf16):
    """The kernel ore_conv2d_wgrad_bias_fwd launches for a k x k convolution."""
    if bf16:
        return "k_wgrad_bf<true>" if k == 3 else "k_wgrad_bf<false>"
    return "k_wgrad3" if k == 3 else "k_wgrad"


def wgrad_tiles(Cin, Cout, k):
    """Blocks of one row split: k_wgrad3 / k_wgrad_bf<true> own the three dx taps of one kernel row per block."""
    return _cdiv(Cout, WG_T) * _cdiv(Cin, WG_T) * (3 if k == 3 else k * k)


def slab_floats(Cin, Cout, k):
    """One slab: the weight part plus the bias part, whether or not a bias gradient is asked for."""
    return Cout * k * k * Cin + Cout


def wgrad_split(M, Cin, Cout, k):
    """The row split the default workspace is sized for (ore_conv_wgrad_workspace_floats = slab_floats * this)."""
    return max(1, min(_cdiv(WG_BLOCKS, wgrad_tiles(Cin, Cout, k)), _cdiv(M, 128)))


def wgrad_plan(M, Cin, Cout, k, bf16, workspace_floats=None, bias=True):
    """(S, chunk, reduce) of one launch over M rows: S row splits of `chunk` rows (the last one shorter), and the G of the
    k_wgrad_reduce<G> that sums the S slabs (0 when S == 1: the kernel writes dW / db itself).  A workspace smaller than the
    default caps S at workspace_floats // slab_floats; `bias` (a bias gradient is asked for) enters the reduce choice through the
    number of floats the reduce sums."""
    S = wgrad_split(M, Cin, Cout, k)
    if workspace_floats is not None:
        S = min(S, workspace_floats // slab_floats(Cin, Cout, k))
    if S < 1:
        raise ValueError("workspace too small")
    step = 32 if bf16 else 16
    chunk = _cdiv(_cdiv(M, S), step) * step
    S = _cdiv(M, chunk)
    if S == 1:
        return S, chunk, 0
    quads = (Cout * k * k * Cin + (Cout if bias else 0)) // 4
    if S >= 64 and quads <= 65536:
        return S, chunk, 16
    return S, chunk, 4 if S >= 16 else 1


def rounding_depth(plan):
    """d of the module docstring: the longest chain of fp32 roundings behind one output element."""
    S, chunk, G = plan
    G = max(G, 1)
    return chunk + _cdiv(S, G) + G + 3


def bound_c(plan):
    return 2.0 * rounding_depth(plan)


def bf16_rne(t):
    """fp32 -> bf16 -> fp32, round to nearest even, as to_bf16x4 in the kernels (finite inputs)."""
    u = t.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    u = torch.where(u >= 2 ** 31, u - 2 ** 32, u)
    return u.to(torch.int32).view(torch.float32)


def scaled_operands(B, H, W, Cin, Cout, seed, device="cpu", lo=-3.0, hi=3.0):
    """x [B,H,W,Cin], dz [B,H,W,Cout] fp32 with per-channel scales 10^U(lo, hi) on both: an error in a small channel is then visible
    in the element-wise bound while a max-norm over the tensor would not see it.  Drawn on `device`."""
    g = torch.Generator(device=device).manual_seed(seed)
    f64 = dict(generator=g, dtype=torch.float64, device=device)
    sx = 10.0 ** (torch.rand(Cin, **f64) * (hi - lo) + lo)
    sz = 10.0 ** (torch.rand(Cout, **f64) * (hi - lo) + lo)
    x = (torch.randn(B, H, W, Cin, **f64) * sx).float()
    dz = (torch.randn(B, H, W, Cout, **f64) * sz).float()
    return x, dz


def wgrad_ref(x, dz, k, *, bf16=False, device=None):
    """float64 dW [Cout,Cin,k,k] (OIHW), db [Cout] and their bound magnitudes A = |dz|^T |x| per element, Ab = sum |dz|, from the
    fp32 operands x [B,H,W,Cin], dz [B,H,W,Cout] (NHWC, channels exactly Cin / Cout).  One GEMM per tap over the x rows shifted by
    the tap, with zeros where the tap leaves its image (each image of the batch on its own).  bf16: x and dz are rounded to bf16
    (nearest even) before the products; db is always the column sum of the unrounded dz."""
    device = device or x.device
    B, H, W, Cin = x.shape
    Cout = dz.shape[-1]
    p = k // 2
    M = B * H * W
    z32 = dz.to(device)
    xo, zo = x.to(device), z32
    if bf16:
        xo, zo = bf16_rne(xo), bf16_rne(zo)
    xp = torch.nn.functional.pad(xo.double(), (0, 0, p, p, p, p))          # zero border of every image
    z = zo.double().reshape(M, Cout)
    zt, zat = z.t(), z.abs().t()
    dw = torch.empty(Cout, Cin, k, k, dtype=torch.float64, device=device)
    aw = torch.empty_like(dw)
    for ky in range(k):
        for kx in range(k):
            xs = xp[:, ky:ky + H, kx:kx + W, :].reshape(M, Cin)
            dw[:, :, ky, kx] = zt @ xs
            aw[:, :, ky, kx] = zat @ xs.abs()
    zd = z32.double().reshape(M, Cout)
    return {"dw": dw, "db": zd.sum(0), "aw": aw, "ab": zd.abs().sum(0)}


def bound_ratio(got, want, mag, c):
    """max over elements of |got - want| / (c u mag); an element with mag == 0 must be exact (ratio inf otherwise)."""
    got = got.to(want.device, torch.float64)
    err = (got - want).abs()
    lim = c * U * mag
    bad = (err > 0) & (lim == 0)
    if bool(bad.any()) or not bool(torch.isfinite(got).all()):
        return math.inf
    r = torch.where(lim > 0, err / lim.clamp(min=1e-300), torch.zeros_like(err))
    return float(r.max()) if r.numel() else 0.0


def wgrad_check(ref, plan, dw=None, db=None, *, old_w=None, beta=0.0, old_b=None, beta_b=0.0):
    """Bound ratios {"dw": r, "db": r} of a launch's outputs (<= 1 passes).  old_w / old_b: what dW / db held before a launch with
    beta / beta_b != 0 (the expected result is beta * old + ref, the bound grows by |beta * old|)."""
    c = bound_c(plan)
    out = {}
    for name, got, old, b, want, mag in (("dw", dw, old_w, beta, ref["dw"], ref["aw"]), ("db", db, old_b, beta_b, ref["db"], ref["ab"])):
        if got is None:
            continue
        if b != 0.0:
            o = b * old.to(want.device, torch.float64)
            want, mag = want + o, mag + o.abs()
        out[name] = bound_ratio(got, want, mag, c)
    return out
