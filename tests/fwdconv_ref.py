"""The forward conv contract (ore_conv_desc: ore_conv2d_fwd and ore_conv2d_levels_fwd) restated in float64, with its bounds.

`fwd_ref` computes, for one launch over one map or over several level-major pyramid levels, in the descriptor's order:
  prologue   xin = relu?(x * in_mul[sid] + in_add[sid]) on the real pixels, sid = level * B + b.  The padding comes after the affine: an
             out-of-image tap is 0, never in_add;
  conv       shifted-window GEMMs at any stride, pad and k in {1, 3}: Ho = (H + 2 pad - k) // stride + 1;
  epilogue   * scale[lvl * ep_stride + n] + shift[lvl * ep_stride + n], + add[b, oy >> 1, ox >> 1, n] (the addend map is
             ceil(Ho / 2) x ceil(Wo / 2)), ReLU on the channels n < relu_cout
and returns ref [rows, Cout] with mag [rows, Cout], the same computation over absolute values.  A launch is held to the two bounds
of tests/dgrad_ref.py (its docstring derives them): every element to 2 d u mag, every 16-row x 16-channel block to an rms of
C_S u sqrt(d), with d = ceil(K / S) + S + 3 from the launcher's split S (Winograd: Cin + WINO_DEPTH + 3 over A_wino).  `check`,
`depth`, `U`, `bf16_rne`, `C_S` and the Winograd magnitude are dgrad_ref's; what the forward-only features add:

Input affine, fp32 operands.  The kernel evaluates v * mul + add in fp32, as one fma or as two roundings.  Either way the operand of
the GEMM is off by at most 2 u (|x| |in_mul| + |in_add|), so that expression stands in for |xin| inside mag and d grows by 2 (the ReLU
is 1-Lipschitz and adds nothing).

Input affine, bf16 operands.  A 1-ulp fp32 difference in front of the bf16 rounding can flip it, and a flipped bf16 rounding is 2^-9
of the operand: no 2 d u bound covers that honestly.  So the bf16 cases use operands for which the affine is exact in fp32 -- x and
in_add multiples of 2^-6 below 2^6 in magnitude, in_mul a signed power of two from 2^-2 to 2^2: the product is a multiple of 2^-8 below
2^8, the sum a multiple of 2^-8 below 2^9, 17 significant bits -- the contracted and the uncontracted form then agree bit for bit, the
reference rounds the exact xin to bf16 and d is the plain one.  `affine_is_exact` is that property; tests/test_fwdconv_host.py asserts
it for every bf16 affine case of the table below.

Column sums.  A launch with d->colsum writes [tiles, Cout16]: per row tile of bm rows (ore_conv_plan's bm) the sums of the stored
values.  `colsum_check` compares the float64 sum of the tile rows with the float64 sum of ref over all pixels:
    |sum_tiles cs - sum_pixels ref| <= 2 (d + bm + 8) u * sum_pixels mag,
d for the elements themselves (sum |got - ref| <= 2 d u sum mag, also through the ReLU), bm for a tile's rows added in any order, 8 for
the xor tree over the 16 pixel lanes and the wave order.  The columns n >= Cout must be exactly 0 and the tile count must equal
ore_conv_colsum_rows.

Operands (`operands`).  x carries per-channel scales 10^U(-3, 3), so does the input-channel axis of w; scale is 10^U(-3, 3) per output
channel with about a third of the signs negative, so the output channels span about 1e6 in magnitude; shift has per-channel scales
10^U(-3, 3) of its own.  in_add and add are of the magnitude of the term they join (|x| |in_mul| per input channel, the rms of
acc * scale + shift per output channel): that is what makes an out-of-image tap that receives in_add, or an addend read one pixel off,
as large as the value it corrupts.

`cases()` is the case table of tests/test_hip_fwdconv.py: feature class x launcher, as ore_conv_plan.cpp admits them.

Test infrastructure (used by tests/ only)."""
import math

import torch

import dgrad_ref as DR
from dgrad_ref import C_S, U, WINO_DEPTH, bf16_rne, c16, check, depth  # noqa: F401  (the same bounds, re-exported)

AFFINE_DEPTH = 2        # v * mul + add in fp32: at most two roundings in front of the GEMM
COLSUM_TREE = 8         # the xor tree over the 16 pixel lanes and the wave / row-tile order


def out_hw(H, W, k, stride, pad):
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


def _cols(t, k, stride, pad, Ho, Wo):
    """t [B,H,W,C] -> the im2col matrix [B*Ho*Wo, k*k*C] in (tap, channel) order, zeros outside the image."""
    tp = torch.nn.functional.pad(t, (0, 0, pad, pad, pad, pad))
    win = [tp[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride, :] for ky in range(k) for kx in range(k)]
    return torch.cat([v.reshape(-1, t.shape[-1]) for v in win], 1)


def prologue(x, in_mul, in_add, in_relu, l, B, bf16=False):
    """float64 (xin, |xin| bound) of level l's x [B,H,W,Cin]: the input affine over sid = l * B + b, ReLU, and in bf16-operand mode the
    rounding of the (exact) result to bf16."""
    xin = x.double()
    mx = xin.abs()
    if in_mul is not None:
        m = in_mul.double()[l * B:(l + 1) * B, None, None, :]
        xin, mx = xin * m, mx * m.abs()
        if in_add is not None:
            a = in_add.double()[l * B:(l + 1) * B, None, None, :]
            xin, mx = xin + a, mx + a.abs()
        if in_relu:
            xin = xin.clamp(min=0)
    if bf16:
        xin = bf16_rne(xin.float()).double()
        mx = xin.abs()
    return xin, mx


def fwd_ref(x_rows, w, HW, B, *, stride=1, pad=None, bf16=False, scale=None, shift=None, ep_stride=0, relu_cout=0, in_mul=None,
            in_add=None, in_relu=False, add=None, wino=False):
    """float64 (ref, mag) [rows_out, Cout] of the launch over x_rows [sum_l B*H_l*W_l, Cin] (level-major; one level for ore_conv2d_fwd)
    with OIHW weights w [Cout,Cin,k,k].  scale / shift: flat, read at lvl * ep_stride + n; in_mul / in_add [L*B, Cin]; add
    [B, ceil(Ho/2), ceil(Wo/2), Cout] (one level only).  bf16: the operands of the GEMM (xin and w) rounded to bf16.  wino: mag is
    A_wino of the Winograd launch."""
    Cout, Cin, k, _ = w.shape
    pad = k // 2 if pad is None else pad
    wt = (bf16_rne(w) if bf16 else w).double()
    wm = wt.permute(2, 3, 1, 0).reshape(k * k * Cin, Cout)              # [(tap, channel), Cout]
    refs, mags, r0 = [], [], 0
    for l, (H, W) in enumerate(HW):
        n = B * H * W
        x = x_rows[r0:r0 + n].reshape(B, H, W, Cin)
        r0 += n
        xin, mx = prologue(x, in_mul, in_add, in_relu, l, B, bf16)
        Ho, Wo = out_hw(H, W, k, stride, pad)
        acc = _cols(xin, k, stride, pad, Ho, Wo) @ wm
        if wino:
            assert k == 3 and stride == 1 and pad == 1 and in_mul is None
            mag = DR.winograd(xin, wt.permute(1, 0, 2, 3), absolute=True).reshape(-1, Cout)
        else:
            mag = _cols(mx, k, stride, pad, Ho, Wo) @ wm.abs()
        sc = None if scale is None else scale.reshape(-1)[l * ep_stride:l * ep_stride + Cout]
        sh = None if shift is None else shift.reshape(-1)[l * ep_stride:l * ep_stride + Cout]
        a, m = DR._epilogue(acc, mag, B, Ho, Wo, None, sc, sh, add, relu_cout)
        refs.append(a)
        mags.append(m)
    assert r0 == x_rows.shape[0]
    return torch.cat(refs, 0), torch.cat(mags, 0)


def fwd_depth(K, S=1, *, affine=False, bf16=False, wino_cin=None):
    """d of a forward launch: dgrad_ref.depth plus the two roundings of an fp32 input affine (exact, so nothing, in bf16 mode)."""
    return depth(K, S, wino_cin=wino_cin) + (AFFINE_DEPTH if affine and not bf16 else 0)


def colsum_check(cs, ref, mag, d, bm, Cout):
    """Ratio (<= 1 passes) of the column sums cs [tiles, Cout16] against ref / mag [rows, Cout]; inf where a column n >= Cout is not
    exactly 0 or a sum is not finite."""
    cs = cs.to(ref.device, torch.float64)
    if not bool(torch.isfinite(cs).all()) or bool((cs[:, Cout:] != 0).any()):
        return math.inf
    err = (cs[:, :Cout].sum(0) - ref.sum(0)).abs()
    bound = 2.0 * (d + bm + COLSUM_TREE) * U * mag.sum(0)
    if bool(((err > 0) & (bound == 0)).any()):
        return math.inf
    return float(torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.zeros_like(err)).max())


def affine_is_exact(x, in_mul, in_add, B, HW):
    """True if x * in_mul[sid] + in_add[sid] is exact in fp32 on every pixel, as a product rounded before the sum and as one fma: the
    fp32 product equals the float64 one, and so does the fp32 sum."""
    r0, ok = 0, True
    for l, (H, W) in enumerate(HW):
        n = B * H * W
        xl = x[r0:r0 + n].reshape(B, H * W, -1)
        r0 += n
        m = in_mul[l * B:(l + 1) * B, None, :]
        p32, p64 = xl * m, xl.double() * m.double()
        ok = ok and bool((p32.double() == p64).all())
        if in_add is not None:
            a = in_add[l * B:(l + 1) * B, None, :]
            ok = ok and bool(((p32 + a).double() == p64 + a.double()).all())
    return ok


def _pow10(n, g, lo=-3.0, hi=3.0):
    return 10.0 ** (torch.rand(n, generator=g, dtype=torch.float64) * (hi - lo) + lo)


def operands(c, mode):
    """The fp32 operands of case c (a dict of cases()) in `mode`, on the CPU: a dict with x [rows, Cin], w [Cout,Cin,k,k], and where the
    case has them scale / shift [L or 1, ep or Cout] (flat index lvl * ep_stride + n; entries n >= Cout are NaN), in_mul / in_add
    [L*B, Cin], add [B, ceil(Ho/2), ceil(Wo/2), Cout]."""
    g = torch.Generator().manual_seed(c["seed"])
    f64 = dict(generator=g, dtype=torch.float64)
    B, HW, Cin, Cout, k = c["B"], c["HW"], c["Cin"], c["Cout"], c["k"]
    L = len(HW)
    rows = sum(B * h * w for h, w in HW)
    exact = c["aff"] is not None and mode == "bf16"
    o = {}
    sw = _pow10(Cin, g)
    if exact:
        sx = 2.0 ** (torch.rand(Cin, **f64) * 9 - 5)                      # 2^-5 .. 2^4: |x| stays below 2^6 at 4 sigma
        o["x"] = ((torch.randn(rows, Cin, **f64) * sx * 64).round() / 64).clamp(-63, 63).float()
    else:
        sx = _pow10(Cin, g)
        o["x"] = (torch.randn(rows, Cin, **f64) * sx).float()
    o["w"] = (torch.randn(Cout, Cin, k, k, **f64) * sw.view(1, Cin, 1, 1) / math.sqrt(Cin * k * k)).float()
    amp_x = sx.clone()                                                     # rms of xin per input channel
    if c["aff"] is not None:
        sign = torch.where(torch.rand(L * B, Cin, **f64) < 0.3, -1.0, 1.0)
        if exact:
            mul = sign * 2.0 ** torch.randint(-2, 3, (L * B, Cin), generator=g).double()
        else:
            mul = sign * (torch.rand(L * B, Cin, **f64) + 0.5)
        o["in_mul"] = mul.float()
        if c["aff"] != "mul":
            a = torch.randn(L * B, Cin, **f64) * sx * mul.abs()
            if exact:
                a = ((a * 64).round() / 64).clamp(-63, 63)
            o["in_add"] = a.float()
    acc_rms = (((amp_x * sw) ** 2).sum() / Cin).sqrt()                     # rms of an accumulator, the same for every output channel
    ep = c["ep_stride"]
    width = ep if ep else c16(Cout)
    nl = L if ep else 1
    s_abs = torch.ones(nl, Cout, dtype=torch.float64)
    if c["scale"]:
        s_abs = _pow10(nl * Cout, g).reshape(nl, Cout)
        sc = torch.full((nl, width), float("nan"), dtype=torch.float64)
        sc[:, :Cout] = s_abs * torch.where(torch.rand(nl, Cout, **f64) < 0.3, -1.0, 1.0)
        o["scale"] = sc.float()
    out_rms = s_abs * acc_rms
    if c["shift"]:
        sh = torch.full((nl, width), float("nan"), dtype=torch.float64)
        sh[:, :Cout] = torch.randn(nl, Cout, **f64) * _pow10(nl * Cout, g).reshape(nl, Cout)
        o["shift"] = sh.float()
        out_rms = (out_rms ** 2 + sh[:, :Cout] ** 2).sqrt()
    if c["add"]:
        H, W = HW[0]
        Ho, Wo = out_hw(H, W, k, c["stride"], c["pad"])
        o["add"] = (torch.randn(B, (Ho + 1) // 2, (Wo + 1) // 2, Cout, **f64) * out_rms[0]).float()
    return o


def reference(c, mode, o, launcher, S):
    """(ref, mag, d) of case c with operands o on the launcher and split that ran."""
    wino = launcher.startswith("k_conv3x3_wino")
    bf16 = mode == "bf16"
    ref, mag = fwd_ref(o["x"], o["w"], c["HW"], c["B"], stride=c["stride"], pad=c["pad"], bf16=bf16, scale=o.get("scale"),
                       shift=o.get("shift"), ep_stride=c["ep_stride"], relu_cout=c["relu"], in_mul=o.get("in_mul"), in_add=o.get("in_add"),
                       in_relu=c["aff"] == "mul_add_relu", add=o.get("add"), wino=wino)
    d = fwd_depth(c["k"] * c["k"] * c["Cin"], S, affine=c["aff"] is not None, bf16=bf16, wino_cin=c["Cin"] if wino else None)
    return ref, mag, d


# ---- the case table of tests/test_hip_fwdconv.py --------------------------------------------------------------------------------------
BOTH, FP32 = ("fp32", "bf16"), ("fp32",)
# launcher -> (ore_conv_set_plan_override codes that force it, modes it has a build for).  The planner (ore_conv_plan.cpp) refuses the
# other mode: k_conv_kd, k_conv_rf and the Winograd kernels test p.bf16 themselves, plan_dma hands bf16 operands no k_conv_gs, plan_patch
# takes bf16 operands on patch<4> and ws<2,64> only.
OV = {
    "k_conv_igemm": ([(-14, 0), (-2, 0), (-1, 0)], BOTH),
    "k_conv_kw": ([(-2, 2), (-10, 0), (-12, 0), (-14, 0)], BOTH),
    "k_conv_gs": ([(-14, 0), (-4, 32, 64)], FP32),
    "k_conv_gd": ([(-12, 0), (-15, 64, 64, 4)], BOTH),
    "k_conv_kd": ([(-12, 2)], FP32),
    "k_conv_rf": ([(-14, 0), (-12, 0), (-10, 2)], FP32),
    "k_conv3x3_patch<4>": ([(-14, 0), (-2, 0), (-1, 4)], BOTH),
    "k_conv3x3_patch<8>": ([(-14, 0), (-2, 0), (-1, 8)], FP32),
    "k_conv3x3_patch_db": ([(-14, 0), (-2, 0), (-1, 16)], FP32),
    "k_conv3x3_ws<2,64>": ([(-14, 0), (-2, 0), (-1, 102)], BOTH),
    "k_conv3x3_ws<2,128>": ([(-14, 0), (-2, 0), (-1, 102)], FP32),
    "k_conv3x3_wino": ([(-7, 2)], FP32),
    "k_conv3x3_wino_nu": ([(-7, 2)], FP32),
}
DMA6 = ("k_conv_igemm", "k_conv_kw", "k_conv_gs", "k_conv_gd", "k_conv_kd", "k_conv_rf")
TILE = ("k_conv3x3_patch<4>", "k_conv3x3_patch<8>", "k_conv3x3_patch_db", "k_conv3x3_ws<2,64>", "k_conv3x3_ws<2,128>", "k_conv3x3_wino",
        "k_conv3x3_wino_nu")
TILE_CIN = {"k_conv3x3_ws<2,128>": 128, "k_conv3x3_wino_nu": 80}          # the widths that select the build; 64 for the others
LEVELS = [(9, 11), (5, 6), (3, 3)]
# Pairs the planner refuses, by class (read from ore_conv_plan.cpp); none of them is in the table, none is skipped at run time.
REFUSED = {
    "AFF, LEV+AFF beyond k_conv_igemm": "plan_dma, gd_applies, plan_patch and plan_wino decline every call with in_mul: k_conv_igemm alone "
                                        "applies the input affine",
    "ADD, COLSUM on the tile and Winograd kernels": "plan_patch and plan_wino decline c.add and c.colsum",
    "LEV 3x3 on k_conv_gd / k_conv_kd / k_conv_rf": "gd_applies / kd_applies take several levels only as a flat 1x1 GEMM with a shared "
                                                    "epilogue (ep_stride 0), rf_covers takes one level",
    "bf16 on k_conv_gs, k_conv_kd, k_conv_rf, patch<8>, patch_db, ws<2,128>, wino, wino_nu": "no bf16-operand build (plan_dma, kd_applies, "
                                                                                            "rf_covers, plan_patch, plan_wino)",
    "bf16 on k_conv_gd tiles 112 / 128 x 64": "ORE_GD_BUILDS has bf16-operand builds of 64x128, 64x64 and 32x64 only",
}
# Not refused but outside the feature table: TAIL on k_conv_gd (its forced tiles are 64 channels wide; the Cout edge inside a tile is held
# by its 40-of-64 channel cases in S2, ADD, COLSUM and LEV) and LEV on k_conv_gs (the automatic plan never sends levels there).


def _case(cls, launcher, label, *, B=2, HW, Cin, Cout, k, stride=1, pad=None, scale=True, shift=True, ep_stride=0, relu=0, aff=None,
          add=False, out_pad=(8, 8), colsum=False, splitk=0, want_S=1, levels=False, ov=None, modes=None):
    ovs, m = OV[launcher]
    return dict(cls=cls, launcher=launcher, label=label, B=B, HW=list(HW), Cin=Cin, Cout=Cout, k=k, stride=stride,
                pad=k // 2 if pad is None else pad, scale=scale, shift=shift, ep_stride=ep_stride, relu=relu, aff=aff, add=add,
                out_coff=out_pad[0], out_tail=out_pad[1], colsum=colsum, splitk=splitk, want_S=want_S, levels=levels,
                ov=ovs if ov is None else ov, modes=m if modes is None else modes, wino=launcher.startswith("k_conv3x3_wino"))


def cases():
    """Every case of the GPU module: dicts with cls, launcher, label, modes, the geometry, the features and the override codes."""
    out = []
    gd112 = [(-12, 0), (-15, 112, 64, 4)]                  # one ragged tile: M below bm (fp32 build only)
    gd128 = [(-12, 0), (-15, 128, 64, 4)]
    for la in DMA6:
        # S2: 3x3 stride 2 pad 1 at even and odd H and W, scale, shift, full ReLU
        for B, H, W in ((2, 12, 14), (1, 13, 11)):
            out.append(_case("S2", la, f"{B}x{H}x{W}", B=B, HW=[(H, W)], Cin=64, Cout=40, k=3, stride=2, relu=40))
        # ADD: nearest-2x addend at odd Ho, Wo from a slice of a wider NaN-padded map, partial ReLU; the 1x1 with a bias and a null
        # scale (the FPN lateral)
        for k in (3, 1):
            out.append(_case("ADD", la, f"k{k}", HW=[(11, 13)], Cin=64, Cout=40, k=k, relu=21, add=True, scale=k == 3))
        # COLSUM: M = 286 is no multiple of any bm, at least 3 row tiles; the 1x1 with a null shift
        for k in (3, 1):
            ov = [(-14, 0), (-12, 0), (-10, 2), (-11, 1, 4, 8)] if la == "k_conv_rf" else None      # a forced build: column sums allowed
            out.append(_case("COLSUM", la, f"k{k}", HW=[(11, 13)], Cin=64, Cout=40, k=k, relu=21, colsum=True, shift=k == 3, ov=ov))
    out.append(_case("S2", "k_conv_gd", "2x12x14 bm112", HW=[(12, 14)], Cin=64, Cout=40, k=3, stride=2, relu=40, ov=gd112, modes=FP32))
    out.append(_case("ADD", "k_conv_gd", "k1 bm112", HW=[(11, 13)], Cin=64, Cout=40, k=1, relu=21, add=True, ov=gd112, modes=FP32))
    out.append(_case("COLSUM", "k_conv_gd", "k1 bm128", HW=[(11, 13)], Cin=64, Cout=40, k=1, relu=21, colsum=True, ov=gd128, modes=FP32))
    # AFF: the three forms of the input affine, 3x3 pad 1 and 1x1, two images
    for aff in ("mul", "mul_add", "mul_add_relu"):
        for k in (3, 1):
            out.append(_case("AFF", "k_conv_igemm", f"{aff} k{k}", HW=[(7, 9)], Cin=48, Cout=24, k=k, relu=13, aff=aff))
    # TAIL: the ReLU edge and the Cout edge inside a quad; a scalar-store output (out_coff % 4 != 0; out_ld % 4 != 0 too at Cout 5 and
    # 18) and its aligned twin
    for la in ("k_conv_igemm", "k_conv_kw", "k_conv_gs", "k_conv_kd", "k_conv_rf"):
        for Cout, relu in ((5, 3), (18, 17), (67, 66)):
            ov = [(-14, 0), (-4, 64, 80)] if (la == "k_conv_gs" and Cout == 67) else None
            for lab, pads in (("scalar", (6, 7)), ("aligned", (8, (-Cout) % 4 + 4))):
                out.append(_case("TAIL", la, f"Cout{Cout} {lab}", HW=[(5, 7)], Cin=32, Cout=Cout, k=3, relu=relu, out_pad=pads, ov=ov))
    for la in TILE:
        out.append(_case("TAIL", la, "Cout64 relu61", HW=[(9, 11)], Cin=TILE_CIN.get(la, 64), Cout=64, k=3, relu=61))
    # LEV: three levels in one launch, per-level scale and shift, partial ReLU; the flat 1x1 form with a shared epilogue, on the 64-row
    # tiles with a bias alone (conv3 over the levels)
    for la in ("k_conv_igemm", "k_conv_kw"):
        out.append(_case("LEV", la, "3x3", HW=LEVELS, Cin=64, Cout=40, k=3, ep_stride=48, relu=21, levels=True))
    for la in TILE:
        out.append(_case("LEV", la, "3x3", HW=LEVELS, Cin=TILE_CIN.get(la, 64), Cout=64, k=3, ep_stride=64, relu=61, levels=True))
    out.append(_case("LEV", "k_conv_gd", "flat 1x1", HW=LEVELS, Cin=64, Cout=40, k=1, relu=21, levels=True, scale=False))
    out.append(_case("LEV", "k_conv_gd", "flat 1x1 bm112", HW=LEVELS, Cin=64, Cout=40, k=1, relu=21, levels=True, ov=gd112, modes=FP32))
    out.append(_case("LEV", "k_conv_kd", "flat 1x1", HW=LEVELS, Cin=64, Cout=40, k=1, relu=21, levels=True, scale=False))
    out.append(_case("LEV+AFF", "k_conv_igemm", "3x3 Cout5", HW=LEVELS, Cin=64, Cout=5, k=3, ep_stride=16, relu=4, aff="mul_add_relu",
                     levels=True))
    # split-K 3: the features whose epilogue runs after the slab reduction (k_conv_igemm takes the descriptor's splitk, k_conv_kw is
    # reached with splitk <= 1 only and splits by its forced tile's S)
    kw3 = [(-2, 2), (-14, 0), (-3, 16, 16, 2, 3)]
    for cls, kw in (("ADD", dict(add=True)), ("COLSUM", dict(colsum=True))):
        out.append(_case(cls + "/splitk", "k_conv_igemm", "k3 S3", HW=[(11, 13)], Cin=64, Cout=40, k=3, relu=21, splitk=3, want_S=3, ov=[], **kw))
        out.append(_case(cls + "/splitk", "k_conv_kw", "k3 S3", HW=[(11, 13)], Cin=64, Cout=40, k=3, relu=21, want_S=3, ov=kw3, **kw))
    for i, c in enumerate(out):
        c["seed"] = 100 + i
        c["id"] = f"{c['cls']}-{c['launcher']}-{c['label']}".replace(" ", "_")
    return out


def expected_cells(cs=None):
    return {(m, c["launcher"], c["cls"]) for c in (cases() if cs is None else cs) for m in c["modes"]}


# ---- the descriptor of a case ---------------------------------------------------------------------------------------------------------
IN_COFF, IN_TAIL = 16, 16           # x is channels 16 .. 16 + Cin of rows Cin + 32 wide (rows stay 64-byte multiples)
ADD_COFF, ADD_TAIL = 8, 16          # the addend is channels 8 .. 8 + Cout of a map Cout + 24 wide
GUARD = 16                          # NaN floats in front of and behind every per-channel vector (keeps 64-byte alignment)
HEAD_ROWS, TAIL_ROWS = 3, 5         # NaN rows in front of and behind every map


def geometry(c):
    """(in_ld, out_ld, add_ld, rows_in, rows_out) of case c's buffers."""
    B, k = c["B"], c["k"]
    rows_in = sum(B * h * w for h, w in c["HW"])
    rows_out = sum(B * math.prod(out_hw(h, w, k, c["stride"], c["pad"])) for h, w in c["HW"])
    return c["Cin"] + IN_COFF + IN_TAIL, c["out_coff"] + c["Cout"] + c["out_tail"], c["Cout"] + ADD_COFF + ADD_TAIL, rows_in, rows_out


def fill_desc(d, c, ptr):
    """Fill the ore_conv_desc d (orehip.ConvDesc) of case c from the addresses in ptr: in, w, out, and where the case has them scale,
    shift, in_mul, in_add, add, colsum, w_wino, workspace (with workspace_floats).  Returns the level arguments (n_levels, H, W,
    ep_stride) of ore_conv_plan / ore_conv2d_levels_fwd, n_levels = 0 for ore_conv2d_fwd."""
    in_ld, out_ld, add_ld, _, _ = geometry(c)
    d.in_, d.in_ld, d.in_coff = ptr["in"], in_ld, IN_COFF
    d.B, d.Cin, d.w = c["B"], c["Cin"], ptr["w"]
    d.H, d.W = (0, 0) if c["levels"] else c["HW"][0]
    d.Cout, d.kh, d.kw, d.stride, d.pad = c["Cout"], c["k"], c["k"], c["stride"], c["pad"]
    d.scale, d.shift, d.relu_cout = ptr.get("scale"), ptr.get("shift"), c["relu"]
    d.in_mul, d.in_add, d.in_relu = ptr.get("in_mul"), ptr.get("in_add"), int(c["aff"] == "mul_add_relu")
    if c["add"]:
        d.add, d.add_ld, d.add_coff = ptr["add"], add_ld, ADD_COFF
    d.out, d.out_ld, d.out_coff = ptr["out"], out_ld, c["out_coff"]
    d.splitk = c["splitk"]
    d.workspace, d.workspace_floats = ptr.get("workspace"), ptr.get("workspace_floats", 0)
    d.colsum, d.w_wino = ptr.get("colsum"), ptr.get("w_wino")
    if not c["levels"]:
        return 0, None, None, 0
    return len(c["HW"]), [h for h, _ in c["HW"]], [w for _, w in c["HW"]], c["ep_stride"]
