"""Restatement of the stride-2 gradient launches (csrc/ore_conv_s2grad.hip) and their float64 references.

Host plans.  `wgrad_s2_plan` and `stem1_wgrad_plan` mirror ore_conv2d_wgrad_s2_fwd / ore_stem1_wgrad_fwd: the rows M = B * Ho * Wo of dZ
are split S ways (until the grid has 1536 blocks, a split keeping at least 128 rows, capped by the workspace), a split owns `chunk`
rows (a multiple of the 16-row MFMA step), and the S slabs are summed by k_wgrad_reduce<G> (G = 16 | 4 | 1; 0: S == 1, the kernel
writes dW itself) -- the reduce launch of the stride-1 weight gradient (tests/wgrad_ref.py).  `dgrad_s2_classes` mirrors the parity
decomposition of ore_conv2d_dgrad_s2_fwd: the pixels of one (y mod 2, x mod 2) class are one GEMM with K = taps x Cout.

References.  float64, as shifted-window GEMMs over the zero-padded maps: one GEMM per tap.

The bound |got - ref| <= 2 d u A, u = 2^-24 (the idiom of wgrad_ref.py, whose `bound_ratio` is used).  A is the same sum over absolute
values (+ |beta * old|); d is the longest chain of fp32 roundings behind one output element, from the plan:
  wgrad_s2     d = chunk + ceil(S / G) + G + 3: a split adds `chunk` products in fp32 (however the matrix core orders the additions
               inside one instruction, at most one rounding per row), the reduce adds ceil(S / G) slabs per group and G group sums, +3
               for the product rounding and `beta * old + s` -- exactly wgrad_ref.rounding_depth, the kernels share the structure.
  stem1_wgrad  the same + 2: the X operand (x - mean) / std is formed in fp32 with two roundings (the subtraction, the division), each a
               relative error u of the term.  A is taken over the float64 normalised values.
  dgrad_s2     d = 4 Cout + 1: no row split and no reduce; an output adds at most 4 taps x Cout products in one fp32 accumulator chain (one
               rounding per product-accumulate, +1 for a product rounded on its own).  The classes with fewer taps have shorter chains;
               the bound uses the longest.
The factor 2 covers a matrix core that truncates instead of rounding to nearest, and the second-order term.  None of these figures is
tuned after a run.

Test infrastructure (used by tests/ only)."""
import torch

import wgrad_ref as WR

U = WR.U
SG_BLOCKS = 1536
SG_T = 64
SG_K = 16

# (B, H, W, Cin, Cout): H, W are the INPUT's; dZ is [B, Ho, Wo, Cout]
MATRIX = [(1, 5, 7, 16, 16), (2, 9, 12, 64, 128), (3, 1, 8, 32, 48), (2, 8, 1, 48, 32), (5, 1, 1, 32, 32), (1, 6, 6, 20, 36),
          (2, 64, 64, 64, 128),          # 2048 rows: S = 16, k_wgrad_reduce<4>
          (2, 128, 128, 64, 128)]        # 8192 rows: S = 64, k_wgrad_reduce<16>, the widest form
# a workspace of cap slabs (+ half a slab) forces S = cap: 2176 rows, ceil(2176 / 17) = 128 is a multiple of the 16-row step
CAP_SHAPE = (1, 68, 128, 64, 128)
CAPS = (1, 2, 3, 17)
SEMANTICS_SHAPES = [(1, 5, 7, 16, 16), (2, 9, 12, 64, 128), (2, 64, 64, 64, 128), (2, 128, 128, 64, 128)]
# stem_1: (B, H, W, Hp, Wp, Cout)
STEM1_MATRIX = [(b, h, w, hp, wp, co) for b in (1, 2) for (h, w, hp, wp) in ((37, 50, 64, 64), (32, 32, 32, 32), (1, 33, 2, 34))
                for co in (16, 64)] + [(1, 180, 190, 192, 192, 16)]      # 9216 rows: S = 72, k_wgrad_reduce<16>
STEM1_CAP_SHAPE = (1, 60, 66, 68, 128, 64)                               # 34 x 64 = 2176 rows
MEAN, STD = (103.53, 116.28, 123.675), (57.375, 57.12, 58.395)           # non-trivial, the detectron2 BGR statistics
REDUCES = (0, 1, 4, 16)


def _cdiv(a, b):
    return -(-a // b)


def out_hw(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def _split_plan(M, tiles, per, workspace_floats):
    S = max(1, min(_cdiv(SG_BLOCKS, tiles), _cdiv(M, 128)))
    if workspace_floats is not None:
        S = min(S, workspace_floats // per)
    if S < 1:
        raise ValueError("workspace too small")
    chunk = _cdiv(_cdiv(M, S), SG_K) * SG_K
    S = _cdiv(M, chunk)
    if S == 1:
        return S, chunk, 0
    quads = per // 4
    if S >= 64 and quads <= 65536:
        return S, chunk, 16
    return S, chunk, 4 if S >= 16 else 1


def wgrad_s2_tiles(Cin, Cout):
    return _cdiv(Cout, SG_T) * _cdiv(Cin, SG_T) * 3       # a block owns the three kx taps of one kernel row


def wgrad_s2_workspace(M, Cin, Cout):
    return Cout * 9 * Cin * max(1, min(_cdiv(SG_BLOCKS, wgrad_s2_tiles(Cin, Cout)), _cdiv(M, 128)))


def wgrad_s2_plan(M, Cin, Cout, workspace_floats=None):
    """(S, chunk, reduce) of ore_conv2d_wgrad_s2_fwd over M = B * Ho * Wo rows."""
    return _split_plan(M, wgrad_s2_tiles(Cin, Cout), Cout * 9 * Cin, workspace_floats)


def stem1_wgrad_workspace(M, Cout):
    return Cout * 27 * max(1, min(_cdiv(SG_BLOCKS, _cdiv(Cout, SG_T)), _cdiv(M, 128)))


def stem1_wgrad_plan(M, Cout, workspace_floats=None):
    """(S, chunk, reduce) of ore_stem1_wgrad_fwd over M = B * Hp/2 * Wp/2 rows."""
    return _split_plan(M, _cdiv(Cout, SG_T), Cout * 27, workspace_floats)


def wgrad_depth(plan, extra=0):
    return WR.rounding_depth(plan) + extra


STEM1_EXTRA = 2       # the roundings of (x - mean) / std


def dgrad_depth(Cout):
    return 4 * Cout + 1


# the parity classes in the order the launch serves them: (py, px, [(ky, kx, doy, dox)]): pixel (2j + py, 2i + px) meets kernel tap
# (ky, kx) at output (j + doy, i + dox)
def dgrad_s2_classes():
    out = []
    for py, px in ((1, 1), (1, 0), (0, 1), (0, 0)):
        ys = [(0, 1), (2, 0)] if py else [(1, 0)]
        xs = [(0, 1), (2, 0)] if px else [(1, 0)]
        out.append((py, px, [(ky, kx, doy, dox) for ky, doy in ys for kx, dox in xs]))
    return out


def dgrad_s2_blocks(B, H, W):
    """Blocks of 64 pixels per class, in launch order."""
    return [_cdiv(B * ((H - py + 1) // 2) * ((W - px + 1) // 2), SG_T) for py, px, _ in dgrad_s2_classes()]


def operands(B, H, W, Cin, Cout, seed, device="cpu"):
    """x [B,H,W,Cin], dz [B,Ho,Wo,Cout] with per-channel scales 1e-3 .. 1e3 (wgrad_ref.scaled_operands)."""
    Ho, Wo = out_hw(H, W)
    x, dz = WR.scaled_operands(B, H, W, Cin, Cout, seed, device=device)
    return x, dz[:, :Ho, :Wo].contiguous()


def scaled_weight(Cout, Cin, seed, device="cpu"):
    """w [Cout,Cin,3,3] fp32 with per-input-channel scales 1e-3 .. 1e3."""
    g = torch.Generator(device=device).manual_seed(seed)
    f64 = dict(generator=g, dtype=torch.float64, device=device)
    s = 10.0 ** (torch.rand(Cin, **f64) * 6.0 - 3.0)
    return (torch.randn(Cout, Cin, 3, 3, **f64) * s.view(1, Cin, 1, 1)).float()


def wgrad_s2_ref(x, dz, *, device=None, drop_tap=None, drop_rows=None):
    """float64 dW [Cout,Cin,3,3] and A = |dz|^T |x| of the 3x3 / stride 2 / pad 1 conv, from x [B,H,W,Cin] and dz [B,Ho,Wo,Cout] (fp32 or
    float64 values).  drop_tap = (ky, kx) / drop_rows = (m0, m1): fault injection for the host tests -- that tap, or those dZ rows (a
    slab), left out of "dw" (not of "aw")."""
    device = device or x.device
    B, H, W, Cin = x.shape
    Ho, Wo = out_hw(H, W)
    assert tuple(dz.shape[:3]) == (B, Ho, Wo)
    Cout = dz.shape[-1]
    M = B * Ho * Wo
    xp = torch.nn.functional.pad(x.to(device).double(), (0, 0, 1, 1, 1, 1))
    z = dz.to(device).double().reshape(M, Cout)
    zg = z
    if drop_rows is not None:
        zg = z.clone()
        zg[drop_rows[0]:drop_rows[1]] = 0
    dw = torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64, device=device)
    aw = torch.zeros_like(dw)
    for ky in range(3):
        for kx in range(3):
            xs = xp[:, ky:ky + 2 * Ho - 1:2, kx:kx + 2 * Wo - 1:2, :].reshape(M, Cin)
            if drop_tap != (ky, kx):
                dw[:, :, ky, kx] = zg.t() @ xs
            aw[:, :, ky, kx] = z.abs().t() @ xs.abs()
    return {"dw": dw, "aw": aw}


def dgrad_s2_ref(dz, w, H, W, *, device=None):
    """float64 dX [B,H,W,Cin] and A = |dz| * |w| of the same conv, from dz [B,Ho,Wo,Cout] and w [Cout,Cin,3,3]: one GEMM per tap, scattered
    to the input pixels 2 o + k - 1 of the padded map."""
    device = device or dz.device
    B, Ho, Wo, Cout = dz.shape
    assert (Ho, Wo) == out_hw(H, W)
    Cin = w.shape[1]
    z = dz.to(device).double().reshape(-1, Cout)
    wd = w.to(device).double()
    dx = torch.zeros(B, H + 2, W + 2, Cin, dtype=torch.float64, device=device)
    ax = torch.zeros_like(dx)
    for ky in range(3):
        for kx in range(3):
            dx[:, ky:ky + 2 * Ho - 1:2, kx:kx + 2 * Wo - 1:2] += (z @ wd[:, :, ky, kx]).view(B, Ho, Wo, Cin)
            ax[:, ky:ky + 2 * Ho - 1:2, kx:kx + 2 * Wo - 1:2] += (z.abs() @ wd[:, :, ky, kx].abs()).view(B, Ho, Wo, Cin)
    return {"dx": dx[:, 1:H + 1, 1:W + 1].contiguous(), "ax": ax[:, 1:H + 1, 1:W + 1].contiguous()}


def dgrad_s2_by_parity(dz, w, H, W, *, wrong_class=None):
    """float64 dX by the kernel's parity decomposition (dgrad_s2_classes), class by class.  wrong_class = (py, px): fault injection -- the
    pixels of that class take the taps of the class with the other x parity."""
    B, Ho, Wo, Cout = dz.shape
    Cin = w.shape[1]
    zp = torch.nn.functional.pad(dz.double(), (0, 0, 0, 1, 0, 1))          # one zero row / column behind the map: output index Ho / Wo
    wd = w.double()
    dx = torch.zeros(B, H, W, Cin, dtype=torch.float64)
    classes = dgrad_s2_classes()
    for py, px, taps in classes:
        Hc, Wc = (H - py + 1) // 2, (W - px + 1) // 2
        if Hc == 0 or Wc == 0:
            continue
        if wrong_class == (py, px):
            taps = [t for qy, qx, t in classes if (qy, qx) == (py, 1 - px)][0]
        acc = torch.zeros(B, Hc, Wc, Cin, dtype=torch.float64)
        for ky, kx, doy, dox in taps:
            acc += zp[:, doy:doy + Hc, dox:dox + Wc, :] @ wd[:, :, ky, kx]
        dx[:, py::2, px::2] = acc
    return dx


def normalised(img, mean, std, Hp, Wp):
    """float64 NHWC [B,Hp,Wp,3] of ((img - mean) / std) zero-padded to (Hp, Wp); mean / std as the fp32 values the kernel is handed."""
    m = torch.tensor(mean, dtype=torch.float32).double().view(1, 3, 1, 1)
    s = torch.tensor(std, dtype=torch.float32).double().view(1, 3, 1, 1)
    xn = (img.double() - m) / s
    B, _, H, W = img.shape
    xn = torch.nn.functional.pad(xn, (0, Wp - W, 0, Hp - H))
    return xn.permute(0, 2, 3, 1).contiguous()


def stem1_wgrad_ref(img, mean, std, Hp, Wp, dz, **kw):
    """float64 dW [Cout,3,3,3] of stem_1 from the raw planar image [B,3,H,W] (uint8 or fp32) and dz [B,Hp/2,Wp/2,Cout]."""
    return wgrad_s2_ref(normalised(img.cpu(), mean, std, Hp, Wp), dz, **kw)


def stem1_image(B, H, W, u8, seed, device="cpu"):
    g = torch.Generator(device=device).manual_seed(seed)
    if u8:
        return torch.randint(0, 256, (B, 3, H, W), generator=g, device=device, dtype=torch.uint8)
    return torch.rand(B, 3, H, W, generator=g, device=device) * 255.0


def scaled_dz(B, Ho, Wo, Cout, seed, device="cpu"):
    return WR.scaled_operands(B, Ho, Wo, 4, Cout, seed, device=device)[1]


def check(got, want, mag, depth, *, old=None, beta=0.0):
    """Bound ratio (<= 1 passes) of `got` against want (+ beta * old), magnitudes mag (+ |beta * old|), c = 2 * depth."""
    if beta != 0.0:
        o = beta * old.to(want.device, torch.float64)
        want, mag = want + o, mag + o.abs()
    return WR.bound_ratio(got.reshape(want.shape), want, mag, 2.0 * depth)


def log_ratios(ratios, env="ORE_S2GRAD_LOG"):
    """Print the largest bound ratio per form, and append the lines to the file ORE_S2GRAD_LOG names."""
    import os
    lines = [f"{form:14s} reduce {G:2d}  max |got-ref|/bound {r:.3e}  ({n} checks)" for (form, G), (r, n) in sorted(ratios.items())]
    print("\n" + "\n".join(lines))
    log = os.environ.get(env)
    if log and lines:
        with open(log, "a") as f:
            f.write("\n".join(lines) + "\n")
