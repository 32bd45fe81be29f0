"""The conv data gradient (dX = ore_conv2d_fwd over dZ with the weights in the data-gradient layout) and its float64 reference.

Every trained conv and linear layer gets dX from ore_conv2d_fwd: the call runs over dZ [B,H,W,Cout16] (channels Cout..Cout16 zero)
with the weights packed as [Cin16][flipped tap][Cout16] (k_pack_weight mode 1 / k_pack_weight_multi), and for the 3x3 layers the
Winograd covers, also with the Winograd form of that layout.  `pack_dgrad` restates that layout, `dgrad_ref` computes dX in float64
as shifted-window GEMMs (stride 1, pad k // 2, taps flipped; with the forward epilogue for the production replay), and
`dgrad_check` holds a launch's output to two bounds.

The hard bound, every element.  An output element is a sum of K = k * k * Cin_launch products (Cin_launch = the dZ channels the
launch reads, Cout16 of the layer).  An fp32 MFMA is a k-ordered fma chain with one rounding per product (guide: "FP32-input
MFMA"); a launch with a cross-block split-K S adds S such chains of ceil(K / S) products; waves that split K inside a block add
their partial sums in a shorter chain still, so the longest chain of roundings behind one element is at most
    d = ceil(K / S) + S + 3,
the +3 covering the epilogue (x * scale, + shift, + the upsampled add).  Any summation whose longest chain of roundings is d gives
    |got - ref| <= ((1 + u)^d - 1) * (sum of |terms|)  <=  2 d u (A + E),      u = 2^-24,
with A = |dZ| * |W| (the same shifted-window GEMMs over absolute values, times |scale|) and E = |shift| + |add|; the factor 2 covers
the second-order term and a matrix core that truncates instead of rounding to nearest.  In bf16-operand mode the products of two
bf16 values are exact in fp32, so the same d holds against the reference on bf16-rounded operands (round to nearest even).

Winograd F(2x2,3x3) computes Aᵀ [sum_c (G g Gᵀ) ⊙ (Bᵀ d B)] A.  Each transform is a short chain of fp32 additions (Bᵀ d B two
roundings, G g Gᵀ four -- 0.5 * ((g0 + g2) +- g1) per axis --, Aᵀ M A four), each bounded relative to the same algorithm run on
absolute values.  So A is replaced by
    A_wino = |Aᵀ| (sum_c |G| |g| |Gᵀ| ⊙ |Bᵀ| |d| |B|) |A|
and d = Cin_launch + WINO_DEPTH + 3 with WINO_DEPTH = 10 (the channel sum is one chain of Cin_launch products, no split).

The block rms bound.  With K in the thousands, 2 d u approaches 1e-3 and cannot see a dropped 16-channel K chunk (whose error is
about sqrt(16) / K of A).  Rounding errors of a correct summation behave like a random walk: the error of an element is about
u * sqrt(sum_i s_i^2) for the partial sums s_i, which for terms of random sign is O(u A) and not O(d u A); for a matrix core that
truncates (biased errors) it is about u sqrt(d) A / 3.  So over every block of 16 output rows x 16 output channels (the MFMA
tile) the check also requires
    rms((got - ref) / (A + E))  <=  C_S * u * sqrt(d),      C_S = 1.
tests/test_dgrad_host.py shows that an fp32 fma-chain emulation (with split-K) and an fp32 Winograd emulation stay well below it at
every production K class, and that a dropped K chunk, a dropped split slab and a 1e-3 error in one block each exceed it.

Test infrastructure (used by tests/ only)."""
import math

import torch

from wgrad_ref import U, bf16_rne  # noqa: F401  (re-exported: the same unit roundoff and bf16 rounding)

C_S = 1.0
WINO_DEPTH = 10

# Winograd F(2x2,3x3) matrices (Lavin & Gray 2016), as the kernels apply them
BT = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float64)
G = torch.tensor([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], dtype=torch.float64)
AT = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=torch.float64)


def c16(n):
    return (n + 15) // 16 * 16


def pack_dgrad(w):
    """OIHW w [Cout, Cin, k, k] -> the data-gradient layout [Cin16][flipped tap][Cout16] (flat), zeros outside Cout x Cin."""
    co, ci, kh, kw = w.shape
    out = torch.zeros(c16(ci), kh * kw, c16(co), dtype=w.dtype, device=w.device)
    out[:ci, :, :co] = w.flip(2, 3).reshape(co, ci, kh * kw).permute(1, 2, 0)
    return out.reshape(-1)


def depth(K, S=1, wino_cin=None):
    """d of the module docstring: the longest chain of fp32 roundings behind one output element."""
    if wino_cin is not None:
        return wino_cin + WINO_DEPTH + 3
    return -(-K // S) + S + 3


def scaled_operands(B, H, W, Cout, Cin, k, seed, device="cpu", lo=-3.0, hi=3.0):
    """dZ [B,H,W,Cout16] fp32 (channels >= Cout exactly 0) and w [Cout,Cin,k,k] fp32, with per-channel scales 10^U(lo, hi) on the
    channels of dZ and on w's input-channel axis: the channels of dX then differ in magnitude by up to 10^(2 (hi - lo)) / 2."""
    g = torch.Generator(device=device).manual_seed(seed)
    f64 = dict(generator=g, dtype=torch.float64, device=device)
    sz = 10.0 ** (torch.rand(Cout, **f64) * (hi - lo) + lo)
    sw = 10.0 ** (torch.rand(Cin, **f64) * (hi - lo) + lo)
    dz = torch.zeros(B, H, W, c16(Cout), dtype=torch.float32, device=device)
    dz[..., :Cout] = (torch.randn(B, H, W, Cout, **f64) * sz).float()
    w = (torch.randn(Cout, Cin, k, k, **f64) * sw.view(1, Cin, 1, 1) / math.sqrt(Cout * k * k)).float()
    return dz, w


def _windows(xp, H, W, ky, kx, rows):
    """[B', H, W, C] window of the padded input at tap offset (ky, kx), as rows [n, C] (rows: an index of the B*H*W output rows)."""
    t = xp[:, ky:ky + H, kx:kx + W, :].reshape(-1, xp.shape[-1])
    return t if rows is None else t[rows]


def dgrad_ref(dz, w, *, bf16=False, device=None, images=None, rows=None, scale=None, shift=None, add=None, relu=0, wino=False):
    """float64 dX [n, Cin] (rows of [B,H,W]) and its magnitude A = |dZ| * |W| for the conv over dz [B,H,W,Cin_launch] with weights
    w [Cout,Cin,k,k] in the data-gradient orientation (dz channels >= Cout are read against zero weights).  images: compare these
    images only (a list of batch indices); rows: for k == 1, these rows of the flattened [B*H*W] only.  scale / shift / add / relu:
    the forward epilogue relu?(acc * scale + shift + add upsampled 2x nearest) of a forward-form call (the replay), with E = |shift| +
    |add| returned in A (relu: the number of leading channels the ReLU applies to).  bf16: dz and w rounded to bf16 first.
    wino: A is A_wino of the Winograd launch (module docstring) instead of |dZ| * |W|."""
    device = device or dz.device
    co, ci, k, _ = w.shape
    p = k // 2
    z, wt = dz.to(device), w.to(device)
    if bf16:
        z, wt = bf16_rne(z), bf16_rne(wt)
    if images is not None:
        z = z[images]
        if add is not None:
            add = add[images]
    B, H, W, cl = z.shape
    wd = torch.zeros(cl, ci, k, k, dtype=torch.float64, device=device)
    wd[:co] = wt.double()
    zp = torch.nn.functional.pad(z.double(), (0, 0, p, p, p, p))
    acc = mag = None
    for ky in range(k):
        for kx in range(k):
            zs = _windows(zp, H, W, ky, kx, rows)
            wk = wd[:, :, k - 1 - ky, k - 1 - kx]
            a, m = zs @ wk, zs.abs() @ wk.abs()
            acc, mag = (a, m) if acc is None else (acc + a, mag + m)
    if wino:
        mag = dgrad_wino_mag(z, wt, device=device)
    return _epilogue(acc, mag, B, H, W, rows, scale, shift, add, relu)


def _epilogue(acc, mag, B, H, W, rows, scale, shift, add, relu):
    dev = acc.device
    if scale is not None:
        s = scale.to(dev).double()
        acc, mag = acc * s, mag * s.abs()
    if shift is not None:
        s = shift.to(dev).double()
        acc, mag = acc + s, mag + s.abs()
    if add is not None:
        a = add.to(dev).double()
        a = a.repeat_interleave(2, 1).repeat_interleave(2, 2)[:, :H, :W].reshape(-1, a.shape[-1])
        a = a if rows is None else a[rows]
        acc, mag = acc + a, mag + a.abs()
    if relu:
        acc = acc.clone()
        acc[:, :relu] = acc[:, :relu].clamp(min=0)        # 1-Lipschitz: |relu(got) - relu(ref)| <= |got - ref|
    return acc, mag


def wino_tiles(x):
    """x [B,H,W,C] -> the 4x4 input tiles of F(2x2,3x3) (pad 1): [B, Ht, Wt, 4, 4, C] with Ht = ceil(H / 2), Wt = ceil(W / 2)."""
    B, H, W, C = x.shape
    Ht, Wt = -(-H // 2), -(-W // 2)
    xp = torch.nn.functional.pad(x, (0, 0, 1, 2 * Wt + 1 - W, 1, 2 * Ht + 1 - H))
    t = xp.unfold(1, 4, 2).unfold(2, 4, 2)                  # [B, Ht, Wt, C, 4, 4]
    return t.permute(0, 1, 2, 4, 5, 3)


def winograd(x, g, *, absolute=False, dtype=torch.float64):
    """F(2x2,3x3) over x [B,H,W,C] with g [C, N, 3, 3] (g[c, n] is the 3x3 correlation kernel from input channel c to output n,
    in the orientation of the launched conv) -> [B,H,W,N].  absolute: every matrix and operand by its absolute value (A_wino of
    the module docstring).  dtype float32 with absolute=False is an fp32 emulation of the algorithm (each transform rounds in fp32,
    the channel sum is an fp32 GEMM)."""
    B, H, W, C = x.shape
    f = (lambda t: t.abs()) if absolute else (lambda t: t)
    bt, gm, at = (f(m).to(x.device, dtype) for m in (BT, G, AT))
    d = f(wino_tiles(x.to(dtype)))                          # [B, Ht, Wt, 4, 4, C]
    V = torch.einsum("ia,ztuabc,jb->ztuijc", bt, d, bt)
    Uw = torch.einsum("ia,cnab,jb->ijcn", gm, f(g.to(dtype)), gm)   # [4, 4, C, N]
    Mt = torch.einsum("btuijc,ijcn->btuijn", V, Uw)
    Y = torch.einsum("pi,btuijn,qj->btupqn", at, Mt, at)   # [B, Ht, Wt, 2, 2, N]
    Ht, Wt = Y.shape[1], Y.shape[2]
    return Y.permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * Ht, 2 * Wt, -1)[:, :H, :W]


def dgrad_wino_mag(dz, w, *, device=None, images=None):
    """A_wino [n, Cin] for the Winograd data-gradient launch (fp32 only; the kernels have no bf16-operand build)."""
    device = device or dz.device
    z = dz.to(device)
    if images is not None:
        z = z[images]
    co, ci = w.shape[:2]
    g = torch.zeros(z.shape[-1], ci, 3, 3, dtype=torch.float64, device=device)
    g[:co] = w.to(device).double().flip(2, 3)
    return winograd(z.double(), g, absolute=True).reshape(-1, ci)


def check(got, ref, mag, d):
    """(hard ratio, rms ratio) of got [n, C] against ref / mag [n, C] (<= 1 passes both).  hard: max |got - ref| / (2 d u mag);
    rms: max over 16-row x 16-channel blocks of rms((got - ref) / mag) / (C_S u sqrt(d)).  An element with mag == 0 must be exact."""
    got = got.to(ref.device, torch.float64).reshape(ref.shape)
    if not bool(torch.isfinite(got).all()):
        return math.inf, math.inf
    err = (got - ref).abs()
    if bool(((err > 0) & (mag == 0)).any()):
        return math.inf, math.inf
    rel = torch.where(mag > 0, err / mag.clamp(min=1e-300), torch.zeros_like(err))
    hard = float(rel.max()) / (2.0 * d * U) if rel.numel() else 0.0
    n, C = rel.shape
    rp = torch.nn.functional.pad(rel, (0, c16(C) - C, 0, c16(n) - n))
    cnt = torch.nn.functional.pad(torch.ones_like(rel), (0, c16(C) - C, 0, c16(n) - n))
    ss = (rp ** 2).reshape(c16(n) // 16, 16, c16(C) // 16, 16).sum((1, 3))
    nn_ = cnt.reshape(c16(n) // 16, 16, c16(C) // 16, 16).sum((1, 3))
    rms = float((ss / nn_).sqrt().max()) / (C_S * U * math.sqrt(d))
    return hard, rms


def dgrad_check(got, ref, mag, d):
    h, r = check(got, ref, mag, d)
    return {"hard": h, "rms": r}


# ---- the shape matrix of tests/test_hip_dgrad.py ----------------------------------------------------------------------------------
# The trained conv and linear layers of configs/fsod/finetune_vovnet.yaml whose input gradient is an ore_conv2d_fwd call, as
# (Cout, Cin, k) of the layer -> the [B, H, W] maps of that call at batch 1 (640 x 640 query, 24 support crops; rows of a linear are
# [1, 1, rows]).  At batch 16 the query and support maps have 16x the images and a linear 16x the rows.
LAYERS = {
    (5, 128, 3): [(1, 80, 80), (1, 40, 40), (1, 20, 20)],          # CenterNet head prediction (agn_hm + bbox_pred as one Cout-5 conv)
    (128, 128, 3): [(1, 80, 80), (1, 40, 40), (1, 20, 20), (24, 32, 32), (24, 16, 16), (24, 8, 8)],   # FPN outputs, head tower
    (96, 96, 3): [(1, 40, 40), (24, 16, 16)],                         # OSA4 layers 1, 2
    (112, 384, 3): [(1, 20, 20), (24, 8, 8)],                         # OSA5 layer 0
    (112, 112, 3): [(1, 20, 20), (24, 8, 8)],                         # OSA5 layers 1, 2
    (384, 544, 1): [(1, 40, 40), (24, 16, 16)],                       # OSA4 concat
    (512, 720, 1): [(1, 20, 20), (24, 8, 8)],                         # OSA5 concat
    (128, 256, 1): [(1, 80, 80), (1, 1, 8192)],                       # FPN lateral 3; second-stage conv3 (256 -> 128 per ROI cell)
    (128, 384, 1): [(1, 40, 40), (24, 16, 16)],                       # FPN lateral 4
    (128, 512, 1): [(1, 20, 20), (24, 8, 8)],                         # FPN lateral 5
    (128, 128, 1): [(1, 1, 24576), (1, 1, 6144), (1, 1, 1536)],       # ViP mlp_h / mlp_w / proj at p3, p4, p5
    (64, 128, 1): [(1, 1, 24), (1, 1, 8192), (1, 1, 64)],             # ViP reweighting fc1; second-stage conv1, conv2
    (256, 64, 1): [(1, 1, 24)],                                       # ViP reweighting fc2
    (128, 8192, 1): [(1, 1, 128)],                                    # fc1 over 128 ROIs
    (2, 128, 1): [(1, 1, 128)],                                       # cls_score
    (4, 128, 1): [(1, 1, 128)],                                       # bbox_pred
}
# trained weights whose input gradient is not an ore_conv2d_fwd call, and why
NOT_DGRAD = {
    (96, 256, 3): "OSA4 layer 0: its input comes from the frozen stage 3, no input gradient is asked for",
    (384, 384, 1): "eSE fc of stage 4: EseFn's own kernels",
    (512, 512, 1): "eSE fc of stage 5: EseFn's own kernels",
    (128, 2048, 1): "fc2 of the second stage: not on the training path of this config",
    (1, 128, 3): "agn_hm: trained as rows 4 of the Cout-5 head prediction (5, 128, 3)",
    (4, 128, 3): "bbox_pred of the head: rows 0..3 of the Cout-5 head prediction (5, 128, 3)",
}


def batch16(bhw):
    B, H, W = bhw
    return (B * 16, H, W) if B > 1 or H > 1 else (1, 1, W * 16)


def matrix():
    """[(label, B, H, W, Cout, Cin, k)]: the data-gradient call of every LAYERS entry at batch 1 and 16."""
    out = []
    for (co, ci, k), maps in sorted(LAYERS.items()):
        for m in maps:
            for lab, bhw in (("bs1", m), ("bs16", batch16(m))):
                out.append((lab,) + bhw + (co, ci, k))
    return out


# edge classes: one image row / column, single pixels, odd sizes, B > 1 with 16-row blocks straddling images, and the 16-channel dZ
# of Cout 2 / 4 / 5
EDGES = [(2, 1, 37, 64, 64, 3), (2, 29, 1, 64, 64, 3), (5, 1, 1, 128, 128, 3), (3, 13, 11, 96, 96, 3), (4, 15, 17, 112, 112, 3),
         (3, 7, 9, 5, 128, 3), (1, 1, 93, 2, 128, 1), (1, 1, 77, 4, 128, 1), (2, 9, 11, 128, 384, 1), (7, 3, 5, 64, 128, 3)]
