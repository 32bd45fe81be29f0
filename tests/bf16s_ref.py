"""The bf16-STORAGE conv contract (ore_conv_desc.storage = ORE_ST_BF16 / ORE_ST_BF16_F32OUT) restated in float64, with its bounds.

The operands of such a launch are bf16 VALUES -- x, w and the top-down addend; scale and shift stay fp32 -- and the kernels multiply them
with v_mfma_f32_16x16x32_bf16 into an fp32 accumulator.  A product of two bf16 numbers is exact in fp32, so float64 on the same values
is the exact result and the only error behind the fp32 value y in front of the store is the summation order: `fwdconv_ref.fwd_ref`
is the reference as it stands (its bf16 switch off: the operands are bf16 already), and y is held to the two bounds of
tests/dgrad_ref.py -- every element to 2 d u mag, every 16 x 16 block to an rms of C_S u sqrt(d) -- with d = depth(K, S) from the
split that ran and mag = |x| * |w| |scale| + |shift| + |add|.

ORE_ST_BF16_F32OUT stores y: the output is held to exactly those bounds (`check`).

ORE_ST_BF16 stores RNE_bf16(y), "rounded ONCE, nearest even" (csrc/ore_conv_epilogue.h step 5).  y itself is not observable, so the
stored tensor is held to two conditions (`store_check`), both asserted:
  window      element by element RNE(ref - bound) <= got <= RNE(ref + bound) with bound = 2 d u mag.  Rounding to nearest even is
              monotone, so a correct y inside [ref - bound, ref + bound] lands inside the window and the window has no slack term;
  round-once  the share of elements with got == RNE(ref) is at least SHARE_MIN = 0.99 per case.  With one rounding the mismatches are
              the elements whose fp32 error straddles a rounding boundary, about sqrt(d) u mag / (2^-8 |y|) of them, well under 1 % at
              these depths.  A store that truncates matches on about half the elements, one that rounds twice (through an intermediate
              precision) on about 92 %, and both stay inside most windows: the share is what sees them.  The operands are chosen so
              that an fp32 emulation stays at SHARE_EMU = 0.999 or more at every case (tests/test_bf16s_host.py asserts it).
`rne_bf16` rounds float64 straight to bf16 (through fp32 it would itself round twice).

Column sums (`colsum_check`).  By contract they are sums of the STORED tensor, so the device's [tiles, Cout16] is compared with the
float64 sum of the stored values read back from the device -- the one place where a number from the code under test enters a check:
    |sum_tiles cs - sum_rows stored| <= 2 (bm + COLSUM_TREE) u sum_rows |stored|,
bm = the plan's rows per tile (a tile's rows added in any order in fp32; the tiles are added here, in float64), COLSUM_TREE for the
xor tree over the 16 pixel lanes and the wave order.  tiles = ore_conv_colsum_rows, the columns n >= Cout are exactly 0.  Sums of the
unrounded y miss the bound by an order of magnitude (about 2^-9 |y| sqrt(rows) against (bm + 8) 2^-24 rows |y|).

Operands (`operands`): fwdconv_ref.operands -- per-channel scales 10^U(-3, 3) on x, on w's input-channel axis, on scale and on shift,
a third of the scale entries negative, the addend of the magnitude of the term it joins -- with x, w and the addend rounded to bf16.
Every value is far inside the normal range of bf16 (8 exponent bits: the range of fp32), which the host test asserts.

`cases()` is the case table of tests/test_hip_bf16s_conv.py: class x launch form as csrc/ore_conv_plan.cpp admits them.  A FORM is a
kernel build: the weight-stationary 3x3 kernel with 64 and with 128 input channels (ws_sb/64, ws_sb/128), its stride-2 build
(ws_s2), its per-level-weight form (ws_wlevel/64, /128), every SB build of k_conv_kd, every ORE_GS_BUILDS tile of k_conv_gs, and the
ten ORE_KW_TILES of k_conv_kw, each of which has an SB build (16x16, 16x32, 16x48, 16x64, 32x16, 32x32, 32x80 as the planner picks
them at M <= 2000 with k_conv_kd off, each on the smallest map that gets it; 32x64 and 16x80, its picks at M >= 4096, and 32x48, which
no shape up to 2000 rows reaches, forced).  Every
form carries PLAIN; the other classes rotate over the builds of a FAMILY (a kernel), so that each (family, class) cell the planner
admits is reached on several builds and the module stays quick.  `expected_cells` is that set, REFUSED the pairs the planner
declines, with the reason from its source.

Test infrastructure (used by tests/ only)."""
import math
import zlib

import torch

import fwdconv_ref as FR
from dgrad_ref import C_S, U, bf16_rne, c16, check, depth  # noqa: F401  (the same bounds, re-exported)

SHARE_MIN = 0.99        # the round-once share a launch must reach
SHARE_EMU = 0.999       # ... and the fp32 emulation on the same operands
COLSUM_TREE = 8         # the xor tree over the 16 pixel lanes and the wave / row-tile order
BF16_MAX = 3.3895313892515355e38      # the largest finite bf16 value
BF16_MIN_NORMAL = 2.0 ** -126


def rne_bf16(t):
    """float64 -> the nearest bf16 value (ties to even), as float64.  Finite inputs inside the normal range of bf16."""
    u = t.contiguous().view(torch.int64)
    sign = u & (-2 ** 63)
    a = u & (2 ** 63 - 1)
    a = (a + (2 ** 44 - 1) + ((a >> 45) & 1)) & ~(2 ** 45 - 1)
    return (a | sign).view(torch.float64)


def trunc_bf16(t32):
    """fp32 -> bf16 by dropping the low 16 bits (the fault, not the contract)."""
    return (t32.contiguous().view(torch.int32) & -65536).view(torch.float32)


def round_bits(t32, keep):
    """fp32 rounded (nearest even) to `keep` explicit mantissa bits: the intermediate precision of a double rounding."""
    drop = 23 - keep
    u = t32.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    u = (u + (2 ** (drop - 1) - 1) + ((u >> drop) & 1)) & ~(2 ** drop - 1) & 0xFFFFFFFF
    u = torch.where(u >= 2 ** 31, u - 2 ** 32, u)
    return u.to(torch.int32).view(torch.float32)


def store_check(got, ref, mag, d):
    """(window misses, round-once share) of the stored bf16 tensor got [rows, Cout] (any float dtype holding bf16 values) against
    ref / mag.  A non-finite element is a miss."""
    got = got.to(ref.device, torch.float64).reshape(ref.shape)
    bound = 2.0 * d * U * mag
    lo, hi = rne_bf16(ref - bound), rne_bf16(ref + bound)
    inside = torch.isfinite(got) & (got >= lo) & (got <= hi)
    misses = int((~inside).sum())
    share = float((got == rne_bf16(ref)).double().mean()) if got.numel() else 1.0
    return misses, share


def colsum_check(cs, stored, bm, Cout):
    """Ratio (<= 1 passes) of the column sums cs [tiles, Cout16] against the float64 sums of stored [rows, Cout]; inf where a column
    n >= Cout is not exactly 0 or a sum is not finite."""
    cs = cs.to(stored.device, torch.float64)
    st = stored.to(torch.float64)
    if not bool(torch.isfinite(cs).all()) or bool((cs[:, Cout:] != 0).any()):
        return math.inf
    err = (cs[:, :Cout].sum(0) - st.sum(0)).abs()
    bound = 2.0 * (bm + COLSUM_TREE) * U * st.abs().sum(0)
    if bool(((err > 0) & (bound == 0)).any()):
        return math.inf
    return float(torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.zeros_like(err)).max())


# ---- operands and reference -----------------------------------------------------------------------------------------------------------
def operands(c):
    """The operands of case c on the CPU, fp32 tensors: x [rows, Cin], w [Cout,Cin,k,k] (wlevel: [L,Cout,Cin,k,k]) and the addend
    [B, ceil(Ho/2), ceil(Wo/2), Cout] hold bf16 values; scale / shift [L or 1, ep or Cout16] are fp32 with NaN past Cout."""
    o = FR.operands(dict(c, aff=None), "fp32")
    for name in ("x", "w", "add"):
        if name in o:
            o[name] = bf16_rne(o[name])
    if c["wlevel"]:
        g = torch.Generator().manual_seed(c["seed"] + 7919)
        L, Cin, k = len(c["HW"]), c["Cin"], c["k"]
        sw = FR._pow10(Cin, g)
        w = torch.randn(L, c["Cout"], Cin, k, k, generator=g, dtype=torch.float64) * sw.view(1, 1, Cin, 1, 1) / math.sqrt(Cin * k * k)
        w[0] = o["w"].double()
        o["w"] = bf16_rne(w.float())
    return o


def reference(c, o, S):
    """(ref, mag, d) of case c with operands o at the split S that ran: float64 [rows_out, Cout]."""
    kw = dict(stride=c["stride"], pad=c["pad"], relu_cout=c["relu"])
    if c["wlevel"]:
        refs, mags, r0 = [], [], 0
        for l, (H, W) in enumerate(c["HW"]):
            n = c["B"] * H * W
            e0 = l * c["ep_stride"]
            sc = o["scale"].reshape(-1)[e0:e0 + c["Cout"]] if "scale" in o else None
            sh = o["shift"].reshape(-1)[e0:e0 + c["Cout"]] if "shift" in o else None
            r, m = FR.fwd_ref(o["x"][r0:r0 + n], o["w"][l], [(H, W)], c["B"], scale=sc, shift=sh, **kw)
            refs.append(r)
            mags.append(m)
            r0 += n
        ref, mag = torch.cat(refs, 0), torch.cat(mags, 0)
    else:
        ref, mag = FR.fwd_ref(o["x"], o["w"], c["HW"], c["B"], scale=o.get("scale"), shift=o.get("shift"), ep_stride=c["ep_stride"],
                              add=o.get("add"), **kw)
    return ref, mag, depth(c["k"] * c["k"] * c["Cin"], S)


# ---- the case table -------------------------------------------------------------------------------------------------------------------
KD_BUILDS = [(16, 16, 4, 4), (16, 16, 4, 8), (16, 16, 8, 4), (16, 16, 16, 2), (16, 32, 4, 4), (16, 32, 8, 2), (32, 32, 4, 4), (32, 32, 8, 2),
             (16, 48, 4, 4), (16, 48, 8, 2), (16, 64, 4, 2), (16, 80, 4, 2), (32, 64, 4, 2), (32, 80, 4, 2), (64, 64, 4, 2), (32, 48, 4, 2),
             (32, 16, 4, 4)]                                              # ORE_KD_BUILDS: every build has its SB twin
GS_TILES = [(64, 112), (64, 128), (64, 64), (128, 64), (128, 128), (32, 128), (128, 112), (64, 80), (32, 64)]     # ORE_GS_BUILDS
# ORE_KW_TILES, every one with an SB build (kw_build, mode 2).  KW_PLANNED: what kw_tile returns somewhere in 1024 <= M <= 2000,
# C16 <= 256 -- its table entries and its generic search (a scan of ore_conv_plan over that range finds these seven and no other);
# KW_FORCED: plan_kw's bf16-storage picks at M >= 4096, and 32x48, which that range never reaches
KW_PLANNED = [(16, 16), (16, 32), (16, 48), (16, 64), (32, 16), (32, 32), (32, 80)]
KW_FORCED = [(32, 64), (16, 80), (32, 48)]
CNT_INTS = 4096                     # ORE_CONV_CNT_INTS of include/ore_hip.h: the split-K arrival counters in front of the workspace
WS = "k_conv3x3_ws<bf16 storage>"
FAMILY_LAUNCHER = {"WS_SB64": WS, "WS_SB128": WS, "WS_S2": WS, "WS_WLEVEL": WS, "KD": "k_conv_kd", "GS": "k_conv_gs", "KW": "k_conv_kw"}
ROTATED = ("F32OUT", "SCALAR_STORE", "ADD", "COLSUM", "S2", "SLICE_IN")    # the classes every DMA-fed family takes besides PLAIN
LEVELS = [(9, 11), (5, 6), (3, 3)]
# Pairs the planner refuses (read from csrc/ore_conv_plan.cpp and conv_setup); none of them is in the table, none is skipped at run time.
REFUSED = {
    "input affine on every form": "conv_setup: bf16 storage needs 16-byte aligned input slices and no input affine (ORE_EINVAL)",
    "F32OUT, SCALAR_STORE, ADD, COLSUM on WS_SB64 / WS_SB128 / WS_S2 / WS_WLEVEL": "plan_ws_sb and plan_ws_s2 take bf16 output (sb & 2) "
        "with whole 8-byte quads only (out_ld % 4, out_coff % 4, the base 8-byte aligned) and decline c.add and c.colsum",
    "LEVELS with per-level scale / shift, WLEVEL on KD": "kd_applies declines ep_stride and takes several levels only as a flat 1x1 GEMM "
                                                          "with a shared epilogue (that form is in the table)",
    "WLEVEL outside the 64 / 128-channel 3x3 form": "conv_plan: with w_level_stride the weight-stationary bf16 kernel or ORE_EINVAL",
    "COLSUM with fp32 output on KD": "kd_applies: fp32 output of a bf16 layer with column sums is not built; k_conv_kw takes the call",
    "SPLITK on KD, GS, WS": "only k_conv_kw splits K across blocks (plan_kw)",
}
# Not refused but outside the table: LEVELS on the 64-channel weight-stationary form and on k_conv_gs (no layer of the engine; the
# 128-channel form and the per-level form WLEVEL run the same level decode), SLICE_IN on WS_S2.

# Operands are chosen so that the fp32 emulation of tests/test_bf16s_host.py reaches SHARE_EMU at every case: a case of about 1000 elements
# misses it with ONE element whose fp32 error straddles a rounding boundary.  These ids take the next seed that reaches it (the
# emulation decides, never the device).
RESEED = {"PLAIN-kd/16x16x16x2-7x3x5": 1}

IN_COFF, IN_TAIL = 16, 16           # x is channels 16 .. 16 + Cin of rows Cin + 32 wide (in_ld, in_coff % 8 == 0: conv_setup)
ADD_COFF = 8                        # the addend is channels 8 .. 8 + Cout of a map round_up(Cout + 16, 8) wide
GUARD = 16                          # NaN floats in front of and behind every per-channel vector
HEAD_ROWS, TAIL_ROWS = 3, 5         # guard rows in front of and behind every map

_EDGE = [(3, 13, 11), (2, 9, 11), (3, 7, 9), (7, 3, 5), (2, 1, 37), (2, 29, 1), (5, 1, 1), (4, 15, 17), (1, 1, 1), (1, 1, 93)]   # dgrad_ref.EDGES' maps + 1x1, 1xN
_ODD = [(3, 13, 11), (2, 9, 11), (3, 7, 9), (7, 3, 5), (4, 15, 17)]                                                            # odd H and W


def _case(cls, family, form, label, *, B, HW, Cin, Cout, k, stride=1, pad=None, scale=True, shift=True, ep_stride=0, relu=0, add=False,
          colsum=False, f32out=False, out_coff=8, out_off=0, wlevel=False, levels=False, want_S=1, ov=(), build=None):
    out_tail = 8 + (-(out_coff + Cout)) % 4                              # out_ld a multiple of 4
    return dict(cls=cls, family=family, form=form, launcher=FAMILY_LAUNCHER[family], label=label, B=B, HW=list(HW), Cin=Cin, Cout=Cout, k=k,
                stride=stride, pad=k // 2 if pad is None else pad, scale=scale, shift=shift, ep_stride=ep_stride, relu=relu, add=add,
                colsum=colsum, f32out=f32out, out_coff=out_coff, out_tail=out_tail, out_off=out_off, wlevel=wlevel, levels=levels,
                want_S=want_S, ov=list(ov), build=build, splitk=0)


def _relu_edge(Cout):
    return Cout - 3 if Cout > 4 else Cout - 1                            # inside a quad for every Cout of the table (5, 40, 112, 64, 128)


def _dma_case(cls, family, form, bn, i, ov, build):
    """Case `cls` on a DMA-fed form whose tile is bn channels wide; i rotates the maps."""
    cout_plain = {16: 5, 32: 40, 48: 40, 64: 112, 80: 112, 112: 112, 128: 128}[bn]
    cout = {16: 5, 32: 38, 48: 38}.get(bn, 110)                           # the other classes: the Cout edge inside a quad of every tile width
    B, H, W = _EDGE[i % len(_EDGE)]
    kw = dict(ov=ov, build=build)
    if cls == "PLAIN":
        return _case(cls, family, form, f"{B}x{H}x{W}", B=B, HW=[(H, W)], Cin=64, Cout=cout_plain, k=3, relu=_relu_edge(cout_plain), **kw)
    if cls == "F32OUT":
        return _case(cls, family, form, f"{B}x{H}x{W}", B=B, HW=[(H, W)], Cin=96, Cout=cout, k=1, relu=_relu_edge(cout), f32out=True, **kw)
    if cls == "SCALAR_STORE":                                            # out_coff % 4 == 2, or a base aligned to 4 bytes but not to 8
        var = dict(out_coff=6) if i % 2 == 0 else dict(out_off=2)
        return _case(cls, family, form, f"{B}x{H}x{W} {'coff6' if i % 2 == 0 else 'base4'}", B=B, HW=[(H, W)], Cin=64, Cout=cout, k=3,
                     relu=_relu_edge(cout), **var, **kw)
    if cls == "ADD":                                                     # bf16 addend from a slice of a wider map, odd Ho and Wo
        B, H, W = _ODD[i % len(_ODD)]
        k = 3 if i % 2 == 0 else 1
        return _case(cls, family, form, f"{B}x{H}x{W} k{k}", B=B, HW=[(H, W)], Cin=64, Cout=cout, k=k, relu=_relu_edge(cout), add=True,
                     scale=k == 3, **kw)
    if cls == "COLSUM":                                                  # at least two row tiles, the last one ragged (the host test checks it)
        B, H, W = (4, 15, 17) if i % 2 == 0 else (3, 13, 11)
        k = 1 if i % 2 == 0 else 3
        return _case(cls, family, form, f"{B}x{H}x{W} k{k}", B=B, HW=[(H, W)], Cin=64, Cout=cout, k=k, relu=_relu_edge(cout), colsum=True,
                     shift=k == 3, **kw)
    if cls == "S2":                                                      # 3x3 stride 2 pad 1 at odd sizes
        B, H, W = _ODD[i % len(_ODD)]
        return _case(cls, family, form, f"{B}x{H}x{W}", B=B, HW=[(H, W)], Cin=64, Cout=cout, k=3, stride=2, relu=cout, **kw)
    if cls == "SLICE_IN":                                                # Cin % 32 == 16: the last chunk of a tap reads 16 channels further
        return _case(cls, family, form, f"{B}x{H}x{W}", B=B, HW=[(H, W)], Cin=112 if i % 2 == 0 else 48, Cout=cout, k=3, relu=_relu_edge(cout), **kw)
    raise KeyError(cls)


def cases():
    """Every case of the GPU module: dicts with cls, family, form, launcher, build, label, the geometry, the features, the override codes."""
    out, cnt = [], {}

    def dma(cls, family, form, bn, ov, build):                            # a counter per class rotates the maps and the variants
        i = cnt.get(cls, 0)
        cnt[cls] = i + 1
        out.append(_dma_case(cls, family, form, bn, i, ov, build))

    # ---- the weight-stationary kernel: reached from 6000 rows (the three maps with partial 16-column and partial TH-row tiles, one
    # with an image seam), bf16 output in whole quads only
    ws = [(-8, 1), (-9, 1)]
    for fam, cin, b1 in (("WS_SB64", 64, 32), ("WS_SB128", 128, 64)):
        form = f"ws_sb/{cin}"
        one, two = dict(B=1, HW=[(77, 78)]), dict(B=2, HW=[(55, 55)])       # each form meets both maps, one of them 128 channels wide
        a, b = (one, two) if cin == 64 else (two, one)
        out.append(_case("PLAIN", fam, form, f"{a['B']}x{a['HW'][0][0]}x{a['HW'][0][1]} Cout{cin}", Cin=cin, Cout=cin, k=3, relu=cin - 3, ov=ws,
                         build=(4, 64, b1, 1), **a))
        out.append(_case("SLICE_IN", fam, form, f"{b['B']}x{b['HW'][0][0]}x{b['HW'][0][1]} Cout{192 - cin}", Cin=cin - 16, Cout=192 - cin, k=3,
                         relu=189 - cin, ov=ws, build=(4, 64, b1, 1), **b))
    # the head tower of a bf16-storage engine: three levels, shared weights, per-level scale and shift, on the 128-channel form
    out.append(_case("LEVELS", "WS_SB128", "ws_sb/128", "3 levels Cout128", B=1, HW=[(69, 71), (35, 36), (18, 18)], Cin=128, Cout=128, k=3,
                     ep_stride=128, relu=125, levels=True, ov=ws, build=(4, 64, 64, 1)))
    out.append(_case("S2", "WS_S2", "ws_s2", "1x155x157", B=1, HW=[(155, 157)], Cin=64, Cout=64, k=3, stride=2, relu=61, ov=ws, build=(2, 64, 32, 2)))
    for cin, b1 in ((64, 32), (128, 64)):
        out.append(_case("WLEVEL", "WS_WLEVEL", f"ws_wlevel/{cin}", "3 levels", B=2, HW=LEVELS, Cin=cin, Cout=cin, k=3, ep_stride=cin,
                         relu=cin - 3, wlevel=True, levels=True, ov=ws, build=(4, 64, b1, 1)))
    # ---- k_conv_kd: every SB build forced (-13); PLAIN on each, the other classes rotate
    for i, (bm, bn, nw, sb) in enumerate(KD_BUILDS):
        form, ov = f"kd/{bm}x{bn}x{nw}x{sb}", [(-13, bm, bn, nw, sb)]
        for cls in ("PLAIN", ROTATED[(2 * i) % 6], ROTATED[(2 * i + 1) % 6]):
            dma(cls, "KD", form, bn, ov, (bm, bn, nw, sb))
    # conv3 of that engine: three levels of a 1x1 layer as one flat GEMM with a shared epilogue (kd_flat)
    out.append(_case("LEVELS", "KD", "kd/32x64x4x2", "flat 1x1", B=2, HW=LEVELS, Cin=96, Cout=110, k=1, relu=107, levels=True,
                     ov=[(-13, 32, 64, 4, 2)], build=(32, 64, 4, 2)))
    # ---- k_conv_gs: every tile forced (-4; the ring stays at its default depth 3)
    for i, (bm, bn) in enumerate(GS_TILES):
        form, ov = f"gs/{bm}x{bn}", [(-4, bm, bn)]
        for cls in ("PLAIN", ROTATED[(2 * i + 1) % 6], ROTATED[(2 * i + 2) % 6]):
            dma(cls, "GS", form, bn, ov, (bm, bn))
    # ---- k_conv_kw: the planner's own tiles with k_conv_kd off (-12 0), reached by the smallest map that gets them, and two forced tiles
    kd_off = [(-12, 0)]
    out.append(_case("PLAIN", "KW", "kw/16x16", "3x13x11", B=3, HW=[(13, 11)], Cin=64, Cout=40, k=3, relu=37, ov=kd_off, build=(16, 16)))
    out.append(_case("PLAIN", "KW", "kw/16x32", "2x9x11 Cout160", B=2, HW=[(9, 11)], Cin=64, Cout=160, k=3, relu=157, ov=kd_off, build=(16, 32)))
    out.append(_case("PLAIN", "KW", "kw/16x48", "4x16x17 Cout96", B=4, HW=[(16, 17)], Cin=64, Cout=96, k=3, relu=93, ov=kd_off, build=(16, 48)))
    out.append(_case("PLAIN", "KW", "kw/32x80", "4x16x17 Cout256", B=4, HW=[(16, 17)], Cin=64, Cout=256, k=1, relu=253, ov=kd_off, build=(32, 80)))
    # kw_tile's generic search (the most FLOP per staged byte among the tiles with >= 384 blocks)
    out.append(_case("PLAIN", "KW", "kw/32x16", "4x16x17 Cout192", B=4, HW=[(16, 17)], Cin=64, Cout=192, k=3, relu=189, ov=kd_off, build=(32, 16)))
    out.append(_case("PLAIN", "KW", "kw/32x32", "4x19x20 Cout240", B=4, HW=[(19, 20)], Cin=64, Cout=240, k=3, relu=237, ov=kd_off, build=(32, 32)))
    out.append(_case("PLAIN", "KW", "kw/16x64", "3x23x23 Cout224", B=3, HW=[(23, 23)], Cin=64, Cout=224, k=3, relu=221, ov=kd_off, build=(16, 64)))
    for i, (bm, bn) in enumerate(KW_FORCED):
        dma("PLAIN", "KW", f"kw/{bm}x{bn}", bn, [(-3, bm, bn, 2, 1)], (bm, bn))
    for i, cls in enumerate(ROTATED):                                     # every rotated class on the planner's small tile and on a forced one
        dma(cls, "KW", "kw/16x16", 32, kd_off, (16, 16))
        bm, bn = KW_FORCED[i % 3]
        dma(cls, "KW", f"kw/{bm}x{bn}", bn, [(-3, bm, bn, 2, 1)], (bm, bn))
    # LEVELS: three levels, per-level scale and shift through ep_stride: the head's last conv (Cout 5, fp32 out) and a 128-channel layer
    out.append(_case("LEVELS", "KW", "kw/16x16", "Cout5 f32", B=2, HW=LEVELS, Cin=64, Cout=5, k=3, ep_stride=16, relu=3, f32out=True, levels=True,
                     ov=kd_off, build=(16, 16)))
    out.append(_case("LEVELS", "KW", "kw/16x16", "Cout128", B=2, HW=LEVELS, Cin=64, Cout=128, k=3, ep_stride=128, relu=125, levels=True,
                     ov=kd_off, build=(16, 16)))
    # SPLITK: a cross-block split of 4 at Cin 384 on a 5x7 map (the arrival counters must be back at zero)
    out.append(_case("SPLITK", "KW", "kw/16x16", "S4 Cin384", B=1, HW=[(5, 7)], Cin=384, Cout=40, k=3, relu=37, want_S=4, ov=[(-3, 16, 16, 2, 4)],
                     build=(16, 16)))
    out.append(_case("SPLITK", "KW", "kw/32x64", "S4 Cin384 colsum", B=1, HW=[(5, 7)], Cin=384, Cout=112, k=3, relu=109, want_S=4, colsum=True,
                     ov=[(-3, 32, 64, 2, 4)], build=(32, 64)))
    for c in out:
        c["id"] = f"{c['cls']}-{c['form']}-{c['label']}".replace(" ", "_")
        c["seed"] = zlib.crc32(c["id"].encode()) % 100000 + RESEED.get(c["id"], 0)      # of the id: a new case moves no other case's operands
    return out


def expected_cells(cs=None):
    return {(c["family"], c["cls"]) for c in (cases() if cs is None else cs)}


def all_forms():
    """Every launch form the table must hold."""
    return ({"ws_sb/64", "ws_sb/128", "ws_s2", "ws_wlevel/64", "ws_wlevel/128"} | {f"kd/{a}x{b}x{n}x{s}" for a, b, n, s in KD_BUILDS}
            | {f"gs/{a}x{b}" for a, b in GS_TILES} | {f"kw/{a}x{b}" for a, b in KW_PLANNED + KW_FORCED})


def plan_matches(c, pl, launchers):
    """True if the plan pl (orehip.ConvPlan) is the launch form case c names, with its split."""
    if launchers[pl.launcher] != c["launcher"] or pl.splitk != c["want_S"]:
        return False
    b = tuple(pl.build)
    fam = c["family"]
    if fam == "KD":
        return (pl.bm, pl.bn, b[0], b[1], b[2]) == c["build"] + (1,)
    if fam == "GS":
        return (pl.bm, pl.bn, b[2], b[3]) == c["build"] + (3, 1)
    if fam == "KW":
        return (pl.bm, pl.bn, b[0], b[1], b[3]) == c["build"] + (2, 4, 2)
    return (pl.bm, pl.bn, b[1], b[3]) == c["build"]


# ---- the descriptor of a case ---------------------------------------------------------------------------------------------------------
def geometry(c):
    """(in_ld, out_ld, add_ld, rows_in, rows_out) of case c's buffers, in elements of the tensor's type."""
    B, k = c["B"], c["k"]
    rows_in = sum(B * h * w for h, w in c["HW"])
    rows_out = sum(B * math.prod(FR.out_hw(h, w, k, c["stride"], c["pad"])) for h, w in c["HW"])
    return c["Cin"] + IN_COFF + IN_TAIL, c["out_coff"] + c["Cout"] + c["out_tail"], (c["Cout"] + 16 + 7) // 8 * 8, rows_in, rows_out


def packed_elems(c):
    """bf16 elements of one level's packed weights (ore_packed_weight_bf16_elems)."""
    return c16(c["Cout"]) * c["k"] * c["k"] * ((c["Cin"] + 31) // 32 * 32)


def fill_desc(d, c, ptr):
    """Fill the ore_conv_desc d (orehip.ConvDesc) of case c from the addresses in ptr: in, w, out, and where the case has them scale,
    shift, add, colsum, workspace (with workspace_floats).  Returns (n_levels, H, W, ep_stride) of ore_conv_plan /
    ore_conv2d_levels_fwd, n_levels = 0 for ore_conv2d_fwd."""
    in_ld, out_ld, add_ld, _, _ = geometry(c)
    d.in_, d.in_ld, d.in_coff = ptr["in"], in_ld, IN_COFF
    d.B, d.Cin, d.w = c["B"], c["Cin"], ptr["w"]
    d.H, d.W = (0, 0) if c["levels"] else c["HW"][0]
    d.Cout, d.kh, d.kw, d.stride, d.pad = c["Cout"], c["k"], c["k"], c["stride"], c["pad"]
    d.scale, d.shift, d.relu_cout = ptr.get("scale"), ptr.get("shift"), c["relu"]
    d.in_mul, d.in_add, d.in_relu = ptr.get("in_mul"), ptr.get("in_add"), 0
    if c["add"]:
        d.add, d.add_ld, d.add_coff = ptr["add"], add_ld, ADD_COFF
    d.out, d.out_ld, d.out_coff = ptr["out"], out_ld, c["out_coff"]
    d.splitk = c["splitk"]
    d.workspace, d.workspace_floats = ptr.get("workspace"), ptr.get("workspace_floats", 0)
    d.colsum = ptr.get("colsum")
    d.storage = 2 if c["f32out"] else 1
    d.w_level_stride = packed_elems(c) if c["wlevel"] else 0
    if not c["levels"]:
        return 0, None, None, 0
    return len(c["HW"]), [h for h, _ in c["HW"]], [w for _, w in c["HW"]], c["ep_stride"]
