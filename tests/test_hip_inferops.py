"""The inference-only non-conv kernels (csrc/ore_misc.hip, the forward of csrc/ore_roi.hip) against float64.

tests/inferops_ref.py restates each op in float64 together with the same expression over absolute values (mag) and derives the chain
depth d of every kernel; each output here is held to |got - ref| <= 2 d u mag per element and to rms((got - ref) / mag) <=
C_S u sqrt(d) per 16-row x 16-channel block (tests/test_inferops_host.py shows that fp32 emulations in the kernels' order pass both
and that the faults these kernels can have fail them).  Operands carry per-channel scales from 1e-3 to 1e3, per-image scales where
B > 1 and per-level scales where an op takes levels; GroupNorm inputs come from trainops_ref.gn_inputs; the eSE inputs keep every
pre-activation 1e-3 away from the hard-sigmoid knees.

Every launch goes through the C ABI, runs twice (the two results are compared bit for bit) and writes into NaN-filled buffers;
wherever an entry point takes ld and coff it also runs on a slice of a wider NaN-filled buffer whose bytes outside the slice must
stay untouched.  No element is left out of any comparison, except in the one stem case on the M >= 2^22 branch, whose sampling rule
is written in the test.  The bf16-storage builds that are the same template as the fp32 build (they differ in ld4 / st4 only, see
inferops_ref) must equal the fp32 build on the up-cast values bit for bit, after bf16_rne of the result where the output is bf16.

Two things the C ABI does not reach, so that no test here covers them: a kernel stride above C in the level correlation
(ore_correlation_levels_fwd fixes kstride = C) and an ore_ese_gate_pool_fwd launch with more pixel blocks than output pixels (the
launcher picks at most ceil(Ho Wo / 64) pixel blocks).

ORE_INFEROPS_LOG=<file>: append the worst hard-bound and rms ratios per op to that file; the module prints the same table at teardown."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import inferops_ref as IR
import trainops_ref as TR

pytestmark = pytest.mark.gpu

NAN = float("nan")
DEV = "cuda"
BF = torch.bfloat16
_RATIOS = {}        # op -> [worst hard, worst rms, checks]
BOX_SEEDS = (0, 1)  # per pyramid: test_inferops_host.py shows the margins for these


@pytest.fixture(scope="module")
def oh():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import orehip
    orehip.lib()
    return orehip


@pytest.fixture(scope="module", autouse=True)
def ratio_report(oh):
    yield
    lines = [f"{op:34s} max hard {h:.3e}  max rms {r:.3e}  ({n} checks)" for op, (h, r, n) in sorted(_RATIOS.items())]
    print("\n" + "\n".join(lines))
    log = os.environ.get("ORE_INFEROPS_LOG")
    if log and lines:
        with open(log, "a") as f:
            f.write("\n".join(lines) + "\n")


def _hold(op, got, ref, mag, d, what):
    """Both checks on one output; the ratios go to the report before the assertion."""
    assert got.numel() == ref.numel(), (op, what, got.shape, ref.shape)
    h, r = TR.check2(got.reshape(ref.shape), ref, mag, d)
    h0, r0, n0 = _RATIOS.get(op, (0.0, 0.0, 0))
    _RATIOS[op] = (max(h0, h), max(r0, r), n0 + 1)
    assert h <= 1 and r <= 1, (op, what, {"hard": h, "rms": r, "d": d})


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _twice(fn):
    """Run a launch twice; every output must be bit-identical (NaN borders too).  Returns the first result."""
    a, b = fn(), fn()
    ta, tb = (a, b) if isinstance(a, (tuple, list)) else ((a,), (b,))
    for x, y in zip(ta, tb):
        assert _same_bits(x, y), "two identical launches differ"
    return a


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, device=DEV, dtype=dtype)


def _sliced(v, ld, coff):
    """v [..., C] inside a NaN-filled [..., ld] buffer at channel offset coff."""
    buf = _nan(*v.shape[:-1], ld, dtype=v.dtype)
    buf[..., coff:coff + v.shape[-1]] = v
    return buf


def _outside_untouched(buf, coff, Cw):
    """The columns of buf [..., ld] outside [coff, coff + Cw) still hold the NaN they were filled with."""
    return bool(buf[..., :coff].isnan().all()) and bool(buf[..., coff + Cw:].isnan().all())


def _i32(v):
    return (C.c_int32 * len(v))(*v)


def _f32x3(v):
    return (C.c_float * 3)(*v)


# ---- stem ------------------------------------------------------------------------------------------------------------------------
def _stem(oh, img, Hp, Wp, mean, std, w, scale, shift, bf16=False, ld=None, coff=0):
    B, _, H, W = img.shape
    Cout = w.shape[0]
    ld = ld or Cout
    L = oh.lib()
    fn = L.ore_stem1_bf16_fwd if bf16 else L.ore_stem1_fwd

    def run():
        out = _nan(B, Hp // 2, Wp // 2, ld, dtype=BF if bf16 else torch.float32)
        oh._chk(fn(oh._ptr(img), int(img.dtype == torch.uint8), B, H, W, Hp, Wp, _f32x3(mean), _f32x3(std), oh._ptr(w), oh._ptr(scale),
                   oh._ptr(shift), Cout, oh._ptr(out), ld, coff, oh._stream()), "ore_stem1_fwd")
        return out
    out = _twice(run)
    assert _outside_untouched(out, coff, Cout), "wrote outside its channel slice"
    return out[..., coff:coff + Cout]


@pytest.mark.parametrize("u8", [True, False], ids=["u8", "f32"])
@pytest.mark.parametrize("case", IR.STEM_CASES, ids=str)
def test_stem(oh, case, u8):
    B, H, W, Hp, Wp, Cout = case
    img, mean, std, w, scale, shift = IR.stem_inputs(B, H, W, Cout, u8, seed=H + W, device=DEV)
    got = _stem(oh, img, Hp, Wp, mean, std, w, scale, shift)
    ref, mag = IR.stem_ref(img, Hp, Wp, mean, std, w, scale, shift)
    _hold(f"stem/NT{Cout // 16}/{'u8' if u8 else 'f32'}", got, ref, mag, IR.D_STEM, case)
    gb = _stem(oh, img, Hp, Wp, mean, std, w, scale, shift, bf16=True)
    assert torch.equal(gb.float(), TR.bf16_rne(got.contiguous())), "the bf16-output build is not the fp32 build rounded to nearest even"


def test_stem_sliced_output(oh):
    """out_ld = 96, out_coff = 16, Cout = 64: the slice equals the dense launch bit for bit, the rest of the buffer keeps its NaN."""
    B, H, W, Hp, Wp, Cout = 2, 33, 31, 34, 32, 64
    args = IR.stem_inputs(B, H, W, Cout, True, seed=5, device=DEV)
    img, rest = args[0], args[1:]
    dense = _stem(oh, img, Hp, Wp, *rest)
    assert _same_bits(_stem(oh, img, Hp, Wp, *rest, ld=96, coff=16).contiguous(), dense.contiguous())
    assert _same_bits(_stem(oh, img, Hp, Wp, *rest, bf16=True, ld=96, coff=16).contiguous(), _stem(oh, img, Hp, Wp, *rest, bf16=True).contiguous())
    ref, mag = IR.stem_ref(img, Hp, Wp, *rest)
    _hold("stem/sliced", dense, ref, mag, IR.D_STEM, "ld 96 coff 16")


def test_stem_two_groups_per_wave(oh):
    """M = 2 * 128 * 128 = 32768 output pixels = 2048 groups of 16: the launcher gives every wave two groups."""
    B, H, W, Hp, Wp, Cout = 2, 255, 256, 256, 256, 64
    assert (B * (Hp // 2) * (Wp // 2) + 15) // 16 >= 2048
    args = IR.stem_inputs(B, H, W, Cout, True, seed=6, device=DEV)
    got = _stem(oh, args[0], Hp, Wp, *args[1:])
    ref, mag = IR.stem_ref(args[0], Hp, Wp, *args[1:])
    _hold("stem/two groups per wave", got, ref, mag, IR.D_STEM, (B, H, W))


def test_stem_integer_division_branch(oh):
    """M = 17 * 500 * 500 >= 2^22: the image index comes from the integer division.  Sampling rule: every pixel of the first and of
    the last image, and of the 15 images in between every 499th output pixel of the image's flattened [Ho * Wo] (499 < Wo = 500, so
    every output row and every image is hit, at a column that moves by one per row)."""
    B, H, W, Cout, STRIDE = 17, 1000, 1000, 16, 499
    assert B * 500 * 500 >= 1 << 22
    img, mean, std, w, scale, shift = IR.stem_inputs(B, H, W, Cout, True, seed=7, device=DEV)
    got = _stem(oh, img, H, W, mean, std, w, scale, shift)
    for b in (0, B - 1):
        ref, mag = IR.stem_ref(img, H, W, mean, std, w, scale, shift, images=[b])
        _hold("stem/M >= 2^22", got[b:b + 1], ref, mag, IR.D_STEM, ("image", b))
    rows = torch.arange(0, 500 * 500, STRIDE, device=DEV)
    assert len(set((rows // 500).tolist())) == 500
    refs, mags, gots = [], [], []
    for b in range(1, B - 1):
        ref, mag = IR.stem_ref(img, H, W, mean, std, w, scale, shift, images=[b])
        refs.append(ref.reshape(-1, Cout)[rows]); mags.append(mag.reshape(-1, Cout)[rows]); gots.append(got[b].reshape(-1, Cout)[rows])
    _hold("stem/M >= 2^22", torch.cat(gots), torch.cat(refs), torch.cat(mags), IR.D_STEM, "strided images")


# ---- max-pool --------------------------------------------------------------------------------------------------------------------
def _maxpool(oh, x, mul, ld_in=None, coff_in=0, ld_out=None, coff_out=0):
    B, H, W, Cc = x.shape
    bf = x.dtype == BF
    Ho, Wo = TR.maxpool_out_hw(H, W)
    ld_in, ld_out = ld_in or Cc, ld_out or Cc
    xb = _sliced(x, ld_in, coff_in)
    fn = oh.lib().ore_maxpool3x3s2_bf16_fwd if bf else oh.lib().ore_maxpool3x3s2_fwd

    def run():
        out = _nan(B, Ho, Wo, ld_out, dtype=x.dtype)
        oh._chk(fn(oh._ptr(xb), ld_in, coff_in, B, H, W, Cc, oh._ptr(mul), oh._ptr(out), ld_out, coff_out, oh._stream()), "ore_maxpool3x3s2_fwd")
        return out
    out = _twice(run)
    assert _outside_untouched(out, coff_out, Cc)
    return out[..., coff_out:coff_out + Cc]


@pytest.mark.parametrize("case", IR.MAXPOOL_CASES, ids=str)
def test_maxpool(oh, case):
    B, H, W, Cc = case
    x = TR.scaled_inputs((B, H, W, Cc), H * W, DEV, per_image=True)
    gate = torch.rand(B, Cc, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    gate[0, 0] = 0.0
    want = TR.maxpool_fwd(x.double())                                      # float64 max of the fp32 values
    for sl in (dict(), dict(ld_in=Cc + 8, coff_in=4, ld_out=Cc + 12, coff_out=8)):
        assert torch.equal(_maxpool(oh, x, None, **sl).double(), want)
        assert torch.equal(_maxpool(oh, x, gate, **sl), want.float() * gate.view(B, 1, 1, Cc))
        xb = x.to(BF)
        wb = TR.maxpool_fwd(xb.double())
        assert torch.equal(_maxpool(oh, xb, None, **sl).double(), wb)
        assert torch.equal(_maxpool(oh, xb, gate, **sl).float(), TR.bf16_rne(wb.float() * gate.view(B, 1, 1, Cc)))


# ---- eSE -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_", IR.ESE_C)
def test_ese_gate_from_map(oh, C_):
    """ore_ese_gate_fwd (k_colsum_partial with the launcher's own P, then ese_gate16), dense and as a channel slice; the bf16 map
    against the fp32 build on the up-cast values; ore_scale_channels_fwd bit for bit against the fp32 product with that gate."""
    L, P_, S = oh.lib(), oh._ptr, oh._stream()
    for HW in IR.ESE_HW:
        for B in (1, 3):
            x, w, b = TR.ese_inputs(B, 1, HW, C_, seed=C_ + HW + B, device=DEV)
            x = x.reshape(B, HW, C_)
            ref, mag, z = IR.ese_gate_ref(x, w, b)
            assert float((z.abs() - 3.0).abs().min()) >= TR.ESE_KNEE_MARGIN
            Pn = IR.ese_plan_P(HW)
            d = IR.d_ese_colsum(HW, C_, Pn) + IR.d_ese_gate(HW, C_, Pn)
            gates = []
            for ld, coff in ((C_, 0), (C_ + 8, 4)):
                xb = _sliced(x, ld, coff)

                def run():
                    gate, ws = _nan(B, C_), _nan(B * (IR.ESE_PARTS + 1) * C_)
                    oh._chk(L.ore_ese_gate_fwd(P_(xb), ld, coff, B, HW, C_, P_(w), P_(b), P_(gate), P_(ws), S), "ore_ese_gate_fwd")
                    return gate
                gates.append(_twice(run))
                _hold("ese/gate from map", gates[-1], ref, mag, d, (C_, HW, B, ld, coff))
            assert _same_bits(gates[0], gates[1])
            x16 = x.to(BF)

            def run16(src=x16):
                gate, ws = _nan(B, C_), _nan(B * (IR.ESE_PARTS + 1) * C_)
                oh._chk(L.ore_ese_gate_bf16_fwd(P_(src), C_, 0, B, HW, C_, P_(w), P_(b), P_(gate), P_(ws), S), "ore_ese_gate_bf16_fwd")
                return gate
            x32 = x16.float()

            def run32():
                gate, ws = _nan(B, C_), _nan(B * (IR.ESE_PARTS + 1) * C_)
                oh._chk(L.ore_ese_gate_fwd(P_(x32), C_, 0, B, HW, C_, P_(w), P_(b), P_(gate), P_(ws), S), "ore_ese_gate_fwd")
                return gate
            assert _same_bits(_twice(run16), run32()), "k_colsum_partial<bf16> differs from the fp32 build on the up-cast map"
            g = gates[0]

            def scale():
                y = _nan(B, HW, C_ + 12)
                oh._chk(L.ore_scale_channels_fwd(P_(xb), C_ + 8, 4, B, HW, C_, P_(g), P_(y), C_ + 12, 8, S), "ore_scale_channels_fwd")
                return y
            y = _twice(scale)
            assert _outside_untouched(y, 8, C_) and torch.equal(y[..., 8:8 + C_], x * g.view(B, 1, C_))


@pytest.mark.parametrize("C_", IR.ESE_C)
def test_ese_gate_from_colsum(oh, C_):
    """ore_ese_gate_from_colsum_fwd on given partial sums: P so that slice 0's unrolled loop runs zero, one and two times with a
    remainder, and P > HW (the parts beyond the rows are exactly 0)."""
    L, P_, S = oh.lib(), oh._ptr, oh._stream()
    for B in (1, 3):
        for Pn in IR.ESE_P[C_]:
            for HW, empty in ((400, None), (max(Pn - 2, 1), max(Pn - 2, 1))):
                part, w, b = IR.ese_parts_inputs(B, Pn, HW, C_, seed=C_ + Pn, device=DEV, empty_from=empty)
                ref, mag, z = IR.ese_gate_from_parts_ref(part, HW, w, b)
                assert float((z.abs() - 3.0).abs().min()) >= TR.ESE_KNEE_MARGIN

                def run():
                    gate, mws = _nan(B, C_), _nan(B * C_)
                    oh._chk(L.ore_ese_gate_from_colsum_fwd(P_(part), Pn, B, HW, C_, P_(w), P_(b), P_(gate), P_(mws), S), "ore_ese_gate_from_colsum_fwd")
                    return gate
                _hold("ese/gate from colsum", _twice(run), ref, mag, IR.d_ese_gate(HW, C_, Pn), (C_, B, Pn, HW))


@pytest.mark.parametrize("C_", IR.ESE_C)
def test_ese_scaled_weight(oh, C_):
    """ore_ese_gate_scaled_weight_fwd / _bf16: the gate held to float64, the scaled columns bit for bit the fp32 product of the packed
    weight with the kernel's own gate (rounded to nearest even in the bf16 form; C % 32 == 0 there)."""
    L, P_, S = oh.lib(), oh._ptr, oh._stream()
    Pn, HW = IR.ESE_P[C_][1], 400
    part, w, b = IR.ese_parts_inputs(1, Pn, HW, C_, seed=C_, device=DEV)
    ref, mag, _ = IR.ese_gate_from_parts_ref(part, HW, w, b)
    for rows in (1, 16, 128):
        lw = TR.scaled_inputs((rows, C_), rows + C_, DEV)

        def run():
            gate, mws, out = _nan(1, C_), _nan(C_), _nan(rows + 1, C_)
            oh._chk(L.ore_ese_gate_scaled_weight_fwd(P_(part), Pn, HW, C_, P_(w), P_(b), P_(gate), P_(mws), P_(lw), rows, P_(out), S),
                    "ore_ese_gate_scaled_weight_fwd")
            return gate, out
        gate, out = _twice(run)
        _hold("ese/gate + scaled weight", gate, ref, mag, IR.d_ese_gate(HW, C_, Pn), (C_, rows))
        assert torch.equal(out[:rows], lw * gate) and bool(out[rows:].isnan().all())
        if C_ % 32 == 0:
            def run16():
                g2, mws, o2 = _nan(1, C_), _nan(C_), _nan(rows + 1, C_, dtype=BF)
                oh._chk(L.ore_ese_gate_scaled_weight_bf16_fwd(P_(part), Pn, HW, C_, P_(w), P_(b), P_(g2), P_(mws), P_(lw), rows, P_(o2), S),
                        "ore_ese_gate_scaled_weight_bf16_fwd")
                return g2, o2
            g2, o2 = _twice(run16)
            assert _same_bits(g2, gate) and torch.equal(o2[:rows].float(), TR.bf16_rne(lw * gate)) and bool(o2[rows:].isnan().all())


@pytest.mark.parametrize("H,W,C_,rows", [(1, 9, 16, 0), (9, 1, 20, 16), (2, 2, 112, 1), (23, 23, 16, 128), (3, 3, 528, 0)])
def test_ese_gate_pool_edges(oh, H, W, C_, rows):
    """ore_ese_gate_pool_fwd against the separate gate + scaled weight + max-pool entry points, bit for bit, as
    tests/test_hip_parity.py::test_ese_gate_pool_one_launch does at production sizes: one-row, one-column and 2 x 2 maps (a single
    output pixel), and 23 x 23 -> 11 x 11 = 121 output pixels in two pixel blocks of 61 and 60."""
    L, P_, S = oh.lib(), oh._ptr, oh._stream()
    HW, Pn = H * W, 5
    part, w, b = IR.ese_parts_inputs(1, Pn, HW, C_, seed=H + C_, device=DEV)
    x = TR.scaled_inputs((1, H, W, C_), H + W, DEV)
    lw = TR.scaled_inputs((rows, C_), 3, DEV) if rows else None
    Ho, Wo = TR.maxpool_out_hw(H, W)
    for dt in (torch.float32, BF):
        if dt == BF and C_ % 32:
            rows, lw = 0, None                                    # the bf16 scaled weight is built for C % 32 == 0
        xs = _sliced(x.to(dt), C_ + 8, 4)
        fn = L.ore_ese_gate_pool_bf16_fwd if dt == BF else L.ore_ese_gate_pool_fwd

        def run():
            gate, out, ws = _nan(1, C_), _nan(1, Ho, Wo, C_ + 12, dtype=dt), (_nan(rows, C_, dtype=dt) if rows else None)
            oh._chk(fn(P_(part), Pn, HW, C_, P_(w), P_(b), P_(gate), P_(lw), rows, P_(ws), P_(xs), C_ + 8, 4, H, W, P_(out), C_ + 12, 8, S),
                    "ore_ese_gate_pool_fwd")
            return (gate, out) + ((ws,) if rows else ())
        res = _twice(run)
        gate, out = res[0], res[1]
        g2, mws = _nan(1, C_), _nan(C_)
        oh._chk(L.ore_ese_gate_from_colsum_fwd(P_(part), Pn, 1, HW, C_, P_(w), P_(b), P_(g2), P_(mws), S), "ore_ese_gate_from_colsum_fwd")
        assert _same_bits(gate, g2) and _outside_untouched(out, 8, C_)
        assert _same_bits(out[..., 8:8 + C_].contiguous(), _maxpool(oh, x.to(dt), gate).contiguous())
        if rows:
            want = lw * gate
            assert torch.equal(res[2].float(), TR.bf16_rne(want) if dt == BF else want)


# ---- correlation -------------------------------------------------------------------------------------------------------------------
def _corr_kernels(Lv, Cc, seed):
    """k11 [Lv,C], k13 / k31 [Lv,C,3] with per-channel and per-level scales."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    sk = 10.0 ** (torch.rand(Lv, Cc, generator=g, device=DEV) * 2 - 1) * 10.0 ** (torch.rand(Lv, 1, generator=g, device=DEV) - 0.5)
    k11 = torch.randn(Lv, Cc, generator=g, device=DEV) * sk
    k13 = torch.randn(Lv, Cc, 3, generator=g, device=DEV) * sk.unsqueeze(-1)
    k31 = torch.randn(Lv, Cc, 3, generator=g, device=DEV) * sk.unsqueeze(-1)
    return k11.contiguous(), k13.contiguous(), k31.contiguous()


@pytest.mark.parametrize("Cc", [4, 128])
@pytest.mark.parametrize("B,H,W", IR.CORR_MAPS)
def test_correlation_single_map(oh, B, H, W, Cc):
    L, P_, S = oh.lib(), oh._ptr, oh._stream()
    q = TR.scaled_inputs((B, H, W, Cc), H * 8 + W, DEV, per_image=True)
    k11, k13, k31 = (t[0] for t in _corr_kernels(1, Cc, Cc + H))
    ref, mag = IR.corr_infer_ref(q, k11, k13, k31)
    outs = []
    for (ld, coff, old, ocoff) in ((Cc, 0, Cc, 0), (Cc + 8, 4, Cc + 12, 8)):
        qb = _sliced(q, ld, coff)

        def run():
            out = _nan(B, H, W, old)
            oh._chk(L.ore_correlation_fwd(P_(qb), ld, coff, B, H, W, Cc, P_(k11), P_(k13), P_(k31), P_(out), old, ocoff, S), "ore_correlation_fwd")
            return out
        out = _twice(run)
        assert _outside_untouched(out, ocoff, Cc)
        outs.append(out[..., ocoff:ocoff + Cc].contiguous())
        _hold("correlation/single map", outs[-1], ref, mag, IR.D_CORR_FWD, (B, H, W, Cc, ld, coff))
    assert _same_bits(outs[0], outs[1])
    # the engine's in-place form: one buffer of width 2C, the query in [C, 2C), the attention written to [0, C)
    buf = _nan(B, H, W, 2 * Cc)
    buf[..., Cc:] = q
    oh._chk(L.ore_correlation_fwd(P_(buf), 2 * Cc, Cc, B, H, W, Cc, P_(k11), P_(k13), P_(k31), P_(buf), 2 * Cc, 0, S), "ore_correlation_fwd")
    assert _same_bits(buf[..., Cc:].contiguous(), q) and _same_bits(buf[..., :Cc].contiguous(), outs[0])


@pytest.mark.parametrize("Cc", [4, 128])
@pytest.mark.parametrize("levels", IR.CORR_LEVELS, ids=str)
def test_correlation_levels(oh, levels, Cc):
    """ore_correlation_levels_fwd with its per-level kernels, B = 2, dense, sliced and in place; the bf16 build against the fp32 build
    on the up-cast query, rounded to nearest even."""
    L, P_, S = oh.lib(), oh._ptr, oh._stream()
    B, Lv = 2, len(levels)
    rows = sum(B * h * w for h, w in levels)
    lsc = torch.cat([torch.full((B * h * w, 1), 10.0 ** (l - 1.0), device=DEV) for l, (h, w) in enumerate(levels)])
    q = TR.scaled_inputs((rows, Cc), Lv + Cc, DEV) * lsc
    k11, k13, k31 = _corr_kernels(Lv, Cc, Cc + Lv)
    ref, mag = IR.corr_levels_ref(q, B, levels, k11, k13, k31)
    Hs, Ws = _i32([h for h, _ in levels]), _i32([w for _, w in levels])

    def launch(fn, qb, ld, coff, out, old, ocoff):
        oh._chk(fn(P_(qb), ld, coff, B, Lv, Hs, Ws, Cc, P_(k11), P_(k13), P_(k31), P_(out), old, ocoff, S), "ore_correlation_levels_fwd")
        return out
    outs = []
    for (ld, coff, old, ocoff) in ((Cc, 0, Cc, 0), (Cc + 8, 4, Cc + 12, 8)):
        qb = _sliced(q, ld, coff)
        out = _twice(lambda: launch(L.ore_correlation_levels_fwd, qb, ld, coff, _nan(rows, old), old, ocoff))
        assert _outside_untouched(out, ocoff, Cc)
        outs.append(out[..., ocoff:ocoff + Cc].contiguous())
        _hold("correlation/levels", outs[-1], ref, mag, IR.D_CORR_FWD, (levels, Cc, ld, coff))
    assert _same_bits(outs[0], outs[1])
    buf = _nan(rows, 2 * Cc)
    buf[..., Cc:] = q
    launch(L.ore_correlation_levels_fwd, buf, 2 * Cc, Cc, buf, 2 * Cc, 0)
    assert _same_bits(buf[..., Cc:].contiguous(), q) and _same_bits(buf[..., :Cc].contiguous(), outs[0])
    q16 = q.to(BF)
    o16 = _twice(lambda: launch(L.ore_correlation_levels_bf16_fwd, _sliced(q16, Cc + 8, 4), Cc + 8, 4, _nan(rows, Cc + 12, dtype=BF), Cc + 12, 8))
    o32 = launch(L.ore_correlation_levels_fwd, q16.float(), Cc, 0, _nan(rows, Cc), Cc, 0)
    assert _outside_untouched(o16, 8, Cc) and torch.equal(o16[..., 8:8 + Cc].float(), TR.bf16_rne(o32))


# ---- support kernels ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cc", IR.SUPPORT_C)
@pytest.mark.parametrize("s", IR.SUPPORT_S)
def test_support_kernels(oh, s, Cc):
    L, P_, S = oh.lib(), oh._ptr, oh._stream()
    proto = (TR.scaled_inputs((s, s, Cc), s + Cc, DEV) + TR.scaled_inputs((1, 1, Cc), 99, DEV)).permute(2, 0, 1).contiguous()

    def run():
        k11, k13, k31 = _nan(Cc + 1), _nan(Cc + 1, 3), _nan(Cc + 1, 3)
        oh._chk(L.ore_support_kernels_fwd(P_(proto), Cc, s, P_(k11), P_(k13), P_(k31), S), "ore_support_kernels_fwd")
        return k11, k13, k31
    got = dict(zip(("k11", "k13", "k31"), _twice(run)))
    ref = IR.support_kernels_ref(proto)
    for k in ("k11", "k13", "k31"):
        assert bool(got[k][Cc:].isnan().all())
        _hold("support_kernels", got[k][:Cc].reshape(Cc, -1), ref[k][0].reshape(Cc, -1), ref[k][1].reshape(Cc, -1), IR.d_support(s), (s, Cc, k))


# ---- GroupNorm statistics of several levels ----------------------------------------------------------------------------------------
GN_BUILD = {(128, 32): "k_gn_chunk_stats4", (64, 16): "k_gn_chunk_stats4", (32, 32): "k_gn_chunk_stats", (256, 32): "k_gn_chunk_stats"}


def _gn_levels(oh, fn, xb, ld, coff, B, HWs, Cc, G, gamma, beta):
    nseg = len(HWs) * B

    def run():
        mul, add = _nan(nseg + 1, Cc), _nan(nseg + 1, Cc)
        ws = torch.empty(sum(B * ((hw + 63) // 64) for hw in HWs) * G * 2 + 64, device=DEV)
        oh._chk(fn(oh._ptr(xb), ld, coff, B, len(HWs), _i32(HWs), Cc, G, 1e-5, oh._ptr(gamma), oh._ptr(beta), oh._ptr(mul), oh._ptr(add),
                   oh._ptr(ws), oh._stream()), "ore_groupnorm_affine_levels_fwd")
        return mul, add
    mul, add = _twice(run)
    assert bool(mul[nseg:].isnan().all()) and bool(add[nseg:].isnan().all())
    return mul[:nseg], add[:nseg]


@pytest.mark.parametrize("Cc,G", IR.GN_CG)
@pytest.mark.parametrize("HWs", IR.GN_LEVELS, ids=str)
def test_groupnorm_levels(oh, HWs, Cc, G):
    """The segment table (gn_locate_chunk) at level sizes off the 64-row chunk: every (level, image) segment against float64 with the
    depth of its own row count.  (128, 32) runs k_gn_chunk_stats4<8>, (64, 16) k_gn_chunk_stats4<4>, (32, 32) and (256, 32) the generic
    kernel -- the predicate of trainops_ref.gn_stats_kernel, which restates the launcher's."""
    assert TR.gn_stats_kernel(Cc, G) == GN_BUILD[(Cc, G)]
    assert (Cc, G) not in ((128, 32), (64, 16)) or TR.GN_ROWS * G // 256 == {(128, 32): 8, (64, 16): 4}[(Cc, G)]          # RPT
    L, B = oh.lib(), 2
    x = torch.cat([TR.gn_inputs(B, hw, Cc, G, 10 * l + Cc, DEV).reshape(B * hw, Cc) * 10.0 ** (l - 1.0) for l, hw in enumerate(HWs)])
    gamma, beta = TR.scaled_inputs((Cc,), 1, DEV, -1, 1), TR.scaled_inputs((Cc,), 2, DEV, -1, 1)
    (mr, mm), (ar, am) = IR.gn_levels_ref(x, B, HWs, G, 1e-5, gamma, beta)
    res = []
    for ld, coff in ((Cc, 0), (Cc + 8, 4)):
        mul, add = _gn_levels(oh, L.ore_groupnorm_affine_levels_fwd, _sliced(x, ld, coff), ld, coff, B, HWs, Cc, G, gamma, beta)
        res.append((mul, add))
        for l, hw in enumerate(HWs):
            sl = slice(l * B, (l + 1) * B)
            d = TR.d_gn_stats(hw, Cc, G)
            _hold(f"groupnorm levels/{GN_BUILD[(Cc, G)]}", mul[sl], mr[sl], mm[sl], d, ("mul", HWs, l, Cc, G, ld))
            _hold(f"groupnorm levels/{GN_BUILD[(Cc, G)]}", add[sl], ar[sl], am[sl], d, ("add", HWs, l, Cc, G, ld))
    assert _same_bits(res[0][0], res[1][0]) and _same_bits(res[0][1], res[1][1])
    if (Cc, G) == (128, 32):
        x16 = x.to(BF)
        m16, a16 = _gn_levels(oh, L.ore_groupnorm_affine_levels_bf16_fwd, _sliced(x16, Cc + 8, 4), Cc + 8, 4, B, HWs, Cc, G, gamma, beta)
        m32, a32 = _gn_levels(oh, L.ore_groupnorm_affine_levels_fwd, x16.float(), Cc, 0, B, HWs, Cc, G, gamma, beta)
        assert _same_bits(m16, m32) and _same_bits(a16, a32), "k_gn_chunk_stats4<8, bf16> differs from the fp32 build on the up-cast rows"


# ---- CenterNet head, last step -----------------------------------------------------------------------------------------------------
def _head(oh, fn_name, tower, ld, B, levels, w16, scale, shift, out_ld, mul=None, add=None, gn=None):
    """One of the four ore_head_pred* entry points; tower [rows, ld] (the channels from 128 on NaN), out [rows + 1, out_ld] NaN-filled."""
    L, P_, S = oh.lib(), oh._ptr, oh._stream()
    rows = tower.shape[0]
    Hs, Ws = _i32([h for h, _ in levels]), _i32([w for _, w in levels])
    ep = scale.shape[1]

    def run():
        out = _nan(rows + 1, out_ld)
        if gn is None:
            rc = getattr(L, fn_name)(P_(tower), ld, B, len(levels), Hs, Ws, P_(mul), P_(add), P_(w16), P_(scale), P_(shift), ep, P_(out), out_ld, S)
        else:
            gamma, beta = gn
            ws = torch.empty(sum(B * ((h * w + 63) // 64) for h, w in levels) * 32 * 2 + 64, device=DEV)
            rc = getattr(L, fn_name)(P_(tower), ld, B, len(levels), Hs, Ws, 32, 1e-5, P_(gamma), P_(beta), P_(w16), P_(scale), P_(shift), ep,
                                     P_(out), out_ld, P_(ws), S)
        oh._chk(rc, fn_name)
        return out
    out = _twice(run)
    assert bool(out[rows:].isnan().all()) and bool(out[:rows, 5:].isnan().all()), "wrote beyond its 5 columns or its rows"
    return out[:rows, :5].contiguous()


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("levels", IR.HEAD_LEVELS, ids=str)
def test_head_pred(oh, levels, B):
    """ore_head_pred_fwd against float64 with the folded affine as given inputs; tower ld 128 and 256 (NaN in the unread half), out_ld 5
    and 8, ep_stride 16 with distinct rows per level (NaN beyond column 5).  The weights are packed as the engine packs pred.w:
    ore_engine_finalize concatenates bbox_pred.weight and agn_hm.weight to [5, 128, 3, 3] and calls ore_pack_conv_weight_host
    (csrc/ore_engine.hip), which orehip.pack_conv_weight wraps.  The bf16 tower build against the fp32 build on the up-cast tower."""
    tower, mul, add, w5, scale, shift = IR.head_inputs(B, levels, seed=len(levels) + B, device=DEV)
    w16 = oh.pack_conv_weight(w5)
    assert w16.numel() == 16 * 9 * 128
    ref, mag = IR.head_ref(tower, B, levels, mul, add, w5, scale, shift)
    outs = []
    for ld, out_ld in ((128, 5), (256, 8), (128, 8), (256, 5)):
        got = _head(oh, "ore_head_pred_fwd", _sliced(tower, ld, 0), ld, B, levels, w16, scale, shift, out_ld, mul, add)
        _hold("head_pred", got, ref, mag, IR.D_HEAD, (levels, B, ld, out_ld))
        outs.append(got)
    assert all(_same_bits(outs[0], o) for o in outs[1:])
    t16 = tower.to(BF)
    g16 = _head(oh, "ore_head_pred_bf16_fwd", _sliced(t16, 256, 0), 256, B, levels, w16, scale, shift, 8, mul, add)
    g32 = _head(oh, "ore_head_pred_fwd", t16.float(), 128, B, levels, w16, scale, shift, 8, mul, add)
    assert _same_bits(g16, g32), "k_head_pred<bf16> differs from the fp32 build on the up-cast tower"


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("levels", IR.HEAD_LEVELS, ids=str)
def test_head_pred_gn(oh, levels, B):
    """ore_head_pred_gn_fwd / _bf16 fold the GroupNorm chunk statistics in the block through gn_combine_block, the function k_gn_combine
    itself consists of (csrc/ore_misc.hip: k_gn_combine only picks the segment and calls it), on the statistics of the same
    gn_stats_levels launch: the same arithmetic in the same order, so the result must equal, bit for bit, ore_head_pred_fwd fed with
    the mul / add of ore_groupnorm_affine_levels_fwd on the same tower."""
    L = oh.lib()
    HWs = [h * w for h, w in levels]
    tower = torch.cat([TR.gn_inputs(B, hw, 128, 32, 7 * l + B, DEV).reshape(B * hw, 128) * 10.0 ** (l - 1.0) for l, hw in enumerate(HWs)])
    _, _, _, w5, scale, shift = IR.head_inputs(B, levels, seed=11, device=DEV)
    w16 = oh.pack_conv_weight(w5)
    gamma, beta = TR.scaled_inputs((128,), 1, DEV, -1, 1), TR.scaled_inputs((128,), 2, DEV, -1, 1)
    for dt, stats_fn, pre_fn, gn_fn in ((torch.float32, L.ore_groupnorm_affine_levels_fwd, "ore_head_pred_fwd", "ore_head_pred_gn_fwd"),
                                        (BF, L.ore_groupnorm_affine_levels_bf16_fwd, "ore_head_pred_bf16_fwd", "ore_head_pred_gn_bf16_fwd")):
        tw = _sliced(tower.to(dt), 256, 0)
        mul, add = _gn_levels(oh, stats_fn, tw, 256, 0, B, HWs, 128, 32, gamma, beta)
        mul, add = mul.contiguous(), add.contiguous()
        want = _head(oh, pre_fn, tw, 256, B, levels, w16, scale, shift, 8, mul, add)
        got = _head(oh, gn_fn, tw, 256, B, levels, w16, scale, shift, 8, gn=(gamma, beta))
        assert _same_bits(got, want), (levels, B, dt)
        # and against float64 with the kernel-side affine as given inputs, on GroupNorm-shaped towers
        ref, mag = IR.head_ref(tower.to(dt).float(), B, levels, mul, add, w5, scale, shift)
        _hold("head_pred/gn", got, ref, mag, IR.D_HEAD, (levels, B, dt))


# ---- ROIAlign ------------------------------------------------------------------------------------------------------------------------
def _roi_setup(pyramid, Cc, B, seed):
    scales, ml, HWs = IR.roi_pyramid(pyramid)
    feats = [TR.scaled_inputs((B, h, w, Cc), seed + l, DEV, per_image=B > 1) * 10.0 ** (l - 1.0) for l, (h, w) in enumerate(HWs)]
    ld, coff = Cc + 8, 4
    bufs = [_sliced(f, ld, coff) for f in feats]
    return scales, ml, HWs, feats, bufs, ld, coff


def _roi_args(oh, bufs, HWs, scales, ld, coff):
    n = len(bufs)
    return ((C.c_void_p * n)(*[oh._ptr(b) for b in bufs]), _i32([ld] * n), _i32([coff] * n), _i32([h for h, _ in HWs]), _i32([w for _, w in HWs]),
            (C.c_float * n)(*scales))


def _roi_boxes(pyramid, seed):
    gen, _ = IR.roi_boxes(64, seed, pyramid)
    return np.concatenate([gen, np.array(IR.ROI_EXACT_BOXES, dtype=np.float32)])


@pytest.mark.parametrize("pyramid", list(IR.ROI_PYRAMIDS))
@pytest.mark.parametrize("Cc,P", [(c, p) for c in (4, 16, 128) for p in IR.ROI_POOLED])
def test_roi_align(oh, Cc, P, pyramid):
    """ore_roi_align_fwd with a host count on 64 generated boxes over all levels plus the exact boxes; features are ld > C slices; the
    rows from the count up to cap are zero-filled; ore_roi_align_bf16_fwd against the fp32 build on the up-cast maps."""
    L, P_, S = oh.lib(), oh._ptr, oh._stream()
    scales, ml, HWs, feats, bufs, ld, coff = _roi_setup(pyramid, Cc, 1, Cc + P)
    boxes = _roi_boxes(pyramid, BOX_SEEDS[0])
    n, cap = len(boxes), len(boxes) + 2
    bd = torch.from_numpy(boxes).to(DEV)
    a = _roi_args(oh, bufs, HWs, scales, ld, coff)

    def run(fn=L.ore_roi_align_fwd, a=a):
        out = _nan(cap + 1, P * P * Cc)
        oh._chk(fn(*a, len(scales), ml, Cc, P, P_(bd), None, n, cap, P_(out), S), "ore_roi_align_fwd")
        return out
    out = _twice(run)
    assert bool((out[n:cap] == 0).all()) and bool(out[cap:].isnan().all())
    ref, mag, d = IR.roi_align_ref(feats, scales, ml, P, boxes)
    _hold(f"roi_align/pooled {P}", out[:n], ref, mag, d, (pyramid, Cc, P))
    f16 = [f.to(BF) for f in feats]
    b16 = [_sliced(f, ld, coff) for f in f16]
    o16 = _twice(lambda: run(L.ore_roi_align_bf16_fwd, _roi_args(oh, b16, HWs, scales, ld, coff)))
    b32 = [_sliced(f.float(), ld, coff) for f in f16]
    o32 = run(L.ore_roi_align_fwd, _roi_args(oh, b32, HWs, scales, ld, coff))
    assert _same_bits(o16, o32), "k_roi_align<bf16> differs from the fp32 build on the up-cast maps"


@pytest.mark.parametrize("count", ["below", "equal", "above"])
def test_roi_align_device_count(oh, count):
    """The device-side count below, at and above cap: rows [count, cap) are exactly zero, rows from cap on are untouched, rows below
    min(count, cap) equal the host-count launch bit for bit."""
    L, P_, S = oh.lib(), oh._ptr, oh._stream()
    Cc, P, pyramid = 16, 7, "p3-5"
    scales, ml, HWs, feats, bufs, ld, coff = _roi_setup(pyramid, Cc, 1, 3)
    boxes = _roi_boxes(pyramid, BOX_SEEDS[1])
    cap = 40
    nd = {"below": 17, "equal": cap, "above": len(boxes)}[count]
    bd = torch.from_numpy(boxes).to(DEV)
    ndev = torch.tensor([nd], dtype=torch.int32, device=DEV)
    a = _roi_args(oh, bufs, HWs, scales, ld, coff)

    def run(dev=True):
        out = _nan(cap + 3, P * P * Cc)
        oh._chk(L.ore_roi_align_fwd(*a, len(scales), ml, Cc, P, P_(bd), P_(ndev) if dev else None, -1 if dev else min(nd, cap), cap, P_(out), S),
                "ore_roi_align_fwd")
        return out
    out = _twice(run)
    k = min(nd, cap)
    assert bool((out[k:cap] == 0).all()) and bool(out[cap:].isnan().all())
    assert _same_bits(out, run(dev=False))
    ref, mag, d = IR.roi_align_ref(feats, scales, ml, P, boxes[:k])
    _hold("roi_align/device count", out[:k], ref, mag, d, count)


@pytest.mark.parametrize("Cc,P,pyramid", [(16, 7, "p3-5"), (128, 8, "p3-5"), (4, 14, "p2-5"), (16, 1, "p2-5")])
def test_roi_align_batched(oh, Cc, P, pyramid):
    """ore_roi_align_batched_fwd, B = 3: box i pools image i % 3 (the boxes of one image interleaved with the others'), the maps with
    per-image scales."""
    L, P_, S = oh.lib(), oh._ptr, oh._stream()
    B = 3
    scales, ml, HWs, feats, bufs, ld, coff = _roi_setup(pyramid, Cc, B, 5)
    boxes = _roi_boxes(pyramid, BOX_SEEDS[1])
    n = len(boxes)
    bidx = [(i * 2 + 1) % B for i in range(n)]
    bd, bi = torch.from_numpy(boxes).to(DEV), torch.tensor(bidx, dtype=torch.int32, device=DEV)
    a = _roi_args(oh, bufs, HWs, scales, ld, coff)

    def run():
        out = _nan(n + 1, P * P * Cc)
        oh._chk(L.ore_roi_align_batched_fwd(*a, len(scales), ml, Cc, P, P_(bd), P_(bi), n, P_(out), S), "ore_roi_align_batched_fwd")
        return out
    out = _twice(run)
    assert bool(out[n:].isnan().all())
    ref, mag, d = IR.roi_align_ref(feats, scales, ml, P, boxes, bidx=bidx)
    _hold("roi_align/batched", out[:n], ref, mag, d, (Cc, P, pyramid))
