"""Every bf16-STORAGE conv launch form against float64, rounded once (ore_conv_desc.storage = ORE_ST_BF16 / ORE_ST_BF16_F32OUT).

The fp32-storage launchers are pinned by tests/test_hip_dgrad.py (the GEMM core) and tests/test_hip_fwdconv.py (prologue and
epilogue).  This module holds the forms that carry every conv of an ORE_CONV_BF16S engine: the weight-stationary 3x3 kernel with 64
and 128 input channels, at stride 2 and with per-level weights, every SB build of k_conv_kd, every tile of k_conv_gs and every
tile of k_conv_kw.  tests/bf16s_ref.py restates the contract in float64, derives the bounds and holds the case table (class x
form as ore_conv_plan.cpp admits them, with the refused pairs and why); tests/test_bf16s_host.py shows on the CPU that an fp32
emulation passes them and that a truncating store, a double rounding and the other faults of that list each fail one.

An fp32 output is held element by element to 2 d u mag and block by block to the rms bound.  A bf16 output is held to the window
RNE(ref - bound) <= got <= RNE(ref + bound), element by element and without slack, AND to a round-once share of at least 0.99: the
share of elements equal to RNE_bf16 of the float64 reference.  Column sums are compared with the float64 sums of the stored tensor
read back from the device (by contract they are sums of the ROUNDED values), the columns from Cout to Cout16 exactly 0.

Every case forces its form through orehip.conv_overrides (or reaches it on the smallest map the planner sends there), asserts that
conv_last_launch() and ore_conv_plan name it with the split that ran, and launches twice (bitwise equal).  Every input, addend and
output is a slice of a wider allocation with guard rows in front and behind and guard channels beside it: NaN wherever the contract
forbids a read, the largest finite bf16 value in the 16 channels behind a Cin % 32 == 16 slice (the header allows that read against
zero weights; NaN x 0 would poison the result by contract, a finite value must contribute nothing).  Scale and shift carry NaN guards
and NaN past Cout, and everything outside the output slice must come back bitwise unchanged.

ORE_BF16S_LOG=<file>: append the worst hard, rms and column-sum ratios, the lowest round-once share and the window misses per
(family, form, class) to that file."""
import ctypes as C
import os

import pytest
import torch

import bf16s_ref as BR

pytestmark = pytest.mark.gpu

NAN = float("nan")
CASES = BR.cases()
BY_ID = {c["id"]: c for c in CASES}
_STATS = {}         # (family, form, class) -> [worst hard, worst rms, worst colsum ratio, lowest share, window misses, checks]
_CELLS = set()      # (family, class) that ran
_FORMS = set()      # launch forms that ran


@pytest.fixture(scope="module")
def oh():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import orehip
    orehip.lib()
    return orehip


@pytest.fixture(scope="module", autouse=True)
def stats_report(oh):
    yield
    lines = [f"{fam:9s} {form:16s} {cl:12s} max hard {h:.3e}  max rms {r:.3e}  max colsum {s:.3e}  min share {sh:.5f}  window misses {wm}  ({n} checks)"
             for (fam, form, cl), (h, r, s, sh, wm, n) in sorted(_STATS.items())]
    print("\n" + "\n".join(lines))
    log = os.environ.get("ORE_BF16S_LOG")
    if log and lines:
        with open(log, "a") as f:
            f.write("\n".join(lines) + "\n")


def _rows(t, ld, coff, dtype, off=0):
    """t [rows, C] as channels coff .. coff + C of a [rows, ld] view of `dtype` with NaN around it, in a NaN-filled allocation that has
    HEAD_ROWS rows (+ off elements) in front of the view and TAIL_ROWS behind it.  Returns (view, allocation)."""
    rows, Cc = t.shape
    big = torch.full(((BR.HEAD_ROWS + rows + BR.TAIL_ROWS) * ld + 8,), NAN, device="cuda", dtype=dtype)
    lo = BR.HEAD_ROWS * ld + off
    v = big[lo:lo + rows * ld].view(rows, ld)
    v[:, coff:coff + Cc] = t.to(dtype).cuda()
    return v, big


def _guarded(t):
    """The fp32 values of t, flat, with GUARD NaN floats in front and behind.  Returns (view, allocation)."""
    n = t.numel()
    big = torch.full((n + 2 * BR.GUARD,), NAN, device="cuda")
    big[BR.GUARD:BR.GUARD + n] = t.reshape(-1).cuda()
    return big[BR.GUARD:BR.GUARD + n], big


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _untouched(after, before, view, coff, Cc):
    """Nothing outside channels [coff, coff + Cc) of `view` changed (compared as bits: NaN stays NaN).  `after` is consumed."""
    lo, n = view.storage_offset(), view.numel()
    _bits(after)[lo:lo + n].view(view.shape)[:, coff:coff + Cc] = _bits(before)[lo:lo + n].view(view.shape)[:, coff:coff + Cc]
    return torch.equal(_bits(after), _bits(before))


def _launch(oh, d, lev):
    L = oh.lib()
    nl, H, W, ep = lev
    if nl == 0:
        oh._chk(L.ore_conv2d_fwd(C.byref(d), oh._stream()), "ore_conv2d_fwd")
    else:
        oh._chk(L.ore_conv2d_levels_fwd(C.byref(d), nl, oh._i32s(H), oh._i32s(W), ep, oh._stream()), "ore_conv2d_levels_fwd")
    return oh.conv_last_launch()


def _run_case(oh, c):
    L = oh.lib()
    bf = torch.bfloat16
    o = BR.operands(c)
    in_ld, out_ld, add_ld, rows_in, rows_out = BR.geometry(c)
    Cout, Cout16, oc = c["Cout"], BR.c16(c["Cout"]), c["out_coff"]
    keep = []                                              # the allocations behind the views
    x, big = _rows(o["x"], in_ld, BR.IN_COFF, bf)
    if c["Cin"] % 32 == 16:                                # the one read the header allows outside the slice: against zero weights
        x[:, BR.IN_COFF + c["Cin"]:BR.IN_COFF + c["Cin"] + 16] = BR.BF16_MAX
    keep.append(big)
    ws_ = [o["w"][l] for l in range(len(c["HW"]))] if c["wlevel"] else [o["w"]]
    pw = torch.stack([oh.pack_conv_weight_bf16(w) for w in ws_]).contiguous().cuda()
    assert pw.shape[1] == BR.packed_elems(c)
    ws = oh._default_ws(x.device)
    ptr = {"in": x.data_ptr(), "w": pw.data_ptr(), "workspace": ws.data_ptr(), "workspace_floats": ws.numel()}
    for name in ("scale", "shift"):
        if name in o:
            v, big = _guarded(o[name])
            keep.append(big)
            ptr[name] = v.data_ptr()
    if c["add"]:
        v, big = _rows(o["add"].reshape(-1, Cout), add_ld, BR.ADD_COFF, bf)
        keep.append(big)
        ptr["add"] = v.data_ptr()
    odt = torch.float32 if c["f32out"] else bf
    out, out_big = _rows(torch.full((rows_out, Cout), NAN), out_ld, oc, odt, off=c["out_off"])
    ptr["out"] = out.data_ptr()
    assert out.data_ptr() % 8 == (4 if c["out_off"] else 0)
    before = out_big.clone()
    d = oh.ConvDesc()
    with oh.conv_overrides(*c["ov"]):
        lev = BR.fill_desc(d, c, ptr)
        cs = None
        if c["colsum"]:
            tiles = int(L.ore_conv_colsum_rows(C.byref(d)))
            assert tiles >= 2, (c["id"], tiles)
            cs, cs_big = _guarded(torch.zeros(tiles, Cout16))
            d.colsum = cs.data_ptr()
        pl = oh.conv_plan(d, None if lev[0] == 0 else c["HW"], lev[3])
        launch = _launch(oh, d, lev)
        torch.cuda.synchronize()
        got_dev = out[:, oc:oc + Cout].clone()
        got_cs = cs.clone().view(-1, Cout16) if cs is not None else None
        after = out_big.clone()
        if cs is not None:
            cs.zero_()
        launch2 = _launch(oh, d, lev)
        torch.cuda.synchronize()
    name, S = launch
    assert name == c["launcher"] and S == c["want_S"], (c["id"], launch)
    assert BR.plan_matches(c, pl, oh.CONV_LAUNCHERS) and (oh.CONV_LAUNCHERS[pl.launcher], pl.splitk) == launch, (c["id"], pl.astuple(), launch)
    assert launch2 == launch and torch.equal(_bits(got_dev), _bits(out[:, oc:oc + Cout].contiguous())), "two identical launches differ"
    assert _untouched(after, before, out, oc, Cout), ("wrote outside its output slice", c["id"])
    got = got_dev.double().cpu()
    ref, mag, dd = BR.reference(c, o, S)
    hard = rms = csr = 0.0
    misses, share = 0, 1.0
    if c["f32out"]:
        hard, rms = BR.check(got, ref, mag, dd)
    else:
        misses, share = BR.store_check(got, ref, mag, dd)
    if cs is not None:
        assert got_cs.shape[0] == -(-rows_out // pl.bm), (c["id"], got_cs.shape, pl.bm)
        assert torch.equal(got_cs, cs.view(-1, Cout16)), "two identical launches differ in their column sums"
        assert bool(cs_big[:BR.GUARD].isnan().all()) and bool(cs_big[-BR.GUARD:].isnan().all()), "wrote outside the column sums"
        csr = BR.colsum_check(got_cs.cpu(), got, pl.bm, Cout)
    if S > 1:
        assert int(ws[:BR.CNT_INTS].view(torch.int32).abs().sum()) == 0, "split-K arrival counters not back at zero"
    key = (c["family"], c["form"], c["cls"])
    h0, r0, s0, sh0, wm0, n0 = _STATS.get(key, (0.0, 0.0, 0.0, 1.0, 0, 0))
    _STATS[key] = (max(h0, hard), max(r0, rms), max(s0, csr), min(sh0, share), wm0 + misses, n0 + 1)
    _CELLS.add((c["family"], c["cls"]))
    _FORMS.add(c["form"])
    print(f"\n{c['id']}: {name} S={S} plan={pl.astuple()} d={dd}: hard {hard:.3e} rms {rms:.3e} colsum {csr:.3e} share {share:.5f} "
          f"window misses {misses}")
    assert hard <= 1 and rms <= 1 and csr <= 1 and misses == 0 and share >= BR.SHARE_MIN, (c["id"], launch, hard, rms, csr, misses, share)


@pytest.mark.parametrize("cid", [c["id"] for c in CASES])
def test_bf16_storage_case(oh, cid):
    _run_case(oh, BY_ID[cid])


def test_refusals_at_the_launch(oh):
    """What ore_conv_plan refuses (tests/test_bf16s_host.py::test_refusals), at the launch itself: an input affine and a per-level
    launch outside the 64 / 128-channel 3x3 form return ORE_EINVAL and launch nothing; column sums with fp32 output leave k_conv_kd."""
    L = oh.lib()
    bf = torch.bfloat16
    c = next(c for c in CASES if c["cls"] == "COLSUM" and c["family"] == "KD")
    in_ld, out_ld, _, rows_in, rows_out = BR.geometry(c)
    x = torch.zeros(rows_in + 8, in_ld, device="cuda", dtype=bf)
    o = BR.operands(c)
    pw = oh.pack_conv_weight_bf16(o["w"]).cuda()
    ws = oh._default_ws(x.device)
    mul = torch.ones(c["B"], c["Cin"], device="cuda")
    sc = torch.ones(BR.c16(c["Cout"]), device="cuda")
    cs = torch.zeros(rows_out, BR.c16(c["Cout"]), device="cuda")

    def desc(case, out):
        d = oh.ConvDesc()
        lev = BR.fill_desc(d, case, {"in": x.data_ptr(), "w": pw.data_ptr(), "out": out.data_ptr(), "scale": sc.data_ptr(), "shift": sc.data_ptr(),
                                     "workspace": ws.data_ptr(), "workspace_floats": ws.numel()})
        return d, lev

    out = torch.zeros(rows_out, out_ld, device="cuda", dtype=bf)
    d, lev = desc(c, out)
    d.in_mul = mul.data_ptr()
    assert L.ore_conv2d_fwd(C.byref(d), oh._stream()) == -22 and oh.conv_last_launch()[0] == "none"
    lv = dict(c, k=1, pad=0, wlevel=True, levels=True, colsum=False, HW=[c["HW"][0]])
    d, lev = desc(lv, out)
    assert L.ore_conv2d_levels_fwd(C.byref(d), 1, oh._i32s(lev[1]), oh._i32s(lev[2]), 0, oh._stream()) == -22
    assert oh.conv_last_launch()[0] == "none"
    torch.cuda.synchronize()
    assert float(out.float().abs().max()) == 0.0
    out32 = torch.zeros(rows_out, out_ld, device="cuda")
    with oh.conv_overrides((-12, 2)):
        d, lev = desc(c, out)
        d.colsum = cs.data_ptr()
        _launch(oh, d, lev)
        assert oh.conv_last_launch()[0] == "k_conv_kd"
        d, lev = desc(dict(c, f32out=True), out32)
        d.colsum = cs.data_ptr()
        _launch(oh, d, lev)
        assert oh.conv_last_launch()[0] not in ("k_conv_kd", "none")
    torch.cuda.synchronize()


def test_reached_cells():
    """The exact set of (family, class) cells and of launch forms that ran (runs after them): a form that stops taking a class, or a
    typo in an override code, fails here instead of testing something else.  Every cell is either run or listed in bf16s_ref.REFUSED."""
    if not _CELLS:
        pytest.fail("the cases did not run before this test")
    print("\ncells reached:", len(_CELLS), "forms:", len(_FORMS))
    assert _CELLS == EXPECTED, (sorted(_CELLS - EXPECTED), sorted(EXPECTED - _CELLS))
    assert _FORMS == BR.all_forms(), sorted(BR.all_forms() - _FORMS)


EXPECTED = {
    ("WS_SB64", "PLAIN"), ("WS_SB64", "SLICE_IN"), ("WS_SB128", "PLAIN"), ("WS_SB128", "SLICE_IN"), ("WS_SB128", "LEVELS"), ("WS_S2", "S2"), ("WS_WLEVEL", "WLEVEL"),
    ("KD", "PLAIN"), ("KD", "F32OUT"), ("KD", "SCALAR_STORE"), ("KD", "ADD"), ("KD", "COLSUM"), ("KD", "S2"), ("KD", "SLICE_IN"), ("KD", "LEVELS"),
    ("GS", "PLAIN"), ("GS", "F32OUT"), ("GS", "SCALAR_STORE"), ("GS", "ADD"), ("GS", "COLSUM"), ("GS", "S2"), ("GS", "SLICE_IN"),
    ("KW", "PLAIN"), ("KW", "F32OUT"), ("KW", "SCALAR_STORE"), ("KW", "ADD"), ("KW", "COLSUM"), ("KW", "S2"), ("KW", "SLICE_IN"),
    ("KW", "LEVELS"), ("KW", "SPLITK"),
}
