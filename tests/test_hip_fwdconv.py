"""Every forward conv launcher's fused prologue and epilogue against float64 (ore_conv2d_fwd and ore_conv2d_levels_fwd).

The data-gradient pin (tests/test_hip_dgrad.py) holds the plain stride-1 GEMM core of every launcher.  This module holds what only the
forward direction uses, launcher by launcher, because each kernel fetches the scale, shift and addend operands its own way
(csrc/ore_conv_epilogue.h): stride 2, the input affine (in_mul / in_add / in_relu over level * B + b), the nearest-2x addend read
from a channel slice of a wider map, the ReLU and Cout edges inside a channel quad with the scalar and the vector store, the fused column
sums, and the level-major entry point with per-level scale and shift.  tests/fwdconv_ref.py restates the contract in float64, derives
the bounds and holds the case table (class x launcher as ore_conv_plan.cpp admits them, with the refused pairs and why);
tests/test_fwdconv_host.py shows on the CPU that the bounds pass an fp32 emulation and fail the faults they are there to catch.

Every case forces its launcher through orehip.conv_overrides, asserts that conv_last_launch() names it and that ore_conv_plan
predicted it, takes d from the split that ran, and launches twice (bitwise equal).  Every input is a slice of a wider NaN-filled
allocation with NaN rows in front of and behind it, the per-channel vectors have NaN guards and NaN past Cout, and everything outside
the output slice must come back bitwise unchanged.  fp32 storage only (bf16 storage: tests/test_hip_bf16s_conv.py); operand precision
fp32 and bf16.

ORE_FWDCONV_LOG=<file>: append the worst hard, rms and column-sum ratios per (mode, launcher, class) to that file."""
import ctypes as C
import os

import pytest
import torch

import fwdconv_ref as FR

pytestmark = pytest.mark.gpu

NAN = float("nan")
CASES = FR.cases()
BY_ID = {c["id"]: c for c in CASES}
_RATIOS = {}        # (mode, launcher, class) -> [worst hard, worst rms, worst column-sum ratio, checks]
_CELLS = set()      # (mode, launcher, class) that ran


@pytest.fixture(scope="module")
def oh():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import orehip
    orehip.lib()
    return orehip


@pytest.fixture(scope="module", autouse=True)
def ratio_report(oh):
    yield
    lines = [f"{m:5s} {l:22s} {c:14s} max hard {h:.3e}  max rms {r:.3e}  max colsum {s:.3e}  ({n} checks)"
             for (m, l, c), (h, r, s, n) in sorted(_RATIOS.items())]
    print("\n" + "\n".join(lines))
    log = os.environ.get("ORE_FWDCONV_LOG")
    if log and lines:
        with open(log, "a") as f:
            f.write("\n".join(lines) + "\n")


@pytest.fixture
def mode(oh, request):
    prev = oh.set_conv_precision(request.param)
    yield request.param
    oh.set_conv_precision(prev)


def _rows(t, ld, coff):
    """t [rows, C] as channels coff .. coff + C of a [rows, ld] view with NaN around it in a NaN-filled allocation that has HEAD_ROWS
    rows in front of the view and TAIL_ROWS behind it.  Returns (view, allocation)."""
    rows, Cc = t.shape
    big = torch.full(((FR.HEAD_ROWS + rows + FR.TAIL_ROWS) * ld,), NAN, device="cuda")
    v = big[FR.HEAD_ROWS * ld:(FR.HEAD_ROWS + rows) * ld].view(rows, ld)
    v[:, coff:coff + Cc] = t.cuda()
    return v, big


def _guarded(t):
    """The values of t, flat, with GUARD NaN floats in front and behind.  Returns (view, allocation)."""
    n = t.numel()
    big = torch.full((n + 2 * FR.GUARD,), NAN, device="cuda")
    big[FR.GUARD:FR.GUARD + n] = t.reshape(-1).cuda()
    return big[FR.GUARD:FR.GUARD + n], big


def _untouched(after, before, view, coff, Cc):
    """Nothing outside channels [coff, coff + Cc) of `view` changed (compared as bits: NaN stays NaN)."""
    a, b = after.clone(), before.clone()
    lo, n = view.storage_offset(), view.numel()
    for t in (a, b):
        t[lo:lo + n].view(view.shape)[:, coff:coff + Cc] = 0
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _launch(oh, d, lev):
    L = oh.lib()
    nl, H, W, ep = lev
    if nl == 0:
        oh._chk(L.ore_conv2d_fwd(C.byref(d), oh._stream()), "ore_conv2d_fwd")
    else:
        oh._chk(L.ore_conv2d_levels_fwd(C.byref(d), nl, oh._i32s(H), oh._i32s(W), ep, oh._stream()), "ore_conv2d_levels_fwd")
    return oh.conv_last_launch()


def _run_case(oh, mode, c):
    L = oh.lib()
    o = FR.operands(c, mode)
    in_ld, out_ld, add_ld, rows_in, rows_out = FR.geometry(c)
    Cout, Cout16 = c["Cout"], FR.c16(c["Cout"])
    keep = []                                              # the allocations behind the views
    x, big = _rows(o["x"], in_ld, FR.IN_COFF)
    keep.append(big)
    pw = oh.pack_conv_weight_dev(o["w"].cuda().contiguous())
    ws = oh._default_ws(x.device)
    ptr = {"in": x.data_ptr(), "w": pw.data_ptr(), "workspace": ws.data_ptr(), "workspace_floats": ws.numel()}
    for name in ("scale", "shift", "in_mul", "in_add"):
        if name in o:
            v, big = _guarded(o[name])
            keep.append(big)
            ptr[name] = v.data_ptr()
    if c["add"]:
        a = o["add"]
        v, big = _rows(a.reshape(-1, Cout), add_ld, FR.ADD_COFF)
        keep.append(big)
        ptr["add"] = v.data_ptr()
    if c["wino"]:
        ww = oh.winograd_weight(pw, Cout, c["Cin"])
        ptr["w_wino"] = ww.data_ptr()
    out, out_big = _rows(torch.full((rows_out, Cout), NAN), out_ld, c["out_coff"])
    ptr["out"] = out.data_ptr()
    before = out_big.clone()
    d = oh.ConvDesc()
    with oh.conv_overrides(*c["ov"]):
        lev = FR.fill_desc(d, c, ptr)
        cs = None
        if c["colsum"]:
            tiles = int(L.ore_conv_colsum_rows(C.byref(d)))
            assert tiles >= 2, (c["id"], tiles)
            cs, cs_big = _guarded(torch.zeros(tiles, Cout16))
            d.colsum = cs.data_ptr()
        pl = oh.conv_plan(d, None if lev[0] == 0 else c["HW"], lev[3])
        launch = _launch(oh, d, lev)
        torch.cuda.synchronize()
        got = out[:, c["out_coff"]:c["out_coff"] + Cout].clone()
        got_cs = cs.clone().view(-1, Cout16) if cs is not None else None
        after = out_big.clone()
        if cs is not None:
            cs.zero_()
        launch2 = _launch(oh, d, lev)
        torch.cuda.synchronize()
    name, S = launch
    assert name == c["launcher"] and S == c["want_S"], (c["id"], launch)
    assert (oh.CONV_LAUNCHERS[pl.launcher], pl.splitk) == launch, (c["id"], pl.astuple(), launch)
    assert launch2 == launch and torch.equal(got, out[:, c["out_coff"]:c["out_coff"] + Cout]), "two identical launches differ"
    assert _untouched(after, before, out, c["out_coff"], Cout), ("wrote outside its output slice", c["id"])
    ref, mag, dd = FR.reference(c, mode, o, name, S)
    hard, rms = FR.check(got.cpu(), ref, mag, dd)
    csr = 0.0
    if cs is not None:
        assert got_cs.shape[0] == -(-rows_out // pl.bm), (c["id"], got_cs.shape, pl.bm)
        assert torch.equal(got_cs, cs.view(-1, Cout16)), "two identical launches differ in their column sums"
        assert bool(cs_big[:FR.GUARD].isnan().all()) and bool(cs_big[-FR.GUARD:].isnan().all()), "wrote outside the column sums"
        csr = FR.colsum_check(got_cs.cpu(), ref, mag, dd, pl.bm, Cout)
    if S > 1:
        assert int(ws[:4096].view(torch.int32).abs().sum()) == 0, "split-K arrival counters not back at zero"
    key = (mode, name, c["cls"])
    h0, r0, s0, n0 = _RATIOS.get(key, (0.0, 0.0, 0.0, 0))
    _RATIOS[key] = (max(h0, hard), max(r0, rms), max(s0, csr), n0 + 1)
    _CELLS.add(key)
    print(f"\n{c['id']} {mode}: {name} S={S} bm={pl.bm} d={dd}: hard {hard:.3e} rms {rms:.3e} colsum {csr:.3e}")
    assert hard <= 1 and rms <= 1 and csr <= 1, (c["id"], mode, launch, hard, rms, csr)


@pytest.mark.parametrize("cid,mode", [(c["id"], m) for c in CASES for m in c["modes"]], indirect=["mode"])
def test_forward_case(oh, cid, mode):
    _run_case(oh, mode, BY_ID[cid])


def test_reached_cells():
    """The exact set of (mode, launcher, class) cells that ran (runs after them): a launcher that stops taking a class, or a typo in an
    override code, fails here instead of testing something else."""
    if not _CELLS:
        pytest.fail("the cases did not run before this test")
    print("\ncells reached:", len(_CELLS))
    assert _CELLS == EXPECTED, (sorted(_CELLS - EXPECTED), sorted(EXPECTED - _CELLS))


EXPECTED = {
    ("bf16", "k_conv_gd", "ADD"), ("fp32", "k_conv_gd", "ADD"), ("fp32", "k_conv_gs", "ADD"), ("bf16", "k_conv_igemm", "ADD"),
    ("fp32", "k_conv_igemm", "ADD"), ("fp32", "k_conv_kd", "ADD"), ("bf16", "k_conv_kw", "ADD"), ("fp32", "k_conv_kw", "ADD"),
    ("fp32", "k_conv_rf", "ADD"),
    ("bf16", "k_conv_igemm", "ADD/splitk"), ("fp32", "k_conv_igemm", "ADD/splitk"), ("bf16", "k_conv_kw", "ADD/splitk"),
    ("fp32", "k_conv_kw", "ADD/splitk"),
    ("bf16", "k_conv_igemm", "AFF"), ("fp32", "k_conv_igemm", "AFF"),
    ("bf16", "k_conv_gd", "COLSUM"), ("fp32", "k_conv_gd", "COLSUM"), ("fp32", "k_conv_gs", "COLSUM"),
    ("bf16", "k_conv_igemm", "COLSUM"), ("fp32", "k_conv_igemm", "COLSUM"), ("fp32", "k_conv_kd", "COLSUM"),
    ("bf16", "k_conv_kw", "COLSUM"), ("fp32", "k_conv_kw", "COLSUM"), ("fp32", "k_conv_rf", "COLSUM"),
    ("bf16", "k_conv_igemm", "COLSUM/splitk"), ("fp32", "k_conv_igemm", "COLSUM/splitk"), ("bf16", "k_conv_kw", "COLSUM/splitk"),
    ("fp32", "k_conv_kw", "COLSUM/splitk"),
    ("bf16", "k_conv3x3_patch<4>", "LEV"), ("fp32", "k_conv3x3_patch<4>", "LEV"), ("fp32", "k_conv3x3_patch<8>", "LEV"),
    ("fp32", "k_conv3x3_patch_db", "LEV"), ("fp32", "k_conv3x3_wino", "LEV"), ("fp32", "k_conv3x3_wino_nu", "LEV"),
    ("fp32", "k_conv3x3_ws<2,128>", "LEV"), ("bf16", "k_conv3x3_ws<2,64>", "LEV"), ("fp32", "k_conv3x3_ws<2,64>", "LEV"),
    ("bf16", "k_conv_gd", "LEV"), ("fp32", "k_conv_gd", "LEV"), ("bf16", "k_conv_igemm", "LEV"), ("fp32", "k_conv_igemm", "LEV"),
    ("fp32", "k_conv_kd", "LEV"), ("bf16", "k_conv_kw", "LEV"), ("fp32", "k_conv_kw", "LEV"),
    ("bf16", "k_conv_igemm", "LEV+AFF"), ("fp32", "k_conv_igemm", "LEV+AFF"),
    ("bf16", "k_conv_gd", "S2"), ("fp32", "k_conv_gd", "S2"), ("fp32", "k_conv_gs", "S2"), ("bf16", "k_conv_igemm", "S2"),
    ("fp32", "k_conv_igemm", "S2"), ("fp32", "k_conv_kd", "S2"), ("bf16", "k_conv_kw", "S2"), ("fp32", "k_conv_kw", "S2"),
    ("fp32", "k_conv_rf", "S2"),
    ("bf16", "k_conv3x3_patch<4>", "TAIL"), ("fp32", "k_conv3x3_patch<4>", "TAIL"), ("fp32", "k_conv3x3_patch<8>", "TAIL"),
    ("fp32", "k_conv3x3_patch_db", "TAIL"), ("fp32", "k_conv3x3_wino", "TAIL"), ("fp32", "k_conv3x3_wino_nu", "TAIL"),
    ("fp32", "k_conv3x3_ws<2,128>", "TAIL"), ("bf16", "k_conv3x3_ws<2,64>", "TAIL"), ("fp32", "k_conv3x3_ws<2,64>", "TAIL"),
    ("fp32", "k_conv_gs", "TAIL"), ("bf16", "k_conv_igemm", "TAIL"), ("fp32", "k_conv_igemm", "TAIL"), ("fp32", "k_conv_kd", "TAIL"),
    ("bf16", "k_conv_kw", "TAIL"), ("fp32", "k_conv_kw", "TAIL"), ("fp32", "k_conv_rf", "TAIL"),
}
