"""CPU: the bf16-storage conv contract of tests/bf16s_ref.py is neither loose nor wrong.

tests/test_hip_bf16s_conv.py holds every bf16-storage launch form to that reference.  Here, without a GPU: an fp32 emulation of a
launch -- an fp32 GEMM on the bf16 operands, in split-K slabs where S > 1, then the epilogue in the order of csrc/ore_conv_epilogue.h
(scale, shift, addend, ReLU, ONE rounding to bf16, column sums of the rounded values) -- passes the window, the round-once share at
SHARE_EMU, the element and block-rms bounds on the value in front of the store, and the column-sum bound at every case of the GPU
table; each fault the pin exists to catch fails the condition named next to it in FAULTS; the operands are normal bf16 numbers;
ore_conv_plan (host code, fake pointers) puts every case on the launch form the table names; and every REFUSED pair is refused."""
import ctypes as C
import os
import re

import pytest
import torch

import bf16s_ref as BR
import fwdconv_ref as FR

CASES = BR.cases()
BY_ID = {c["id"]: c for c in CASES}


def _first(cls, family=None, pred=None, **kw):
    for c in CASES:
        if c["cls"] == cls and (family is None or c["family"] == family) and all(c[k] == v for k, v in kw.items()) and (pred is None or pred(c)):
            return c
    raise KeyError((cls, family, kw))


def emulate(c, o, *, S=1, bm=16, fault=None):
    """(y [rows, Cout] fp32 in front of the store, stored [rows, Cout] fp32 holding what the launch stores, colsum [tiles, Cout16]) of
    case c as a launch computes it; fault: one of FAULTS."""
    B, Cin, Cout, k, stride, pad = c["B"], c["Cin"], c["Cout"], c["k"], c["stride"], c["pad"]
    outs, r0 = [], 0
    for l, (H, W) in enumerate(c["HW"]):
        n = B * H * W
        x = o["x"][r0:r0 + n].reshape(B, H, W, Cin)
        r0 += n
        w = o["w"][l] if c["wlevel"] else o["w"]
        b = w.permute(2, 3, 1, 0).reshape(k * k * Cin, Cout)
        Ho, Wo = FR.out_hw(H, W, k, stride, pad)
        if fault == "halo_across_seam":                                  # the images of a level as one tall image: no zero rows between them
            assert B > 1 and k == 3 and stride == 1
            a = FR._cols(x.reshape(1, B * H, W, Cin), k, stride, pad, B * Ho, Wo)
        else:
            a = FR._cols(x, k, stride, pad, Ho, Wo)
        M, K = a.shape
        if fault == "tap_missing_last_tile" and l == len(c["HW"]) - 1:
            a = a.clone()
            a[(M // bm) * bm:, (k * k // 2) * Cin:(k * k // 2 + 1) * Cin] = 0        # the centre tap: inside every image
        per = -(-K // S)
        acc = torch.zeros(M, Cout)
        for s in range(S):
            acc = acc + a[:, s * per:(s + 1) * per] @ b[s * per:(s + 1) * per]
        le = 0 if (fault == "wrong_level" and l > 0) else l
        e0 = le * c["ep_stride"]
        v = acc
        if "scale" in o:
            v = v * o["scale"].reshape(-1)[e0:e0 + Cout]
        if "shift" in o:
            sh = o["shift"].reshape(-1)[e0:e0 + Cout].clone()
            if fault == "relu_after_rounding_shift_ulp":                 # every shift one bf16 ulp off: THIS is what the case catches; the
                # ReLU behind the rounding alone changes no bit (test_relu_behind_the_rounding_alone_changes_nothing)
                sh = sh * (1.0 + 2.0 ** -7)
            v = v + sh
        if "add" in o:
            oy, ox = torch.arange(Ho)[:, None], torch.arange(Wo)[None, :]
            aH, aW = (Ho + 1) // 2, (Wo + 1) // 2
            up = o["add"][:, oy.clamp(max=aH - 1), ox.clamp(max=aW - 1)] if fault == "add_at_oy_ox" else o["add"][:, oy >> 1, ox >> 1]
            v = v + up.reshape(-1, Cout)
        outs.append(v)
    y = torch.cat(outs, 0)
    relu = c["relu"]
    if fault != "relu_after_rounding_shift_ulp":
        y = torch.cat([y[:, :relu].clamp(min=0), y[:, relu:]], 1)
    if c["f32out"]:
        stored = y
    elif fault == "truncate":
        stored = BR.trunc_bf16(y)
    elif fault == "round_twice":
        stored = BR.bf16_rne(BR.round_bits(y, 10))
    else:
        stored = BR.bf16_rne(y)
    if fault == "relu_after_rounding_shift_ulp":
        stored = torch.cat([stored[:, :relu].clamp(min=0), stored[:, relu:]], 1)
    src = y if fault == "colsum_unrounded" else stored
    tiles = -(-y.shape[0] // bm)
    cs = torch.zeros(tiles, BR.c16(Cout))
    for t in range(tiles):
        cs[t, :Cout] = src[t * bm:(t + 1) * bm].sum(0)
    if fault == "colsum_lane_not_zeroed" and BR.c16(Cout) > Cout:
        cs[tiles - 1, Cout] = 1e-30
    return y, stored, cs


def _measure(c, **kw):
    """dict(hard, rms, misses, share, colsum) of the emulation of case c."""
    o = BR.operands(c)
    S = c["want_S"]
    bm = c["build"][0] if c["family"] in ("KD", "GS", "KW") else 16
    y, stored, cs = emulate(c, o, S=S, bm=bm, **kw)
    ref, mag, d = BR.reference(c, o, S)
    hard, rms = BR.check(y, ref, mag, d)
    misses, share = (0, 1.0) if c["f32out"] else BR.store_check(stored, ref, mag, d)
    if c["f32out"]:
        hard, rms = BR.check(stored, ref, mag, d)
    return dict(hard=hard, rms=rms, misses=misses, share=share, colsum=BR.colsum_check(cs, stored, bm, c["Cout"]))


# ---- the reference and its tools ----------------------------------------------------------------------------------------------------
def test_rne_bf16_is_round_to_nearest_even_from_float64():
    g = torch.Generator().manual_seed(1)
    t = torch.randn(20000, generator=g, dtype=torch.float64) * 10.0 ** (torch.rand(20000, generator=g, dtype=torch.float64) * 12 - 6)
    r = BR.rne_bf16(t)
    assert torch.equal(r, r.float().bfloat16().double())                 # a bf16 value
    assert bool(((t - r).abs() <= (t.abs() * 2.0 ** -8)).all())                      # within half an ulp
    # a tie goes to the even neighbour; a value one float64 ulp past the tie goes up, although fp32 would round it onto the tie first
    one = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -40], dtype=torch.float64)
    assert BR.rne_bf16(one).tolist() == [1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7]
    assert BR.bf16_rne(one.float()).double().tolist() == [1.0, 1.0 + 2.0 ** -6, 1.0]
    assert BR.rne_bf16(-one).tolist() == [-1.0, -(1.0 + 2.0 ** -6), -(1.0 + 2.0 ** -7)]
    assert bool((BR.rne_bf16(torch.zeros(3, dtype=torch.float64)) == 0).all())


def test_reference_reuses_the_forward_reference():
    """bf16s_ref.reference is fwdconv_ref.fwd_ref on the bf16 values; the per-level-weight form is the same level by level."""
    c = _first("WLEVEL")
    o = BR.operands(c)
    ref, mag, d = BR.reference(c, o, 1)
    assert ref.shape == (BR.geometry(c)[4], c["Cout"]) and d == BR.depth(9 * c["Cin"], 1)
    r0 = 0
    for l, (H, W) in enumerate(c["HW"]):
        n = c["B"] * H * W
        x = o["x"][r0:r0 + n].reshape(c["B"], H, W, -1).permute(0, 3, 1, 2).double()
        y = torch.nn.functional.conv2d(x, o["w"][l].double(), None, 1, 1).permute(0, 2, 3, 1).reshape(n, -1)
        y = y * o["scale"][l, :c["Cout"]].double() + o["shift"][l, :c["Cout"]].double()
        y[:, :c["relu"]] = y[:, :c["relu"]].clamp(min=0)
        assert torch.allclose(ref[r0:r0 + n], y, rtol=1e-11, atol=1e-11 * float(y.abs().max())), l
        r0 += n
    assert not torch.equal(o["w"][0], o["w"][1])


@pytest.mark.parametrize("cid", [c["id"] for c in CASES])
def test_operands_are_normal_bf16_numbers(cid):
    c = BY_ID[cid]
    o = BR.operands(c)
    for name in ("x", "w", "add"):
        if name in o:
            t = o[name]
            assert torch.equal(t, t.bfloat16().float()), name
            assert bool(((t.abs() >= BR.BF16_MIN_NORMAL) & (t.abs() < BR.BF16_MAX)).all()), name
    ref, mag, d = BR.reference(c, o, c["want_S"])
    if not c["f32out"]:                                                   # every stored value is a normal bf16 number or a ReLU zero
        r = BR.rne_bf16(ref).abs()
        assert bool((((r >= BR.BF16_MIN_NORMAL) & (r < BR.BF16_MAX)) | (ref == 0)).all())
    for name in ("scale", "shift"):
        if name in o:
            assert bool(o[name][:, c["Cout"]:].isnan().all()) and bool(o[name][:, :c["Cout"]].isfinite().all())


# ---- the emulation passes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c["id"] for c in CASES])
def test_fp32_emulation_passes_every_condition(cid):
    m = _measure(BY_ID[cid])
    assert m["misses"] == 0 and m["share"] >= BR.SHARE_EMU and m["hard"] < 0.25 and m["rms"] < 0.5 and m["colsum"] < 0.5, m


# ---- seeded faults: (fault, case, the condition that fails) ------------------------------------------------------------------------------
FAULTS = [
    ("truncate", _first("PLAIN", "KD")["id"], "share"),
    ("truncate", _first("PLAIN", "WS_SB64")["id"], "share"),
    ("truncate", _first("S2", "GS")["id"], "share"),
    ("round_twice", _first("PLAIN", "KD")["id"], "share"),
    ("round_twice", _first("PLAIN", "WS_SB128")["id"], "share"),
    ("round_twice", _first("ADD", "KW")["id"], "share"),
    ("relu_after_rounding_shift_ulp", _first("PLAIN", "KD", Cout=112)["id"], "window"),
    ("wrong_level", _first("LEVELS", "KW", f32out=False)["id"], "window"),
    ("wrong_level", _first("LEVELS", "KW", f32out=True)["id"], "hard"),
    ("wrong_level", _first("WLEVEL")["id"], "window"),
    ("wrong_level", _first("LEVELS", "WS_SB128")["id"], "window"),
    ("add_at_oy_ox", _first("ADD", "KD")["id"], "window"),
    ("add_at_oy_ox", _first("ADD", "GS")["id"], "window"),
    ("tap_missing_last_tile", _first("COLSUM", "KD", k=3)["id"], "window"),
    ("tap_missing_last_tile", _first("PLAIN", "WS_SB64")["id"], "window"),
    ("halo_across_seam", _first("PLAIN", "WS_SB128", B=2)["id"], "window"),
    ("halo_across_seam", _first("PLAIN", "KD", pred=lambda c: c["B"] > 1 and c["HW"][0][0] >= 3)["id"], "window"),
    ("colsum_unrounded", _first("COLSUM", "KD")["id"], "colsum"),
    ("colsum_unrounded", _first("COLSUM", "GS")["id"], "colsum"),
    ("colsum_unrounded", _first("SPLITK", "KW", colsum=True)["id"], "colsum"),
    ("colsum_lane_not_zeroed", _first("COLSUM", "KD")["id"], "colsum"),
]


def _failed(m):
    f = set()
    if m["misses"] > 0:
        f.add("window")
    if m["share"] < BR.SHARE_MIN:
        f.add("share")
    if m["hard"] > 1 or m["rms"] > 1:
        f.add("hard")
    if m["colsum"] > 1:
        f.add("colsum")
    return f


@pytest.mark.parametrize("fault,cid,cond", FAULTS)
def test_seeded_fault_fails_its_condition(fault, cid, cond):
    c = BY_ID[cid]
    assert not _failed(_measure(c))
    m = _measure(c, fault=fault)
    assert cond in _failed(m), (fault, cid, m)


def test_relu_behind_the_rounding_alone_changes_nothing():
    """Rounding to nearest even keeps the sign and maps 0 to 0, so max(RNE(y), 0) == RNE(max(y, 0)) bit for bit: the order of ReLU and
    store is not observable, and the seeded fault of that name is caught through its shift, one bf16 ulp off."""
    c = _first("PLAIN", "KD", Cout=112)
    o = BR.operands(c)
    y, stored, _ = emulate(dict(c, relu=0), o)                            # no ReLU in front of the store
    relu = c["relu"]
    behind = torch.cat([stored[:, :relu].clamp(min=0), stored[:, relu:]], 1)
    assert torch.equal(behind, emulate(c, o)[1]) and bool((y[:, :relu] < 0).any())


def test_every_fault_of_the_pin_is_seeded():
    assert {f for f, _, _ in FAULTS} == {"truncate", "round_twice", "relu_after_rounding_shift_ulp", "wrong_level", "add_at_oy_ox",
                                         "tap_missing_last_tile", "halo_across_seam", "colsum_unrounded", "colsum_lane_not_zeroed"}


def test_wrong_roundings_pass_the_older_measures():
    """What tests/test_hip_bf16.py asks of a stored tensor -- within one bf16 ulp plus 1e-6 of the largest value, or 1e-2 of the largest
    value -- passes most elements of a store that truncates (over three quarters of the one-ulp windows, all of the 1e-2 measure) and
    nearly all of one that rounds twice (over 99 % of the windows); the round-once share fails both outright."""
    c = _first("PLAIN", "KD")
    o = BR.operands(c)
    ref, mag, d = BR.reference(c, o, 1)
    for fault, lo, hi, inside in (("truncate", 0.3, 0.9, 0.75), ("round_twice", 0.85, 0.97, 0.99)):
        y, stored, _ = emulate(c, o, fault=fault)
        ulp = y.abs().clamp(min=1e-30) * 2.0 ** -8 + 1e-6 * float(y.abs().max())
        assert float(((stored - y).abs() <= ulp).float().mean()) >= inside
        assert float((stored.double() - ref).abs().max() / ref.abs().max()) < 1e-2
        share = BR.store_check(stored, ref, mag, d)[1]
        assert lo < share < hi, (fault, share)


# ---- the case table against the planner ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oh():
    import orehip
    if not os.path.exists(orehip.LIB_PATH):
        orehip.build()
    orehip.lib()
    return orehip


def _fake_ptrs(c, L):
    ptr = {"in": 0x10000000, "w": 0x20000000, "out": 0x30000000 + 2 * c["out_off"], "workspace": 0x40000000,
           "workspace_floats": L.ore_conv_workspace_floats()}
    for name, on, addr in (("scale", c["scale"], 0x50000040), ("shift", c["shift"], 0x51000040), ("add", c["add"], 0x54000000),
                           ("colsum", c["colsum"], 0x55000000)):
        if on:
            ptr[name] = addr
    return ptr


def _plan(oh, c, ov=None, **ptr_over):
    L = oh.lib()
    d, pl = oh.ConvDesc(), oh.ConvPlan()
    ptr = _fake_ptrs(c, L)
    ptr.update(ptr_over)
    nl, H, W, ep = BR.fill_desc(d, c, ptr)
    with oh.conv_overrides(*(c["ov"] if ov is None else ov)):
        rc = L.ore_conv_plan(C.byref(d), nl, oh._i32s(H) if nl else None, oh._i32s(W) if nl else None, ep, C.byref(pl))
    return rc, pl


def test_case_table_plans_on_its_forms(oh):
    """ore_conv_plan puts every case on the launch form -- kernel, build, split -- the table names; a column-sum case has at least two
    row tiles with a ragged last one."""
    bad = []
    for c in CASES:
        rc, pl = _plan(oh, c)
        if rc != 0 or not BR.plan_matches(c, pl, oh.CONV_LAUNCHERS):
            bad.append((c["id"], rc, oh.CONV_LAUNCHERS[pl.launcher], pl.astuple()))
        elif c["colsum"]:
            rows = BR.geometry(c)[4]
            if rows <= pl.bm or rows % pl.bm == 0:
                bad.append((c["id"], "column sums need two tiles and a ragged last one", rows, pl.bm))
    assert not bad, bad


def test_kw_tiles_the_planner_picks(oh):
    """bf16s_ref.KW_PLANNED is what ore_conv_plan picks for k_conv_kw with bf16 storage and k_conv_kd off somewhere in 1024 <= M <= 2000,
    Cout16 <= 256 (kw_tile's table entries and its generic search), below 1024 rows it picks 16x16 and 16x32 only, and together with
    KW_FORCED the table holds every tile of ORE_KW_TILES."""
    base = _first("PLAIN", "KW", build=(16, 48))
    kw = oh.CONV_LAUNCHERS.index("k_conv_kw")
    found, small = set(), set()
    for M in list(range(16, 1024, 48)) + list(range(1024, 2001, 8)):
        for Cout in range(16, 257, 16):
            c = dict(base, B=1, HW=[(1, M)], Cout=Cout, k=1, pad=0, out_tail=8)
            rc, pl = _plan(oh, c)
            assert rc == 0 and pl.launcher == kw and tuple(pl.build)[3] == 2, (M, Cout, pl.astuple())
            (found if M >= 1024 else small).add((pl.bm, pl.bn))
    assert found == set(BR.KW_PLANNED), sorted(found ^ set(BR.KW_PLANNED))
    assert small == {(16, 16), (16, 32)}
    with open(os.path.join(oh.CSRC, "ore_conv_internal.h")) as f:
        tiles = re.search(r"#define ORE_KW_TILES\(X\) \\\n(.*)", f.read())[1]
    assert {(int(a), int(b)) for a, b in re.findall(r"X\((\d+), (\d+)\)", tiles)} == set(BR.KW_PLANNED + BR.KW_FORCED)
    with open(oh.HEADER) as f:
        assert int(re.search(r"#define ORE_CONV_CNT_INTS (\d+)", f.read())[1]) == BR.CNT_INTS


def test_case_table_is_the_feature_table():
    """Every launch form appears and carries PLAIN (the weight-stationary forms: their one class), every DMA-fed family takes every
    rotated class on at least two builds, sizes stay within the limits of the pin, and the GPU module's literal EXPECTED set is the table's."""
    import test_hip_bf16s_conv as G
    assert len(BY_ID) == len(CASES)
    assert {c["form"] for c in CASES} == BR.all_forms()
    for form in BR.all_forms():
        cls = {c["cls"] for c in CASES if c["form"] == form}
        assert cls & {"PLAIN", "S2", "WLEVEL"}, form
    for fam in ("KD", "GS", "KW"):
        for cl in BR.ROTATED:
            assert len({c["form"] for c in CASES if c["family"] == fam and c["cls"] == cl}) >= 2, (fam, cl)
    big = {(1, (77, 78)), (2, (55, 55)), (1, (155, 157)), (1, (69, 71))}      # the weight-stationary forms start at 6000 rows
    for c in CASES:
        rows = BR.geometry(c)[4]
        assert rows <= 2000 or ((c["B"], c["HW"][0]) in big and c["launcher"] == BR.WS), c["id"]
        if c["cls"] == "SCALAR_STORE":
            assert c["out_coff"] % 4 == 2 or c["out_off"] == 2
        if c["cls"] == "SLICE_IN":
            assert c["Cin"] % 32 == 16
        if c["cls"] in ("ADD", "S2"):
            assert all(h % 2 == 1 and w % 2 == 1 for h, w in c["HW"])
        if c["cls"] != "S2" and c["relu"]:
            assert c["relu"] % 4 != 0 and c["relu"] < c["Cout"], c["id"]       # the ReLU edge lies inside a quad
    assert {c["Cout"] for c in CASES if c["cls"] == "PLAIN"} >= {5, 40, 112, 64, 128}
    assert BR.expected_cells() == G.EXPECTED, (sorted(BR.expected_cells() - G.EXPECTED), sorted(G.EXPECTED - BR.expected_cells()))


def test_refusals(oh):
    """bf16s_ref.REFUSED through ore_conv_plan: an input affine is ORE_EINVAL; a per-level launch outside the 64 / 128-channel 3x3 form is
    ORE_EINVAL; column sums with fp32 output do not run on k_conv_kd, nor do per-level epilogues; the weight-stationary kernel declines
    fp32 output, a scalar-store output, an addend and column sums (another launcher takes the call)."""
    EINVAL = -22
    c = _first("PLAIN", "KD")
    rc, pl = _plan(oh, c, in_mul=0x52000040)
    assert rc == EINVAL and pl.launcher == 0
    wl = _first("WLEVEL")
    for over in (dict(k=1, pad=0), dict(Cin=96), dict(Cout=40, ep_stride=48)):
        rc, pl = _plan(oh, dict(wl, **over))
        assert rc == EINVAL and pl.launcher == 0, over
    rc, pl = _plan(oh, dict(wl, f32out=True))
    assert rc == EINVAL
    kd = oh.CONV_LAUNCHERS.index("k_conv_kd")
    cs = _first("COLSUM", "KD")
    rc, pl = _plan(oh, cs, ov=[(-12, 2)])
    assert rc == 0 and pl.launcher == kd
    rc, pl = _plan(oh, dict(cs, f32out=True), ov=[(-12, 2)])
    assert rc == 0 and pl.launcher != kd and pl.launcher != 0
    rc, pl = _plan(oh, _first("LEVELS", "KD"))
    assert rc == 0 and pl.launcher == kd                                  # (the flat 1x1 form with a shared epilogue is k_conv_kd's)
    rc, pl = _plan(oh, dict(_first("LEVELS", "KW", f32out=False), ov=[(-12, 2)]))
    assert rc == 0 and pl.launcher != kd
    ws = oh.CONV_LAUNCHERS.index(BR.WS)
    for fam in ("WS_SB64", "WS_SB128", "WS_S2"):
        base = _first("S2" if fam == "WS_S2" else "PLAIN", fam)
        assert _plan(oh, base)[1].launcher == ws
        for over in (dict(f32out=True), dict(out_coff=6, out_tail=10), dict(out_off=2), dict(add=True), dict(colsum=True)):
            rc, pl = _plan(oh, dict(base, **over))
            assert rc == 0 and pl.launcher not in (ws, 0), (fam, over, pl.astuple())
    for la in ("KD", "GS"):                                               # no cross-block split outside k_conv_kw
        for c in CASES:
            if c["family"] == la:
                assert _plan(oh, dict(c, splitk=4))[1].splitk == 1, c["id"]
                break
