"""CPU: the float64 forward-conv reference of tests/fwdconv_ref.py is the contract, and its bounds are neither loose nor wrong.

tests/test_hip_fwdconv.py holds every forward launcher's fused prologue and epilogue to that reference.  Here, without a GPU: the
reference equals float64 F.conv2d with the affine, the addend and the ReLU spelled out; an fp32 emulation of the contract (the input
affine in fp32, a k-ordered fma chain in S slabs, an fp32 epilogue, fp32 tile sums; operands rounded to bf16 in that mode) passes the
element, block-rms and column-sum bounds at every case of the GPU table; each seeded fault exceeds one of them; every bf16 affine case
has an affine that is exact in fp32; and ore_conv_plan (host code, fake pointers) puts every case on the launcher the table names, in
the modes it names, and on another launcher or on none in the mode it leaves out."""
import ctypes as C
import math

import pytest
import torch

import fwdconv_ref as FR

CASES = FR.cases()
BY_ID = {c["id"]: c for c in CASES}
# one case per class for the emulation (the launcher only decides S and bm here) plus everything that differs in arithmetic
EMU = [c for c in CASES if c["launcher"] in ("k_conv_igemm", "k_conv_gd", "k_conv3x3_patch<4>", "k_conv3x3_wino")]


def _affine32(x, mul, add, relu):
    v = x * mul if mul is not None else x
    if add is not None:
        v = v + add
    return v.clamp(min=0) if relu else v


def emulate(c, o, mode, *, S=1, bm=16, fault=None):
    """fp32 (out [rows, Cout], colsum [tiles, Cout16]) of case c as a launch computes it; fault: one of the seeded faults."""
    B, Cin, Cout, k, stride, pad = c["B"], c["Cin"], c["Cout"], c["k"], c["stride"], c["pad"]
    bf16 = mode == "bf16"
    w = FR.bf16_rne(o["w"]) if bf16 else o["w"]
    b = w.permute(2, 3, 1, 0).reshape(k * k * Cin, Cout).double()
    relu_in = c["aff"] == "mul_add_relu"
    outs, r0 = [], 0
    for l, (H, W) in enumerate(c["HW"]):
        n = B * H * W
        x = o["x"][r0:r0 + n].reshape(B, H, W, Cin)
        r0 += n
        sid = slice(l * B, (l + 1) * B)
        if fault == "in_mul_by_b" or (fault == "level1_in_mul_of_level0" and l == 1):
            sid = slice(0, B)
        mul = o["in_mul"][sid, None, None, :] if "in_mul" in o else None
        ia = o["in_add"][l * B:(l + 1) * B, None, None, :] if "in_add" in o else None
        pads = (0, 0, pad, pad, pad, pad)
        if fault == "s2_window_shifted" and H % 2 == 0:
            pads = (0, 0, pad, pad, 0, 2 * pad)             # rows start at 0 instead of -1
        if fault == "pad_gets_in_add":
            tp = _affine32(torch.nn.functional.pad(x, pads), mul, ia, relu_in)
        else:
            tp = torch.nn.functional.pad(_affine32(x, mul, ia, relu_in), pads)
        if bf16:
            tp = FR.bf16_rne(tp)
        Ho, Wo = FR.out_hw(H, W, k, stride, pad)
        a = FR._cols(tp, k, stride, 0, Ho, Wo).double()
        M, K = a.shape
        per = -(-K // S)
        acc = torch.zeros(M, Cout)
        for s in range(S if not c["wino"] else 0):
            part = torch.zeros(M, Cout)
            for kk in range(s * per, min(K, (s + 1) * per)):
                part = (part.double() + a[:, kk:kk + 1] * b[kk:kk + 1]).float()
            acc = part if S == 1 else (acc.double() + part.double()).float()
        if c["wino"]:                                       # F(2x2,3x3) with every transform and the channel sum in fp32
            acc = FR.DR.winograd(x, w.permute(1, 0, 2, 3), dtype=torch.float32).reshape(-1, Cout)
        le = 0 if (fault == "level1_scale_of_level0" and l == 1) else l
        v = acc
        if "scale" in o:
            v = v * o["scale"].reshape(-1)[le * c["ep_stride"]:le * c["ep_stride"] + Cout]
        if "shift" in o:
            v = v + o["shift"].reshape(-1)[l * c["ep_stride"]:l * c["ep_stride"] + Cout]
        if "add" in o:
            oy, ox = torch.arange(Ho)[:, None], torch.arange(Wo)[None, :]
            aH, aW = (Ho + 1) // 2, (Wo + 1) // 2
            if fault == "add_at_oy_ox":
                up = o["add"][:, oy.clamp(max=aH - 1), ox.clamp(max=aW - 1)]
            elif fault == "add_floor_dims":
                flat = o["add"].reshape(-1, Cout)
                idx = (torch.arange(B)[:, None, None] * (Ho // 2) + (oy >> 1)) * (Wo // 2) + (ox >> 1)
                up = flat[idx]
            else:
                up = o["add"][:, oy >> 1, ox >> 1]
            v = v + up.reshape(-1, Cout)
        relu = c["relu"]
        if fault == "relu_whole_quad":
            relu = -(-relu // 4) * 4
        v = torch.cat([v[:, :relu].clamp(min=0), v[:, relu:]], 1)
        outs.append(v)
    out = torch.cat(outs, 0)
    if fault == "small_channel_off":
        live = (out != 0).float().mean(0) > 0.25           # (a channel the ReLU empties has nothing to be off by)
        n = int(torch.where(live, out.abs().mean(0), torch.full((Cout,), math.inf)).argmin())
        out[:, n] *= 1.0 + 1e-3
    tiles = -(-out.shape[0] // bm)
    cs = torch.zeros(tiles, FR.c16(Cout))
    for t in range(tiles):
        if fault == "colsum_last_tile_missing" and t == tiles - 1:
            continue
        for r in range(t * bm, min(out.shape[0], (t + 1) * bm)):
            cs[t, :Cout] = cs[t, :Cout] + out[r]
    return out, cs


def _ratios(c, mode, **kw):
    o = FR.operands(c, mode)
    S, bm = c["want_S"], 16
    got, cs = emulate(c, o, mode, S=S, bm=bm, **kw)
    ref, mag, d = FR.reference(c, mode, o, c["launcher"], S)
    hard, rms = FR.check(got, ref, mag, d)
    return hard, rms, FR.colsum_check(cs, ref, mag, d, bm, c["Cout"])


# ---- the reference ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["S2-k_conv_igemm-2x12x14", "S2-k_conv_igemm-1x13x11", "ADD-k_conv_igemm-k3", "ADD-k_conv_igemm-k1",
                                 "AFF-k_conv_igemm-mul_add_relu_k3", "AFF-k_conv_igemm-mul_k1", "LEV-k_conv_igemm-3x3",
                                 "LEV+AFF-k_conv_igemm-3x3_Cout5", "TAIL-k_conv_igemm-Cout18_scalar"])
def test_reference_is_the_contract(cid):
    """fwd_ref against float64 F.conv2d per level and image, the affine, the nearest-2x addend and the ReLU written out."""
    F = torch.nn.functional
    c = BY_ID[cid]
    o = {k: v.double() for k, v in FR.operands(c, "fp32").items()}
    ref, mag = FR.fwd_ref(o["x"], o["w"], c["HW"], c["B"], stride=c["stride"], pad=c["pad"], scale=o.get("scale"), shift=o.get("shift"),
                          ep_stride=c["ep_stride"], relu_cout=c["relu"], in_mul=o.get("in_mul"), in_add=o.get("in_add"),
                          in_relu=c["aff"] == "mul_add_relu", add=o.get("add"))
    B, Cout, r0, q0 = c["B"], c["Cout"], 0, 0
    for l, (H, W) in enumerate(c["HW"]):
        for b in range(B):
            x = o["x"][r0:r0 + H * W].reshape(H, W, -1)
            r0 += H * W
            if "in_mul" in o:
                x = x * o["in_mul"][l * B + b]
                if "in_add" in o:
                    x = x + o["in_add"][l * B + b]
                if c["aff"] == "mul_add_relu":
                    x = x.clamp(min=0)
            y = F.conv2d(x.permute(2, 0, 1)[None], o["w"], None, c["stride"], c["pad"])[0].permute(1, 2, 0)
            e0 = l * c["ep_stride"]
            if "scale" in o:
                y = y * o["scale"].reshape(-1)[e0:e0 + Cout]
            if "shift" in o:
                y = y + o["shift"].reshape(-1)[e0:e0 + Cout]
            Ho, Wo = y.shape[:2]
            assert (Ho, Wo) == FR.out_hw(H, W, c["k"], c["stride"], c["pad"])
            if "add" in o:
                assert o["add"].shape[1:3] == (-(-Ho // 2), -(-Wo // 2))
                for oy in range(Ho):
                    for ox in range(Wo):
                        y[oy, ox] += o["add"][b, oy // 2, ox // 2]
            y[..., :c["relu"]] = y[..., :c["relu"]].clamp(min=0)
            want = y.reshape(-1, Cout)
            got = ref[q0:q0 + Ho * Wo]
            assert torch.allclose(got, want, rtol=1e-11, atol=1e-11 * float(want.abs().max())), (cid, l, b)
            assert bool((mag[q0:q0 + Ho * Wo] >= want.abs() * (1 - 1e-12)).all())
            q0 += Ho * Wo
    assert q0 == ref.shape[0] == FR.geometry(c)[4]


def test_operands_are_what_the_module_says():
    """Scales over about 1e6, negative scale entries, NaN in the epilogue vectors past Cout, and in_add / add as large as the term they
    join (the padding and addend-offset faults are then as large as the values they corrupt)."""
    c = BY_ID["LEV+AFF-k_conv_igemm-3x3_Cout5"]
    o = FR.operands(c, "fp32")
    assert o["scale"].shape == (3, 16) and bool(o["scale"][:, 5:].isnan().all()) and bool(o["shift"][:, 5:].isnan().all())
    c = BY_ID["ADD-k_conv_igemm-k3"]
    o = FR.operands(c, "fp32")
    sc = o["scale"][0, :40]
    assert bool((sc < 0).any()) and bool((sc > 0).any()) and float(sc.abs().max() / sc.abs().min()) > 1e4
    sx = o["x"].abs().amax(0)
    assert float(sx.max() / sx.min()) > 1e4
    ref, _, _ = FR.reference(dict(c, add=False, relu=0), "fp32", {k: v for k, v in o.items() if k != "add"}, "k_conv_igemm", 1)
    ratio = o["add"].double().reshape(-1, 40).pow(2).mean(0).sqrt() / ref.pow(2).mean(0).sqrt()
    assert 0.2 < float(ratio.min()) and float(ratio.max()) < 5, ratio
    c = BY_ID["AFF-k_conv_igemm-mul_add_k3"]
    o = FR.operands(c, "fp32")
    ratio = o["in_add"].double().pow(2).mean(0).sqrt() / (o["x"].double().pow(2).mean(0).sqrt() * o["in_mul"].double().abs().mean(0))
    assert 0.3 < float(ratio.median()) < 3, ratio         # (two images: two draws per channel)


@pytest.mark.parametrize("cid", [c["id"] for c in CASES if c["aff"] is not None])
def test_bf16_affine_operands_are_exact(cid):
    c = BY_ID[cid]
    o = FR.operands(c, "bf16")
    assert FR.affine_is_exact(o["x"], o["in_mul"], o.get("in_add"), c["B"], c["HW"])
    assert float(o["x"].abs().max()) < 64 and bool((o["x"] * 64 == (o["x"] * 64).round()).all())
    m = o["in_mul"].abs().log2()
    assert bool((m == m.round()).all()) and float(m.abs().max()) <= 2
    # and the fp32-mode operands of the same case are not (the property is the operands', not the check's)
    o32 = FR.operands(c, "fp32")
    assert not FR.affine_is_exact(o32["x"], o32["in_mul"], o32.get("in_add"), c["B"], c["HW"])


# ---- the emulation passes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,mode", [(c["id"], m) for c in EMU for m in c["modes"]])
def test_fp32_emulation_passes_every_bound(cid, mode):
    hard, rms, cs = _ratios(BY_ID[cid], mode)
    assert hard < 0.25 and rms < 0.5 and cs < 0.25, (hard, rms, cs)


def test_emulation_covers_every_class():
    assert {c["cls"] for c in EMU} == {c["cls"] for c in CASES}


def test_bf16_emulation_fails_against_the_fp32_reference():
    c = BY_ID["S2-k_conv_igemm-2x12x14"]
    o = FR.operands(c, "bf16")
    got, _ = emulate(c, o, "bf16")
    ref, mag, d = FR.reference(c, "fp32", o, c["launcher"], 1)
    assert FR.check(got, ref, mag, d)[0] > 1


# ---- seeded faults ---------------------------------------------------------------------------------------------------------------------
FAULTS = [
    ("pad_gets_in_add", "AFF-k_conv_igemm-mul_add_k3", "fp32"),
    ("pad_gets_in_add", "AFF-k_conv_igemm-mul_add_relu_k3", "bf16"),
    ("add_at_oy_ox", "ADD-k_conv_igemm-k3", "fp32"),
    ("add_at_oy_ox", "ADD-k_conv_igemm-k1", "bf16"),
    ("add_floor_dims", "ADD-k_conv_igemm-k3", "fp32"),
    ("relu_whole_quad", "ADD-k_conv_igemm-k3", "fp32"),
    ("relu_whole_quad", "TAIL-k_conv_igemm-Cout18_scalar", "bf16"),
    ("level1_scale_of_level0", "LEV-k_conv_igemm-3x3", "fp32"),
    ("level1_in_mul_of_level0", "LEV+AFF-k_conv_igemm-3x3_Cout5", "fp32"),
    ("in_mul_by_b", "LEV+AFF-k_conv_igemm-3x3_Cout5", "fp32"),
    ("in_mul_by_b", "LEV+AFF-k_conv_igemm-3x3_Cout5", "bf16"),
    ("s2_window_shifted", "S2-k_conv_igemm-2x12x14", "fp32"),
    ("small_channel_off", "S2-k_conv_igemm-2x12x14", "fp32"),
    ("small_channel_off", "LEV-k_conv3x3_wino-3x3", "fp32"),
]


@pytest.mark.parametrize("fault,cid,mode", FAULTS)
def test_seeded_fault_exceeds_a_bound(fault, cid, mode):
    c = BY_ID[cid]
    ok = _ratios(c, mode)
    assert ok[0] <= 1 and ok[1] <= 1
    hard, rms, _ = _ratios(c, mode, fault=fault)
    assert hard > 1 or rms > 1, (fault, hard, rms)


@pytest.mark.parametrize("cid", ["COLSUM-k_conv_igemm-k3", "COLSUM-k_conv_gd-k1_bm128", "COLSUM/splitk-k_conv_kw-k3_S3"])
def test_missing_last_tile_exceeds_the_colsum_bound(cid):
    c = BY_ID[cid]
    assert _ratios(c, "fp32")[2] <= 1
    hard, rms, cs = _ratios(c, "fp32", fault="colsum_last_tile_missing")
    assert hard <= 1 and rms <= 1 and cs > 1, (hard, rms, cs)


def test_small_channel_fault_is_invisible_to_the_max_norm():
    """The measure of tests/test_hip_parity.py (max |a - b| / max |b| < 1e-4) passes the fault the block rms catches."""
    c = BY_ID["S2-k_conv_igemm-2x12x14"]
    o = FR.operands(c, "fp32")
    got, _ = emulate(c, o, "fp32", fault="small_channel_off")
    ref, mag, d = FR.reference(c, "fp32", o, c["launcher"], 1)
    assert float((got.double() - ref).abs().max() / ref.abs().max()) < 1e-4
    assert FR.check(got, ref, mag, d)[1] > 1


def test_colsum_check_requires_zero_past_cout():
    ref, mag = torch.ones(32, 5, dtype=torch.float64), torch.ones(32, 5, dtype=torch.float64)
    cs = torch.zeros(2, 16)
    cs[:, :5] = 16
    assert FR.colsum_check(cs, ref, mag, 10, 16, 5) == 0
    cs[1, 7] = 1e-30
    assert FR.colsum_check(cs, ref, mag, 10, 16, 5) == math.inf


# ---- the case table against the planner ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oh():
    import os
    import orehip
    if not os.path.exists(orehip.LIB_PATH):
        orehip.build()
    orehip.lib()
    return orehip


def _fake_ptrs(c, L):
    ptr = {"in": 0x10000000, "w": 0x20000000, "out": 0x30000000, "workspace": 0x40000000, "workspace_floats": L.ore_conv_workspace_floats()}
    for name, on, addr in (("scale", c["scale"], 0x50000040), ("shift", c["shift"], 0x51000040), ("in_mul", c["aff"], 0x52000040),
                           ("in_add", c["aff"] not in (None, "mul"), 0x53000040), ("add", c["add"], 0x54000000),
                           ("colsum", c["colsum"], 0x55000000), ("w_wino", c["wino"], 0x56000000)):
        if on:
            ptr[name] = addr
    return ptr


def test_case_table_plans_on_its_launchers(oh):
    """ore_conv_plan puts every case on its launcher with its split in the modes the table names, and not in the mode it leaves out: a
    refused (mode, launcher) pair is a row of the table, not a skip at run time."""
    L = oh.lib()
    prev = oh.get_conv_precision()
    bad = []
    try:
        for c in CASES:
            for mode in ("fp32", "bf16"):
                oh.set_conv_precision(mode)
                d, pl = oh.ConvDesc(), oh.ConvPlan()
                nl, H, W, ep = FR.fill_desc(d, c, _fake_ptrs(c, L))
                with oh.conv_overrides(*c["ov"]):
                    rc = L.ore_conv_plan(C.byref(d), nl, oh._i32s(H) if nl else None, oh._i32s(W) if nl else None, ep, C.byref(pl))
                hit = rc == 0 and oh.CONV_LAUNCHERS[pl.launcher] == c["launcher"] and pl.splitk == c["want_S"]
                if hit != (mode in c["modes"]):
                    bad.append((c["id"], mode, rc, oh.CONV_LAUNCHERS[pl.launcher], pl.splitk))
                if hit and c["colsum"]:
                    tiles = -(-FR.geometry(c)[4] // pl.bm)
                    if tiles < 2 or FR.geometry(c)[4] % pl.bm == 0:
                        bad.append((c["id"], mode, "column sums need a ragged last tile and two tiles", pl.bm))
    finally:
        oh.set_conv_precision(prev)
    assert not bad, bad


def test_case_table_is_the_feature_table():
    """Class by launcher as the module's docstring states it, sizes within the limits, ids unique, and the GPU module's literal
    EXPECTED set is the table's."""
    import test_hip_fwdconv as G
    assert len(BY_ID) == len(CASES)
    by = {}
    for c in CASES:
        by.setdefault(c["cls"], set()).add(c["launcher"])
        assert FR.geometry(c)[4] <= 1500 and c["k"] * c["k"] * c["Cin"] <= 1152, c["id"]
    assert by["S2"] == by["ADD"] == by["COLSUM"] == set(FR.DMA6)
    assert by["AFF"] == by["LEV+AFF"] == {"k_conv_igemm"}
    assert by["TAIL"] == {"k_conv_igemm", "k_conv_kw", "k_conv_gs", "k_conv_kd", "k_conv_rf"} | set(FR.TILE)
    assert by["LEV"] == {"k_conv_igemm", "k_conv_kw", "k_conv_gd", "k_conv_kd"} | set(FR.TILE)
    assert by["ADD/splitk"] == by["COLSUM/splitk"] == {"k_conv_igemm", "k_conv_kw"}
    assert FR.expected_cells() == G.EXPECTED, (sorted(FR.expected_cells() - G.EXPECTED), sorted(G.EXPECTED - FR.expected_cells()))


def test_refused_pairs_are_refused(oh):
    """The (class, launcher) pairs the table leaves out because the planner declines them (fwdconv_ref.REFUSED): with the launcher's
    own override codes the call is planned on another launcher."""
    L = oh.lib()
    trials = []
    for la in FR.DMA6[1:] + FR.TILE:
        trials.append((dict(BY_ID["AFF-k_conv_igemm-mul_add_relu_k3"], Cin=FR.TILE_CIN.get(la, 64), Cout=64), la))
        trials.append((dict(BY_ID["LEV+AFF-k_conv_igemm-3x3_Cout5"], Cin=FR.TILE_CIN.get(la, 64), Cout=64, ep_stride=64), la))
    for la in FR.TILE:
        for cid in ("ADD-k_conv_igemm-k3", "COLSUM-k_conv_igemm-k3"):
            trials.append((dict(BY_ID[cid], Cin=FR.TILE_CIN.get(la, 64), Cout=64), la))
    for la in ("k_conv_gd", "k_conv_kd", "k_conv_rf"):
        trials.append((BY_ID["LEV-k_conv_igemm-3x3"], la))
    bad = []
    for c, la in trials:
        c = dict(c, ov=FR.OV[la][0], wino=la.startswith("k_conv3x3_wino"))
        d, pl = oh.ConvDesc(), oh.ConvPlan()
        nl, H, W, ep = FR.fill_desc(d, c, _fake_ptrs(c, L))
        with oh.conv_overrides(*c["ov"]):
            rc = L.ore_conv_plan(C.byref(d), nl, oh._i32s(H) if nl else None, oh._i32s(W) if nl else None, ep, C.byref(pl))
        if rc != 0 or oh.CONV_LAUNCHERS[pl.launcher] == la:
            bad.append((c["cls"], la, rc, oh.CONV_LAUNCHERS[pl.launcher]))
    assert not bad, bad
