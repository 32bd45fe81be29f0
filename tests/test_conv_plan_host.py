"""CPU: ore_conv_plan reproduces, call for call, the conv plans recorded in tests/golden/conv_plan_table.json.

The table holds every distinct ore_conv2d_fwd / ore_conv2d_levels_fwd call of the GPU conv test modules and one bench.py run, as the
launch code chose them before the host-side planner existed: launcher, tile, build, split-K, steps per split, XCD mapping and grid, or
the error code, under the tuning-aid settings in force.  Each row is replayed here with fake pointers that have the recorded nullness
and address residues (only those are planned on); no GPU is touched."""
import ctypes as C
import json
import os

import pytest

from conftest import GOLDEN

LAUNCHERS = 15          # ORE_LAUNCH_NONE .. ORE_LAUNCH_WS_SB
PTRS = ("in_", "w", "scale", "shift", "in_mul", "in_add", "add", "out", "workspace", "colsum", "w_wino")
INTS = ("in_ld", "in_coff", "B", "H", "W", "Cin", "Cout", "kh", "kw", "stride", "pad", "relu_cout", "in_relu", "add_ld", "add_coff",
        "out_ld", "out_coff", "splitk", "storage", "workspace_floats", "w_wino_level_stride", "w_level_stride")


@pytest.fixture(scope="module")
def table():
    with open(os.path.join(GOLDEN, "conv_plan_table.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def L():
    import orehip
    if not os.path.exists(orehip.LIB_PATH):
        orehip.build()
    return orehip.lib()


def _desc(rec, i):
    import orehip
    fn, nl, lv, ep, ints, ptrs = rec
    d = orehip.ConvDesc()
    for k, v in zip(INTS, ints):
        setattr(d, k, v)
    for j, (k, r) in enumerate(zip(PTRS, ptrs)):
        setattr(d, k, None if r < 0 else (0x10000000 * (j + 1) + (i % 4096) * 0x10000 + r))   # distinct fake addresses, recorded residue mod 64
    return d, fn, nl, lv, ep


def test_table_reaches_every_launcher(table):
    assert {r[4][0] for r in table["rows"] if r[3] == 0} == set(range(1, LAUNCHERS))


def test_plans_match_recorded_with_full_overrides(table, L):
    import orehip
    bad = []
    try:
        for i, (di, prec, ki, rc, plan) in enumerate(table["rows"]):
            d, fn, nl, lv, ep = _desc(table["descs"][di], i)
            L.ore_conv_reset_plan_overrides()
            assert L.ore_conv_set_precision(prec) == 0
            knobs = table["knobs"][ki]
            for code in sorted((int(c) for c in knobs), key=lambda c: (c == 0, -c)):   # -1, -2, ..., -16, then the k_conv_igemm tile (0)
                args = (code, *knobs[str(code)]) if code else tuple(knobs[str(code)])
                args += (0,) * (5 - len(args))            # padded with zeros to its five arguments, as orehip.conv_overrides does
                assert L.ore_conv_set_plan_override(*args) == 0
            pl = orehip.ConvPlan()
            if fn == 0:
                got_rc = L.ore_conv_plan(C.byref(d), 0, None, None, 0, C.byref(pl))
            else:
                n = max(nl, 0)
                H, W = (C.c_int32 * 4)(*[h for h, _ in lv]), (C.c_int32 * 4)(*[w for _, w in lv])
                got_rc = L.ore_conv_plan(C.byref(d), n if n else -1, H, W, ep, C.byref(pl))
            got = (pl.launcher,) if rc else pl.astuple()
            if got_rc != rc or got != tuple(plan) or pl.error != rc:
                bad.append((i, table["descs"][di], prec, knobs, rc, plan, got_rc, got))
    finally:
        L.ore_conv_reset_plan_overrides()
        L.ore_conv_set_precision(0)
    assert not bad, f"{len(bad)} of {len(table['rows'])} plans differ, first: {bad[:3]}"
