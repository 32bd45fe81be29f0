"""GPU: the Winograd kernels' input addressing (buffer descriptors: out-of-image taps are the descriptor's out-of-range zeros).

A. every case of tests/wino_cases.py is bit-identical to what the kernels computed before they moved to descriptors
   (tests/golden/wino_parent_sha256.json, tools/gen_wino_parent_hashes.py);
B. nothing outside the tensor is used: with NaN in front of it, behind it and in the channels outside the slice the result is finite,
   the same bit for bit, and the output's neighbours keep their sentinel;
C. every case against F.conv2d on float64 inputs at the file-wide tolerance of tests/test_hip_parity.py."""
import functools
import json
import os

import pytest
import torch

import wino_cases as wc
from conftest import GOLDEN, rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4                                          # tests/test_hip_parity.py
IDS = [c["id"] for c in wc.CASES]


@pytest.fixture(scope="module")
def ore():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import orehip
    orehip.lib()
    with orehip.conv_overrides((-7, 2)):
        yield orehip


@functools.lru_cache(maxsize=None)
def _data(i):
    return wc.make(wc.CASES[i])


@functools.lru_cache(maxsize=None)
def _plain(i):
    """The case's output, computed once and shared by the tests (never modified)."""
    import orehip
    return wc.run(orehip, wc.CASES[i], _data(i))


@functools.lru_cache(maxsize=None)
def _reference(i):
    return wc.reference(wc.CASES[i], _data(i))


def _payload(case, out_rows):
    ld, coff = wc.out_geometry(case)
    return out_rows[:, coff:coff + wc.cout_of(case["cin"])]


def _err(i, out_rows):
    return rel_err(_payload(wc.CASES[i], out_rows).numpy(), _reference(i).numpy())


@pytest.fixture(scope="module")
def parent():
    with open(os.path.join(GOLDEN, "wino_parent_sha256.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("i", range(len(wc.CASES)), ids=IDS)
def test_bit_identical_to_parent(ore, parent, i):
    case = wc.CASES[i]
    got = wc.digest(_plain(i))
    assert got == parent["sha256"][case["id"]], (
        f"{case['id']}: output differs from the one recorded at {parent['commit']} (ore_version {parent['ore_version']}); "
        f"relative error against float64 F.conv2d: {_err(i, _plain(i)):.3e}")


@pytest.mark.parametrize("i", [k for k, c in enumerate(wc.CASES) if c["multi"]], ids=[c["id"] for c in wc.GUARDED])
def test_nothing_outside_the_tensor_is_used(ore, i):
    case = wc.CASES[i]
    got = wc.run(ore, case, _data(i), guarded=True)
    ld, coff = wc.out_geometry(case)
    cout = wc.cout_of(case["cin"])
    assert bool(torch.isfinite(got).all()), f"{case['id']}: a NaN from outside the tensor reached the output"
    assert torch.equal(got, _plain(i)), f"{case['id']}: the result depends on memory outside the tensor (error {_err(i, got):.3e})"
    assert float(got[:, :coff].min()) == wc.SENTINEL and float(got[:, :coff].max()) == wc.SENTINEL
    assert float(got[:, coff + cout:].min()) == wc.SENTINEL and float(got[:, coff + cout:].max()) == wc.SENTINEL


@pytest.mark.parametrize("i", range(len(wc.CASES)), ids=IDS)
def test_against_float64_reference(ore, i):
    case = wc.CASES[i]
    out = _plain(i)
    ld, coff = wc.out_geometry(case)
    cout = wc.cout_of(case["cin"])
    e = _err(i, out)
    print(f"{case['id']}: rel err {e:.3e}")
    assert e < TOL
    assert float(out[:, :coff].min()) == wc.SENTINEL and float(out[:, :coff].max()) == wc.SENTINEL
    assert float(out[:, coff + cout:].min()) == wc.SENTINEL and float(out[:, coff + cout:].max()) == wc.SENTINEL
