"""MORE_POS on the host (no GPU): the float64 restatement of tests/more_pos_ref.py reproduces the list the executed reference returned for
every fixture tests/golden/cn_more_pos_*.npz, the fixtures' seeds keep the margin that makes that comparison exact, the three losses the
reference returned agree with the float64 restatement of the loss kernels fed that list, and the configuration surface: MORE_POS is
accepted, a MORE_POS_TOPK outside 1 .. 9 L says what to set, NOT_NMS / CENTER_NMS stay refused, the new yaml loads, the header declares
the new entry point."""
import os
import re

import numpy as np
import pytest
import torch

import more_pos_ref as MP
import trainloss_ref as TL
from conftest import PKG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _case(name):
    return MP.load_case(os.path.join(GOLD, f"cn_more_pos_{name}.npz"))


@pytest.mark.parametrize("name", MP.CASES)
def test_restatement_reproduces_the_reference_list(name):
    c = _case(name)
    r = MP.more_pos_ref(c["gt"], c["counts"], c["head"], c["shapes"], c["strides"], c["soi"], c["thresh"], c["topk"])
    print(name, "positives", len(c["pos_inds"]), "worst margin ratio", r["worst"], "inside the margin", r["near"], "soi margin", r["soi_margin"])
    assert r["pos_inds"].dtype == np.int64 and np.array_equal(r["pos_inds"], c["pos_inds"])
    assert c["pos_inds"].size == 0 or (0 <= c["pos_inds"].min() and c["pos_inds"].max() < c["head"].shape[0])
    if name not in MP.NO_MARGIN:
        assert r["near"] == 0 and r["worst"] < 1.0, (r["near"], r["worst"])
        assert r["soi_margin"] >= TL.CN_MARGIN
        assert not np.isnan(r["loss"].v).any()
    else:
        assert np.isnan(r["loss"].v).any()                      # the case is there for the NaN order of torch.kthvalue


def test_fixtures_cover_the_cases():
    """What each case is there for is true of its data."""
    a = _case("a")
    assert a["counts"].tolist() == [7, 0]
    b = _case("b")
    cb = MP.candidates(b["gt"], b["counts"], b["shapes"], b["strides"], b["soi"])
    assert (cb["rows"] < 0).any(axis=(1, 2)).all()               # every object has a neighbour outside the map
    c = _case("c")
    cc = MP.candidates(c["gt"], c["counts"], c["shapes"], c["strides"], c["soi"])
    assert (cc["target"][0, 0] < 0).any() and float(c["gt"][0, 0, 2] - c["gt"][0, 0, 0]) < 8
    d = _case("d")
    assert MP.candidates(d["gt"], d["counts"], d["shapes"], d["strides"], d["soi"])["level_mask"][0].tolist() == [True, True, False]
    for name in ("a", "e", "g27", "j"):                          # rows named more than once
        p = _case(name)["pos_inds"]
        assert len(p) > len(np.unique(p)), name
    e = _case("e")
    ce = MP.candidates(e["gt"], e["counts"], e["shapes"], e["strides"], e["soi"])
    assert len(np.intersect1d(ce["rows"][0][ce["rows"][0] >= 0], ce["rows"][1][ce["rows"][1] >= 0])) > 0
    f = _case("f")
    rf = MP.more_pos_ref(f["gt"], f["counts"], f["head"], f["shapes"], f["strides"], f["soi"], f["thresh"], f["topk"])
    assert (rf["loss"].v[0] < 0.2).sum() > f["topk"] and rf["thresh_eff"][0] < 0.2          # the k-th value binds
    assert rf["thresh_eff"][1] == np.float64(np.float32(0.2)) and rf["sel"][1].sum() == rf["cand"]["level_mask"][1].sum()
    g1 = _case("g1")
    assert g1["topk"] == 1 and g1["pos_inds"].size == 0          # a real centre: the threshold is 0, nothing is strictly below
    assert _case("g27")["topk"] == 27
    h = _case("h")
    assert h["strides"] == (4,) and h["soi"] == ((0.0, 1000000.0),) and h["shapes"] == [(40, 48)]
    for n in ("i", "i27"):
        i = _case(n)
        assert float(i["gt"][0, 0, 0]) == float(i["gt"][0, 0, 2])
    assert _case("i27")["topk"] == 27
    assert _case("j")["counts"].tolist() == [128]


@pytest.mark.parametrize("name", [n for n in MP.CASES if n not in MP.NO_MARGIN])
def test_reference_losses_agree_with_the_float64_losses(name):
    """The three losses the reference's forward returned against the float64 restatement of the loss kernels (tests/trainloss_ref.py)
    fed the fixture's list: the element bound of that file, 3 more roundings for weight / normaliser."""
    c = _case(name)
    tg = TL.centernet_targets_ref(c["gt"], c["counts"], c["shapes"], c["strides"], c["soi"])
    npos = len(c["pos_inds"])
    ref = TL.centernet_losses_ref(c["head"], tg["reg_targets"], tg["hm"].v.astype(np.float32), c["pos_inds"], np.array([npos]))
    den_reg, den_pos = max(ref["count"], 1), max(npos, 1)
    want = {"giou": (1.0 / den_reg, 0), "pos": (-0.5 * 0.25 / den_pos, 1), "neg": (-0.5 * 0.75 / den_pos, 2)}
    for k, (w, i) in want.items():
        x = TL.X(ref[k].v * w, ref[k].m * abs(w), ref[k].d)
        hard, _ = TL.hold(torch.tensor([c["losses"][i]], dtype=torch.float64), x, extra_d=3 + tg["hm"].d)
        print(name, k, "reference", c["losses"][i], "float64", float(x.v), "hard ratio", hard)
        assert hard <= 1.0, (name, k, hard)


def _cfg(*extra, yaml="finetune_vovnet_more_pos.yaml"):
    from fewx.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(PKG, "configs", "fsod", yaml))
    cfg.merge_from_list(list(extra))
    cfg.freeze()
    return cfg


def _centernet(cfg):
    from detectron2.layers import ShapeSpec
    from fewx.modeling.fsod.fsod_rpn import CenterNet
    return CenterNet(cfg, {f: ShapeSpec(channels=cfg.MODEL.FPN.OUT_CHANNELS, stride=s)
                           for f, s in zip(cfg.MODEL.CENTERNET.IN_FEATURES, cfg.MODEL.CENTERNET.FPN_STRIDES)})


def test_yaml_loads_and_more_pos_is_accepted():
    cfg = _cfg()
    base = _cfg(yaml="finetune_vovnet.yaml")
    assert cfg.MODEL.CENTERNET.MORE_POS is True and base.MODEL.CENTERNET.MORE_POS is False
    assert cfg.MODEL.CENTERNET.MORE_POS_THRESH == 0.2 and cfg.MODEL.CENTERNET.MORE_POS_TOPK == 9
    a, b = cfg.clone(), base.clone()
    a.defrost(); b.defrost()
    a.MODEL.CENTERNET.MORE_POS = False
    assert a == b                                                # the switch is the only difference
    pg = _centernet(cfg)
    assert pg.more_pos is True and pg.more_pos_thresh == 0.2 and pg.more_pos_topk == 9
    assert _centernet(base).more_pos is False


@pytest.mark.parametrize("topk", [0, 28, -3])
def test_topk_outside_the_candidates_says_what_to_set(topk):
    with pytest.raises(ValueError, match=r"MORE_POS_TOPK.*1 \.\. 27"):
        _centernet(_cfg("MODEL.CENTERNET.MORE_POS_TOPK", topk))
    for ok in (1, 27):
        assert _centernet(_cfg("MODEL.CENTERNET.MORE_POS_TOPK", ok)).more_pos_topk == ok


@pytest.mark.parametrize("key", ["NOT_NMS", "CENTER_NMS"])
def test_the_other_two_switches_stay_refused(key):
    with pytest.raises(NotImplementedError, match="NOT_NMS and CENTER_NMS"):
        _centernet(_cfg(f"MODEL.CENTERNET.{key}", True))


def test_header_and_binding_declare_the_entry_point():
    with open(os.path.join(ROOT, "include", "ore_hip.h")) as f:
        src = f.read()
    m = re.search(r"int\s+ore_centernet_more_pos_fwd\s*\(([^;]*)\)\s*;", src)
    assert m is not None
    params = " ".join(m[1].split())
    for p in ("const float* head", "int32_t head_ld", "float more_pos_thresh", "int32_t more_pos_topk", "int64_t* pos_inds",
              "int32_t* pos_count", "void* stream"):
        assert p in params, p
    import orehip
    assert "ore_centernet_more_pos_fwd" in orehip.SYMBOLS
    import inspect
    assert "more_pos" in inspect.signature(orehip.centernet_targets).parameters
