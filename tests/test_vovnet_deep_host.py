"""CPU checks of the deep VoVNet bodies (V-39-eSE, V-57-eSE, V-99-eSE): the oracle's restatement (oracle/ref_model.py, identity blocks
included) against the fixtures recorded from the executed reference (tools/gen_golden_vovnet_deep.py), the module tree against the
reference's state-dict names, the shipped config, and the recorded own-error figures the stage-wise GPU test hangs its tolerance on."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, PKG, chan_err, rel_err
from oracle import ref_model as R

TOL = 1e-4      # tests/test_hip_parity.py's figure for fp32 feature maps
BODIES = ("V-39-eSE", "V-57-eSE", "V-99-eSE")
P = "backbone.bottom_up."


def _cfg(body=None, yaml="finetune_vovnet_v39.yaml"):
    from fewx.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(PKG, "configs", "fsod", yaml))
    cfg.merge_from_list(["MODEL.DEVICE", "cpu"] + (["MODEL.VOVNET.CONV_BODY", body] if body else []))
    return cfg


def _close(got, want, what):
    r, c = rel_err(got, want), chan_err(got, want)
    assert r < TOL and c < TOL, (what, r, c)


def _stage(x, sd, body, k):
    """Stage k of the restatement alone: the max-pool and the chain of OSA blocks, the blocks behind the first with their identity."""
    spec = R.VOVNET_SPECS[body]
    z = F.max_pool2d(x, 3, 2, ceil_mode=True)
    for b in range(spec["blocks"][k - 2]):
        mod = f"OSA{k}_{b + 1}"
        z = R.osa_module(z, sd, f"{P}stage{k}.{mod}.", mod, spec["layers"], identity=b > 0)
    return z


def test_restatement_reproduces_backbone_fixture(golden):
    fx = golden("backbone_fpn_v39_96x128")
    sd = R.synth_state_dict(int(fx["seed"]), "V-39-eSE")
    with torch.no_grad():
        out = R.backbone_fpn(torch.from_numpy(fx["x"]), sd, body="V-39-eSE")
    for k in ("p3", "p4", "p5"):
        _close(out[k].numpy(), fx[k], k)


@pytest.mark.parametrize("body,tag", [("V-39-eSE", "v39"), ("V-57-eSE", "v57")])
def test_restatement_reproduces_unit_fixtures(golden, body, tag):
    fx = golden("deep_units")
    sd = R.synth_state_dict(int(fx[tag + "_seed"]), body)
    with torch.no_grad():
        for k in (4, 5):
            y = _stage(torch.from_numpy(fx[f"stage{k}_x"]), sd, body, k)
            assert tuple(y.shape) == tuple(fx[f"{tag}_stage{k}_y"].shape)
            _close(y.numpy(), fx[f"{tag}_stage{k}_y"], (body, k))


def test_whole_backbone_and_units_share_the_v39_seed(golden):
    assert int(golden("deep_units")["v39_seed"]) == int(golden("backbone_fpn_v39_96x128")["seed"])


@pytest.mark.parametrize("body", BODIES)
def test_module_tree_has_the_reference_names(body):
    from detectron2.layers import ShapeSpec
    from detectron2.modeling.backbone.vovnet import build_fcos_vovnet_fpn_backbone
    with open(os.path.join(GOLDEN, "vovnet_deep_state_keys.json")) as f:
        want = json.load(f)[body]
    bb = build_fcos_vovnet_fpn_backbone(_cfg(body), ShapeSpec(channels=3))
    got = {k: list(v.shape) for k, v in bb.state_dict().items()}
    assert sorted(got) == sorted(want), (sorted(set(got) ^ set(want))[:8])
    assert got == want
    # the identity blocks are there under the reference's names: one per block behind the first of a stage
    blocks = R.VOVNET_SPECS[body]["blocks"]
    for si, n in enumerate(blocks):
        k = si + 2
        assert f"bottom_up.stage{k}.OSA{k}_{n}.ese.fc.weight" in want and f"bottom_up.stage{k}.OSA{k}_{n + 1}.ese.fc.weight" not in want
    # a reference-layout state dict loads strictly
    sd = R.synth_state_dict(0, body)
    bb.load_state_dict({k[len("backbone."):]: v for k, v in sd.items() if k.startswith("backbone.")}, strict=True)


def test_shipped_yaml_resolves():
    cfg = _cfg()
    base = _cfg(yaml="finetune_vovnet.yaml")
    assert cfg.MODEL.VOVNET.CONV_BODY == "V-39-eSE"
    cfg.MODEL.VOVNET.CONV_BODY = base.MODEL.VOVNET.CONV_BODY
    assert cfg.dump() == base.dump()                                   # the body is the only difference


def test_own_error_record_covers_every_deep_stage(golden):
    """deep_own_error.json: the executed reference's fp32 error against fp64 for every multi-block stage of V-57 and V-99, run alone."""
    with open(os.path.join(GOLDEN, "deep_own_error.json")) as f:
        rec = json.load(f)
    assert sorted(rec) == ["V-57-eSE", "V-99-eSE", "stagewise_input"]
    for body in ("V-57-eSE", "V-99-eSE"):
        r = rec[body]
        deep = [f"stage{si + 2}" for si, n in enumerate(R.VOVNET_SPECS[body]["blocks"]) if n > 1]
        assert sorted(r) == sorted(deep + ["seed"]), (body, sorted(r))
        assert all(0.0 < r[s] < 1e-2 for s in deep), r
    # the image of the stage-wise GPU test: one per body, picked where the executed reference's own stages are within TOL / 4 of fp64
    picks = rec["stagewise_input"]
    assert sorted(picks) == sorted(BODIES)
    seeds = {"V-39-eSE": int(golden("backbone_fpn_v39_96x128")["seed"]), "V-57-eSE": rec["V-57-eSE"]["seed"], "V-99-eSE": rec["V-99-eSE"]["seed"]}
    for body, p in picks.items():
        assert 0.0 < p["own"] < TOL / 4 and p["image_std"] == 0.25 and p["weights_seed"] == seeds[body], (body, p)
