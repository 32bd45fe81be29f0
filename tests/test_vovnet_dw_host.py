"""CPU checks of the depthwise VoVNet bodies (V-19-slim-dw-eSE, V-19-dw-eSE): the plain-torch restatement (tests/vovnet_dw_ref.py)
against the fixtures recorded from the executed reference, the module tree against the reference's state-dict names, the shipped
config, the bf16 refusal and the FLOP helper."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, PKG, chan_err, rel_err
import vovnet_dw_ref as D

TOL = 1e-4      # tests/test_hip_parity.py's figure for fp32 feature maps
BODIES = list(D.DW_SPECS)


def _cfg(body=None, yaml="finetune_vovnet_dw.yaml"):
    from fewx.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(PKG, "configs", "fsod", yaml))
    cfg.merge_from_list(["MODEL.DEVICE", "cpu"] + (["MODEL.VOVNET.CONV_BODY", body] if body else []))
    return cfg


def _backbone(body):
    from detectron2.layers import ShapeSpec
    from detectron2.modeling.backbone.vovnet import build_fcos_vovnet_fpn_backbone
    return build_fcos_vovnet_fpn_backbone(_cfg(body), ShapeSpec(channels=3))


def _close(got, want, what):
    r, c = rel_err(got, want), chan_err(got, want)
    assert r < TOL and c < TOL, (what, r, c)


def test_restatement_reproduces_backbone_fixture(golden):
    fx = golden("backbone_fpn_dw_96x128")
    sd = D.synth_state_dict_dw(int(fx["seed"]), "V-19-slim-dw-eSE")
    with torch.no_grad():
        out = D.backbone_fpn_dw(torch.from_numpy(fx["x"]), sd)
    for k in ("p3", "p4", "p5"):
        _close(out[k].numpy(), fx[k], k)


def test_restatement_reproduces_unit_fixtures(golden):
    fx = golden("dw_units")
    sd = D.synth_state_dict_dw(int(fx["seed"]), "V-19-slim-dw-eSE")
    t = lambda k: torch.from_numpy(fx[k])
    with torch.no_grad():
        _close(D.dw_unit(t("stem2_x"), sd, D.P + "stem.stem_2", 1).numpy(), fx["stem2_y"], "stem_2")
        y3 = D.dw_unit(t("stem3_x"), sd, D.P + "stem.stem_3", 2)
        assert tuple(y3.shape) == (1, 64, 13, 19)                      # odd size: (H - 1) / 2 + 1
        _close(y3.numpy(), fx["stem3_y"], "stem_3")
        _close(D.osa_stage_dw(t("stage3_x"), sd, 3).numpy(), fx["stage3_y"], "stage3")
        _close(D.osa_stage_dw(t("stage5_x"), sd, 5).numpy(), fx["stage5_y"], "stage5")


@pytest.mark.parametrize("body", BODIES)
def test_module_tree_has_the_reference_names(body):
    with open(os.path.join(GOLDEN, "vovnet_dw_state_keys.json")) as f:
        rec = json.load(f)
    bb = _backbone(body)
    got = {k: list(v.shape) for k, v in bb.state_dict().items()}
    want = rec[body]
    assert sorted(got) == sorted(want), (sorted(set(got) ^ set(want))[:8])
    assert got == want
    assert len(want) == {"V-19-slim-dw-eSE": 144, "V-19-dw-eSE": 149}[body]
    # a reference-layout state dict loads strictly
    sd = D.synth_state_dict_dw(0, body)
    bb.load_state_dict({k[len("backbone."):]: v for k, v in sd.items() if k.startswith("backbone.")}, strict=True)
    # FREEZE_AT 3: stem, stage2, stage3 frozen; stage4 / stage5 train -- exactly the reference's trainable set
    trainable = sorted(n for n, p in bb.named_parameters() if p.requires_grad and n.startswith("bottom_up."))
    assert trainable == rec[body + "/trainable"]
    for n, p in bb.bottom_up.named_parameters():
        assert p.requires_grad == n.startswith(("stage4.", "stage5.")), n
    assert any("dw_conv3x3" in n for n in trainable) and any("conv_reduction" in n for n in trainable)


def test_dense_bodies_are_untouched():
    from detectron2.modeling.backbone.vovnet import _STAGE_SPECS
    assert not any(v.get("dw") for k, v in _STAGE_SPECS.items() if "-dw-" not in k)
    from oracle import ref_model as R
    from detectron2.layers import ShapeSpec
    from detectron2.modeling.backbone.vovnet import build_fcos_vovnet_fpn_backbone
    bb = build_fcos_vovnet_fpn_backbone(_cfg(yaml="finetune_vovnet.yaml"), ShapeSpec(channels=3))
    sd = R.synth_state_dict(0)
    bb.load_state_dict({k[len("backbone."):]: v for k, v in sd.items() if k.startswith("backbone.")}, strict=True)


def test_shipped_yaml_resolves():
    cfg = _cfg()
    base = _cfg(yaml="finetune_vovnet.yaml")
    assert cfg.MODEL.VOVNET.CONV_BODY == "V-19-slim-dw-eSE"
    assert list(cfg.MODEL.VOVNET.OUT_FEATURES) == ["stage3", "stage4", "stage5"] and cfg.MODEL.BACKBONE.FREEZE_AT == 3
    cfg.MODEL.VOVNET.CONV_BODY = base.MODEL.VOVNET.CONV_BODY
    assert cfg.dump() == base.dump()                                   # the body is the only difference


def test_bf16_frozen_storage_is_refused():
    bb = _backbone("V-19-slim-dw-eSE").bottom_up
    bb.frozen_storage = "bf16"
    with pytest.raises(ValueError, match="depthwise"):
        bb(torch.zeros(1, 3, 32, 32))


def test_flop_helper():
    """ore_dwpw_flops is host code of the library: 2 * M * C * (9 + C)."""
    import orehip
    L = orehip.lib()
    for M, C in ((1, 16), (160 * 160, 64), (2 * 40 * 40, 96), (20 * 20, 112), (3 * 7 * 5, 224), (1 << 33, 1024)):
        assert L.ore_dwpw_flops(M, C) == 2.0 * M * C * (9 + C)
    assert L.ore_dw3x3_wgrad_workspace_floats(2 * 40 * 40, 96) == 13 * 96 * 9       # parts of 256 pixels
    assert L.ore_dw3x3_wgrad_workspace_floats(256, 64) == 64 * 9 and L.ore_dw3x3_wgrad_workspace_floats(257, 64) == 2 * 64 * 9


def test_every_autograd_dw_call_is_listed():
    """The guarantee tests/test_trainops_host.py keeps for orehip/autograd.py, for the depthwise block's module: every orehip function it
    calls is listed with the test that holds it to float64, nothing listed is stale, and the three depthwise bindings are exercised by
    tests/test_hip_dw.py."""
    import re
    with open(os.path.join(PKG, "orehip", "autograd_dw.py")) as f:
        called = set(re.findall(r"\borehip\.(\w+)\(", f.read()))
    assert called == set(D.OSA_DW_CALLS), (sorted(called - set(D.OSA_DW_CALLS)), sorted(set(D.OSA_DW_CALLS) - called))
    root = os.path.dirname(PKG)
    for fn, why in D.OSA_DW_CALLS.items():
        files = re.findall(r"tests/\w+\.py", why)
        assert files and all(os.path.exists(os.path.join(root, p)) for p in files), (fn, why)
    with open(os.path.join(root, "tests", "test_hip_dw.py")) as f:
        gpu = f.read()
    for fn in ("dwpw", "dw3x3", "dw3x3_wgrad"):
        assert re.search(r"\boh\.%s\(" % fn, gpu), fn
    # orehip.autograd re-exports the block
    from orehip import autograd as A
    import orehip.autograd_dw as ADW
    assert A.OSADwFn is ADW.OSADwFn and A.osa_block_dw is ADW.osa_block_dw
