"""Record the depthwise VoVNet fixtures by EXECUTING the reference's vovnet.py / fpn.py through oracle/refrun/shims.py:

    python tools/gen_golden_vovnet_dw.py          # writes tests/golden/{backbone_fpn_dw_96x128,dw_units}.npz, vovnet_dw_state_keys.json

Runs only where the reference lies (oracle.refrun.shims.REF).  The fixtures are data: seeded inputs, the seed of
tests/vovnet_dw_ref.synth_state_dict_dw for the weights, the outputs the reference modules gave, and the names and shapes of their
state dicts.  No reference source text is stored.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle.refrun import shims  # noqa: E402
import vovnet_dw_ref as D  # noqa: E402
from conftest import chan_err, rel_err  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
SEED = 0                 # first seed tried
OWN_ERROR = 1e-4 / 4     # the reference's own fp32 error (against fp64) a fixture may have: a quarter of the tests' TOL
BODY = "V-19-slim-dw-eSE"


def np_(t):
    return t.detach().cpu().numpy()


def save(name, **arrays):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    print(f"{name}: {os.path.getsize(path) / 1024:.0f} KiB  " + ", ".join(f"{k}{tuple(v.shape)}" for k, v in arrays.items()))


def build(ns, body):
    return ns.vovnet.build_fcos_vovnet_fpn_backbone(shims.vovnet_cfg(body), ns.layers.ShapeSpec(channels=3))


def main():
    torch.manual_seed(SEED)
    torch.set_num_threads(8)
    ns = shims.setup()
    keys = {}
    for body in D.DW_SPECS:
        bb = build(ns, body)
        keys[body] = {k: list(v.shape) for k, v in bb.state_dict().items()}
        # FREEZE_AT 3 (shims.vovnet_cfg): what the reference leaves trainable in the bottom-up
        keys[body + "/trainable"] = sorted(n for n, p in bb.named_parameters() if p.requires_grad and n.startswith("bottom_up."))
    with open(os.path.join(OUT, "vovnet_dw_state_keys.json"), "w") as f:
        json.dump(keys, f, indent=0, sort_keys=True)
    print({k: len(v) for k, v in keys.items()})

    bb = build(ns, BODY)
    bb.eval()
    g = torch.Generator().manual_seed(1234)
    x = torch.randn(2, 3, 96, 128, generator=g) * 50.0
    x2 = torch.randn(1, 64, 24, 40, generator=g)
    x3 = torch.randn(1, 64, 25, 37, generator=g)
    x4 = torch.relu(torch.randn(1, 112, 21, 21, generator=g))
    x5 = torch.relu(torch.randn(1, 384, 10, 10, generator=g))

    def run(seed):
        sd = D.synth_state_dict_dw(seed, BODY)
        bb.load_state_dict({k[len("backbone."):]: v for k, v in sd.items() if k.startswith("backbone.")}, strict=True)
        st = bb.bottom_up.stem
        with torch.no_grad():
            o = bb(x)
            y2, y3 = x2, x3
            for i in range(3, 7):           # stem_2: dw, pw, norm, relu
                y2 = st[i](y2)
            for i in range(7, 11):          # stem_3: stride 2, odd size
                y3 = st[i](y3)
            got = dict(p3=o["p3"], p4=o["p4"], p5=o["p5"], stem2_y=y2, stem3_y=y3, stage3_y=bb.bottom_up.stage3(x4),
                       stage5_y=bb.bottom_up.stage5(x5))
            # the same in fp64 (tests/vovnet_dw_ref.py): what the reference's fp32 run is a rounding of
            sd64 = {k: v.double() for k, v in sd.items()}
            e = D.backbone_fpn_dw(x.double(), sd64)
            exact = dict(p3=e["p3"], p4=e["p4"], p5=e["p5"], stem2_y=D.dw_unit(x2.double(), sd64, D.P + "stem.stem_2", 1),
                         stem3_y=D.dw_unit(x3.double(), sd64, D.P + "stem.stem_3", 2), stage3_y=D.osa_stage_dw(x4.double(), sd64, 3),
                         stage5_y=D.osa_stage_dw(x5.double(), sd64, 5))
        own = max(max(rel_err(np_(got[k]), np_(exact[k])), chan_err(np_(got[k]), np_(exact[k]))) for k in got)
        return got, own

    # A fixture pins an fp32 implementation to TOL = 1e-4 (rel_err and chan_err) only if its OWN rounding error is well inside that:
    # with these weights the eSE pre-activations spread over +-100, so now and then a channel's gate lands on the foot of the
    # hard sigmoid, where relu6(z + 3) / 6 turns the absolute error of z into a relative error of 1e-4 .. 1e-3 of the whole channel --
    # in the reference's own fp32 run as in anyone's.  Such a draw measures the luck of a summation order, not an implementation.  So
    # the seed is the first whose reference run lies within TOL / 4 of the fp64 restatement.  The criterion looks at the executed
    # reference alone, never at the code under test.
    for seed in range(SEED, SEED + 64):
        got, own = run(seed)
        print(f"seed {seed}: the reference's fp32 run is within {own:.2e} of fp64")
        if own < OWN_ERROR:
            break
    else:
        raise SystemExit("no seed gives a well-conditioned fixture")
    save("backbone_fpn_dw_96x128", seed=np.int64(seed), x=np_(x), p3=np_(got["p3"]), p4=np_(got["p4"]), p5=np_(got["p5"]))
    save("dw_units", seed=np.int64(seed), stem2_x=np_(x2), stem2_y=np_(got["stem2_y"]), stem3_x=np_(x3), stem3_y=np_(got["stem3_y"]),
         stage3_x=np_(x4), stage3_y=np_(got["stage3_y"]), stage5_x=np_(x5), stage5_y=np_(got["stage5_y"]))


if __name__ == "__main__":
    main()
