"""Record the fixtures of the deep VoVNet bodies (V-39-eSE, V-57-eSE, V-99-eSE) by EXECUTING the reference's vovnet.py / fpn.py through
oracle/refrun/shims.py:

    python tools/gen_golden_vovnet_deep.py   # writes tests/golden/{backbone_fpn_v39_96x128,deep_units}.npz,
                                             #        tests/golden/{vovnet_deep_state_keys,deep_own_error}.json

Runs only where the reference lies (oracle.refrun.shims.REF).  The fixtures are data: seeded inputs, the seed of
oracle.ref_model.synth_state_dict for the weights, the outputs the reference modules gave, the names and shapes of their state dicts,
and the reference's own fp32 error against the fp64 restatement.  No reference source text is stored.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle.refrun import shims  # noqa: E402
from oracle import ref_model as R  # noqa: E402
from conftest import chan_err, rel_err  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
SEED = 0                 # first seed tried
OWN_ERROR = 1e-4 / 4     # the reference's own fp32 error (against fp64) a fixture may have: a quarter of the tests' TOL
BODIES = ("V-39-eSE", "V-57-eSE", "V-99-eSE")
P = "backbone.bottom_up."


def np_(t):
    return t.detach().cpu().numpy()


def err(a, b):
    return max(rel_err(np_(a), np_(b)), chan_err(np_(a), np_(b)))


def save(name, **arrays):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    print(f"{name}: {os.path.getsize(path) / 1024:.0f} KiB  " + ", ".join(f"{k}{tuple(np.shape(v))}" for k, v in arrays.items()))


def build(ns, body):
    return ns.vovnet.build_fcos_vovnet_fpn_backbone(shims.vovnet_cfg(body), ns.layers.ShapeSpec(channels=3)).eval()


def load(bb, sd):
    bb.load_state_dict({k[len("backbone."):]: v for k, v in sd.items() if k.startswith("backbone.")}, strict=True)


def stage_exact(x, sd64, body, k):
    """Stage k of the fp64 restatement on its own: the max-pool and the chain of OSA blocks (oracle.ref_model.osa_module)."""
    spec = R.VOVNET_SPECS[body]
    z = F.max_pool2d(x.double(), 3, 2, ceil_mode=True)
    for b in range(spec["blocks"][k - 2]):
        mod = f"OSA{k}_{b + 1}"
        z = R.osa_module(z, sd64, f"{P}stage{k}.{mod}.", mod, spec["layers"], identity=b > 0)
    return z


def main():
    torch.manual_seed(SEED)
    torch.set_num_threads(8)
    ns = shims.setup()
    bbs = {body: build(ns, body) for body in BODIES}
    keys = {body: {k: list(v.shape) for k, v in bb.state_dict().items()} for body, bb in bbs.items()}
    with open(os.path.join(OUT, "vovnet_deep_state_keys.json"), "w") as f:
        json.dump(keys, f, indent=0, sort_keys=True)
    print({k: len(v) for k, v in keys.items()})

    g = torch.Generator().manual_seed(1234)
    x = torch.randn(2, 3, 96, 128, generator=g) * 50.0
    x4 = torch.relu(torch.randn(1, 512, 13, 11, generator=g))
    x5 = torch.relu(torch.randn(1, 768, 7, 9, generator=g))

    def units(body, sd, sd64):
        """stage 4 and stage 5 alone through the executed reference, and how far its fp32 run lies from fp64"""
        bb = bbs[body]
        with torch.no_grad():
            got = dict(stage4_y=bb.bottom_up.stage4(x4), stage5_y=bb.bottom_up.stage5(x5))
            own = max(err(got["stage4_y"], stage_exact(x4, sd64, body, 4)), err(got["stage5_y"], stage_exact(x5, sd64, body, 5)))
        return got, own

    # V-39, the whole backbone.  A fixture pins an fp32 implementation to TOL = 1e-4 (rel_err and chan_err) only if its OWN rounding
    # error is well inside that (tools/gen_golden_vovnet_dw.py has the reasons: gates on the foot of the hard sigmoid, ReLU sign flips;
    # over the two-block stages they compound).  So the seed is the first whose reference run lies within TOL / 4 of the fp64
    # restatement.  The criterion looks at the executed reference alone, never at the code under test.
    body = "V-39-eSE"
    for seed in range(SEED, SEED + 64):
        sd = R.synth_state_dict(seed, body)
        sd64 = {k: v.double() for k, v in sd.items()}
        load(bbs[body], sd)
        with torch.no_grad():
            o = bbs[body](x)
            e = R.backbone_fpn(x.double(), sd64, body=body)
        own = max(err(o[k], e[k]) for k in ("p3", "p4", "p5"))
        print(f"{body} seed {seed}: the reference's fp32 run is within {own:.2e} of fp64")
        if own < OWN_ERROR:
            break
    else:
        raise SystemExit("no seed gives a well-conditioned fixture")
    save("backbone_fpn_v39_96x128", seed=np.int64(seed), x=np_(x), p3=np_(o["p3"]), p4=np_(o["p4"]), p5=np_(o["p5"]))
    got, own = units(body, sd, sd64)
    print(f"{body} seed {seed}: stage 4 / stage 5 alone within {own:.2e}")
    assert own < OWN_ERROR, own
    arrays = {"stage4_x": np_(x4), "stage5_x": np_(x5), "v39_seed": np.int64(seed), "v39_stage4_y": np_(got["stage4_y"]),
              "v39_stage5_y": np_(got["stage5_y"])}

    # V-57: the whole backbone is not conditioned well enough at any seed, one stage is: the first seed whose two units
    # lie within TOL / 4
    body = "V-57-eSE"
    for seed57 in range(SEED, SEED + 64):
        sd = R.synth_state_dict(seed57, body)
        load(bbs[body], sd)
        got, own = units(body, sd, {k: v.double() for k, v in sd.items()})
        print(f"{body} seed {seed57}: stage 4 / stage 5 alone within {own:.2e}")
        if own < OWN_ERROR:
            break
    else:
        raise SystemExit("no seed gives well-conditioned V-57 units")
    arrays.update({"v57_seed": np.int64(seed57), "v57_stage4_y": np_(got["stage4_y"]), "v57_stage5_y": np_(got["stage5_y"])})
    save("deep_units", **arrays)

    # The reference's own fp32 error, stage by stage, at the sizes the stage-wise engine test runs (a 64 x 96 image: stage k works at
    # 64 / 2^k x 96 / 2^k and reads the map of stage k - 1): every multi-block stage alone on a relu(randn) input of its width.  The
    # tolerance of that test hangs on these figures.
    own_rec = {}
    g2 = torch.Generator().manual_seed(4321)
    for body, s in (("V-57-eSE", seed57), ("V-99-eSE", SEED)):
        spec = R.VOVNET_SPECS[body]
        sd = R.synth_state_dict(s, body)
        sd64 = {k: v.double() for k, v in sd.items()}
        load(bbs[body], sd)
        rec = {"seed": int(s)}
        for k in (3, 4, 5):
            if spec["blocks"][k - 2] == 1:
                continue
            xin = torch.relu(torch.randn(1, spec["out"][k - 3], 64 >> (k - 1), 96 >> (k - 1), generator=g2))
            with torch.no_grad():
                rec[f"stage{k}"] = err(getattr(bbs[body].bottom_up, f"stage{k}")(xin), stage_exact(xin, sd64, body, k))
            print(f"{body} seed {s} stage {k} ({spec['blocks'][k - 2]} blocks): own error {rec[f'stage{k}']:.2e}")
        own_rec[body] = rec

    # The image of the stage-wise engine test.  The figures above are measured at unit-scale inputs, where the eSE pre-activations are
    # of order one and the gates sit on the slope of the hard sigmoid.  An image of the usual amplitude (pixel - mean of order 100)
    # drives them to order 100: most gates saturate, and the few that land on the slope carry the absolute error of a sum of terms
    # of order 100 -- there the reference's own fp32 stages lie 1e-4 .. 3e-2 from fp64 on their own inputs (V-99 stage 4, nine
    # blocks), whatever the implementation.  So that test feeds pixel - mean = N(0, 1) * IMAGE_STD, the scale the tolerance was
    # measured at, and of those images the first whose EXECUTED REFERENCE stages, each on the fp32 input the reference itself
    # produced, lie within TOL / 4 of fp64 with one image and with two.  The criterion looks at the reference alone.
    IMAGE_STD = 0.25
    picks = {}
    for body, s in (("V-39-eSE", seed), ("V-57-eSE", seed57), ("V-99-eSE", SEED)):
        sd = R.synth_state_dict(s, body)
        sd64 = {k: v.double() for k, v in sd.items()}
        load(bbs[body], sd)
        bu = bbs[body].bottom_up
        for xs in range(64):
            xi = torch.randn(2, 3, 64, 96, generator=torch.Generator().manual_seed(xs)) * IMAGE_STD
            worst = 0.0
            with torch.no_grad():
                for B in (1, 2):
                    prev = bu.stage2(bu.stem(xi[:B]))
                    for k in (3, 4, 5):
                        cur = getattr(bu, f"stage{k}")(prev)
                        worst = max(worst, err(cur, stage_exact(prev, sd64, body, k)))
                        prev = cur
            print(f"{body} weights {s}, image {xs}: the reference's stages on their own inputs within {worst:.2e}")
            if worst < OWN_ERROR:
                break
        else:
            raise SystemExit(f"no well-conditioned stage-wise image for {body}")
        picks[body] = {"weights_seed": int(s), "image_seed": xs, "image_std": IMAGE_STD, "own": worst}
    own_rec["stagewise_input"] = picks
    with open(os.path.join(OUT, "deep_own_error.json"), "w") as f:
        json.dump(own_rec, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
