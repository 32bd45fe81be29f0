#!/usr/bin/env python3
"""What the engine computes NOW, as one SHA-256 per named buffer: for a host-side refactor of csrc/ore_engine.hip or of the launchers
under it, which must not move a bit.

    ORE_LIB=libore_hip_parent.so python3 tools/engine_digest.py OUT.json      (ORE_LIB: a library under faster-orefsdet_amd/lib/, as tools/lib_ab.py)
    python3 tools/engine_digest.py --diff A.json B.json                       (lists what differs, exit 1 if anything does; needs no GPU)

Per case one eager pass of an engine built by the tests' own case builders, then the SHA-256 of every buffer ore_engine_buffer names for
that engine (the rows of the last pass, "name#b" for every image / class slot), and of the detection record where the case has a second
stage.  The cases are the smallest that reach every branch of run_backbone, run_heads and run_roi:

    V-19-slim-eSE fp32, 64x96 and 90x150, one image      the fused one-image path (gate + pool, gate-scaled lateral weights)
    V-19-slim-eSE fp32, 64x96, two images                eSE gate from the map, max-pool with a multiplier, plain laterals
    V-19-slim-eSE bf16 storage, 64x96, one image         every storage-tagged launcher in its bf16 form
    V-19-slim-dw-eSE, 64x96, one image and two           depthwise units and the reduction conv
    V-39-eSE, 64x96, one image / two images              identity blocks: ore_ese_gate_residual_fwd / ore_scale_residual_fwd
    N-way pass, K = 2, second stage                      class slots, the fan-out correlation, the merge
    three-stage cascade (one image; bf16 storage too)    cascade stages; split-K fc1 (the fixtures' fc width 128 gives 32 slices)
    three-stage cascade, fc1 cut to 112 rows             single-slab fc1 ("roi_h" is a known name only there)
    "profile"                                            V-19-slim fp32 640x640, eager with profiling: launches and both flop totals

Run the tool twice with ONE library first: a buffer that differs there (memory no launch of the pass writes) says nothing.  The
hashes are not golden values: later work may move bits on purpose."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "faster-orefsdet_amd"), ROOT):
    sys.path.insert(0, p)


def diff(a_path, b_path):
    with open(a_path) as f:
        a = json.load(f)
    with open(b_path) as f:
        b = json.load(f)
    bad = 0
    for case in sorted(set(a["cases"]) | set(b["cases"])):
        x, y = a["cases"].get(case, {}), b["cases"].get(case, {})
        names = [n for n in sorted(set(x) | set(y)) if x.get(n) != y.get(n)]
        print("%-40s %3d entries  %s" % (case, len(x), "equal" if not names else "DIFFER: " + " ".join(names)))
        bad += len(names)
    print("%s (%s) vs %s (%s): %d differing entries" % (a_path, a["lib"], b_path, b["lib"], bad))
    return 1 if bad else 0


if len(sys.argv) == 4 and sys.argv[1] == "--diff":
    sys.exit(diff(sys.argv[2], sys.argv[3]))

import torch  # noqa: E402

import orehip  # noqa: E402

if os.environ.get("ORE_LIB"):
    orehip.LIB_PATH = os.path.join(ROOT, "faster-orefsdet_amd", "lib", os.environ["ORE_LIB"])
import bf16_engine_ref as E  # noqa: E402
import test_hip_cascade as TC  # noqa: E402
import test_hip_nway as TN  # noqa: E402
from oracle import ref_model as R  # noqa: E402

PER_IMAGE = ("pre_boxes", "pre_scores", "pre_loc", "pre_level", "keep_idx", "counts", "out_boxes", "out_scores", "det_boxes", "det_scores",
             "det_src", "det_count", "final_boxes", "final_scores", "final_count", "final_classes")
ONCE = ("roi_h", "roi_raw_boxes", "roi_raw_scores", "roi_ok")


def sha(t):
    t = t.contiguous().cpu()
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    return hashlib.sha256(t.numpy().tobytes()).hexdigest()


def digest(e, B):
    """{name: sha256} of every buffer the engine knows after its last pass of B images (class slots)."""
    torch.cuda.synchronize()
    names = ["stem1", "stem2", "stem3"] + [f"{n}{k}" for k in (2, 3, 4, 5) for n in ("stage", "gate", "cat", "ycat", "icat", "red")]
    names += [f"icat{k}b" for k in (2, 3, 4, 5)] + [f"{n}{l}" for l in (3, 4, 5) for n in ("p", "attn", "lat", "pos", "tower", "head")]
    names += [f"{n}#{b}" for b in range(B) for n in PER_IMAGE] + list(ONCE)
    out = {}
    for n in names:
        try:
            out[n] = sha(e.buffer(n))
        except orehip.OreError:                                 # a name this engine does not have (ycat / icat / red, det_* without a second stage)
            pass
    return out


def body_engine(body, hw, max_batch, mode="fp32"):
    spec, dw = E.body_spec(body)
    prev = orehip.set_conv_precision(mode)
    try:
        e = orehip.Engine(stem=spec["stem"], conv=spec["conv"], out=spec["out"], layers=spec["layers"], blocks=spec["blocks"], depthwise=dw,
                          max_batch=max_batch, max_h=hw[0], max_w=hw[1])
    finally:
        orehip.set_conv_precision(prev)
    return e


def body_cases(cases):
    for body, H, W, mode in (("V-19-slim-eSE", 64, 96, "fp32"), ("V-19-slim-eSE", 90, 150, "fp32"), ("V-19-slim-eSE", 64, 96, "bf16s"),
                             ("V-19-slim-dw-eSE", 64, 96, "fp32"), ("V-39-eSE", 64, 96, "fp32")):
        sd, x = E.case_inputs(body, H, W)
        one_only = mode == "bf16s" or (H, W) != (64, 96)        # bf16 storage takes one image per pass
        e = body_engine(body, (H, W), 1 if one_only else 2, mode)
        try:
            e.load_state_dict(sd)
            e.set_support(R.synth_support(0))
            e.finalize()
            xd = x.cuda()
            e.eval_forward(xd[0].contiguous(), use_graph=False)
            put(cases, f"{body} {mode} {H}x{W} B=1", digest(e, 1))
            if not one_only:
                e.eval_forward_batch(xd, use_graph=False)
                put(cases, f"{body} {mode} {H}x{W} B=2", digest(e, 2))
        finally:
            e.close()


def record(rec):
    return {"record_boxes": sha(rec[0]), "record_scores": sha(rec[1]), "record_classes": sha(rec[2]), "record_rows": str(len(rec[1]))}


def second_stage_cases(cases):
    sd = R.synth_state_dict(0)
    roi_sd = R.synth_roi_state(sd, 0)
    roi_sd["roi_heads.box_head.0.fc1.weight"] = roi_sd["roi_heads.box_head.0.fc1.weight"] * 0.01    # as tests/test_hip_nway.py's roi_sd
    e = TN.nway_engine(orehip, sd, roi_sd, TN.supports(2), [11, 12])
    try:
        rec = e.detect_classes(R.synth_image(7, *TN.HW).cuda(), *TN.HW)
        put(cases, "N-way K=2 with the second stage", dict(digest(e, 2), **record(rec)))
    finally:
        e.close()
    sup = TC._supports(1)[0]
    for mode, fc in (("fp32", 128), ("bf16s", 128), ("fp32", 112)):
        sd3 = TC._sd3(0.01)
        for k in range(3 if fc != 128 else 0):                  # a narrower fc1 than the fixtures': not a multiple of 64, so one slab
            for n, rows in ((f"box_head.{k}.fc1.weight", True), (f"box_head.{k}.fc1.bias", True), (f"box_predictor.{k}.cls_score.weight", False),
                            (f"box_predictor.{k}.bbox_pred.weight", False)):
                t = sd3["roi_heads." + n]
                sd3["roi_heads." + n] = (t[:fc] if rows else t[:, :fc]).contiguous()
        prev = orehip.set_conv_precision(mode)
        try:
            e = TC._engine(orehip, sd3, sd3, sup, 3)
        finally:
            orehip.set_conv_precision(prev)
        try:
            img = R.synth_image(7, *TC.HW).cuda()
            e.eval_forward(img, use_graph=False)
            d = digest(e, 1)
            rec = e.detect(img, *TC.HW)
            split = "single-slab fc1" if "roi_h" in d else "split-K fc1"
            put(cases, f"three-stage cascade {mode}, fc width {fc}, {split}", dict(d, **record(rec)))
        finally:
            e.close()


def profile_case(cases):
    e = orehip.Engine(max_batch=1, max_h=640, max_w=640)
    try:
        e.load_state_dict(R.synth_state_dict(0))
        e.set_support(R.synth_support(0))
        e.finalize()
        e.set_profiling(True)
        e.eval_forward(R.synth_image(3, 640, 640).cuda(), use_graph=False)
        torch.cuda.synchronize()
        _, flops, launches = e.read_profile()
        put(cases, "profile V-19-slim fp32 640x640", {"launches": str(launches), "flops": repr(flops),
                                                      "flops_executed": repr(e.profile_executed_flops()), "last_flops": repr(e.last_flops())})
    finally:
        e.close()


def put(cases, name, entries):
    """Record one case and write the file as it stands: a case that raises later loses nothing of the ones before it."""
    cases[name] = entries
    rec = {"lib": os.path.basename(orehip.LIB_PATH), "ore_version": int(orehip.lib().ore_version()), "cases": cases}
    with open(sys.argv[1], "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


def main():
    out_path = sys.argv[1]
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    cases = {}
    body_cases(cases)
    second_stage_cases(cases)
    profile_case(cases)
    print("%d cases, %d entries, %s -> %s" % (len(cases), sum(len(c) for c in cases.values()), os.path.basename(orehip.LIB_PATH), out_path))


if __name__ == "__main__":
    main()
