"""An ORE_CONV_BF16 engine (fp32 tensors, both MFMA operands rounded to bf16 as they enter a conv), launch by launch on the engine's own
buffers: every launch's output against tests/bf16_engine_ref.py's float64 contract applied to what the engine itself holds as that
launch's input, at TOL_LAYER = 1e-4 in rel_err and chan_err.  Whatever the layers before accumulated, one launch's fp32 summation error
apart -- where tests/test_hip_bf16.py::test_engine_bf16_vs_oracle_bf16 can only bound two decorrelated bf16 networks at 2.5e-2, which
an orchestration fault of a few 1e-3 (a rounding on the wrong side of a fold, an exempt launch that rounds, an MFMA conv that does
not) passes.

Which launch is of which class (bf16_engine_ref.py lists the classes):
  mfma     stem_2, stem_3, every OSA layer and concat conv, a depthwise stage's reduction conv, the lateral of a stage that ends in an
           identity block, conv3, the tower conv.  Each must also lie more than 1e-4 from its unrounded twin.
  fold-w   the lateral of a one-block stage in a ONE-image pass: conv(round(x), round(fp32(g * W))), the gate-scaled weight written by
           the gate kernel.  Must fail the batched form by more than 1e-3.
  fold-in  the same lateral in a batched pass: conv(round(fp32(x * g)), round(W)).  Must fail the one-image form by more than 1e-3.
  exempt   stem_1, the max-pools (gated), the eSE gates, the depthwise units, the identity-block tail, the three FPN output convs (ONE
           per-level Winograd launch, which multiplies in fp32 in this mode: include/ore_hip.h), the correlation, GroupNorm + ReLU +
           the head's last conv (one fp32 VALU kernel).
  chain    block 1's concat conv of a two-block stage + its eSE tail (the conv's output map is reused by block 2; read from block 2's
           identity slice), and a depthwise stage's reduction conv + unit 0 (the reduction map is also held directly, "redK").

Bodies: V-19-slim-eSE, V-19-slim-dw-eSE, V-39-eSE; per body one image eagerly, the same image twice through the captured graph (every
checked buffer bit-equal to the eager pass) and a batch of two (ore_ese_gate_fwd, the gate as the conv's input multiplier), at 64 x 96,
the default body also at 90 x 150 (padded to 96 x 160: p5 is 3 x 5).  The kernels' shapes are pinned elsewhere; this module is about
which operand meets which rounding.  V-57 and V-99 overwrite their ping-pong buffers several times per stage and are NOT walked here:
in this mode they remain unpinned at launch level.

The worst rel_err / chan_err per (body, pass, launch) is printed at module teardown and appended to the file named by ORE_BF16E_LOG
(profiles/bf16_engine_ratios.txt is that file from the MI355X)."""
import os

import pytest
import torch

import bf16_engine_ref as E
from oracle import ref_model as R

pytestmark = pytest.mark.gpu

_WORST = {}


@pytest.fixture(scope="module")
def oh():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import orehip
    orehip.lib()
    return orehip


@pytest.fixture(scope="module", autouse=True)
def report(oh):
    yield
    lines = [f"{body:17s} {ps:6s} {launch:22s} {cls:8s} rel_err {r:.2e}  chan_err {c:.2e}"
             + ("" if t is None else f"  from its {'ROUNDED' if cls == 'exempt' else 'unrounded'} form {t:.2e}")
             + ("" if o is None else f"  from the other lateral form {o:.2e}")
             for (body, ps, launch), (cls, r, c, t, o) in sorted(_WORST.items())]
    for body in sorted({k[0] for k in _WORST}):
        for ps in sorted({k[1] for k in _WORST if k[0] == body}):
            v = [x for k, x in _WORST.items() if k[0] == body and k[1] == ps]
            tw = [x[3] for x in v if x[0] in ("mfma", "fold-w", "fold-in", "chain")]
            lines.append(f"{body:17s} {ps:6s} worst against the float64 contract: rel_err {max(x[1] for x in v):.2e} chan_err {max(x[2] for x in v):.2e};"
                         f" smallest distance of a rounded launch from its unrounded twin {min(tw):.2e} ({len(v)} launches)")
    print("\n" + "\n".join(lines))
    log = os.environ.get("ORE_BF16E_LOG")
    if log and lines:
        with open(log, "a") as f:
            f.write("\n".join(lines) + "\n")


def _note(body, ps, led):
    for row in led.rows:
        key = (body, ps, row["launch"])
        cls, r, c, t, o = _WORST.get(key, (row["cls"], 0.0, 0.0, None, None))
        t = row["twin"] if t is None else t if row["twin"] is None else min(t, row["twin"])
        o = row["other"] if o is None else o if row["other"] is None else min(o, row["other"])
        _WORST[key] = (row["cls"], max(r, row["rel"]), max(c, row["chan"]), t, o)


def _engine(oh, body, sd, hw):
    spec, dw = E.body_spec(body)
    prev = oh.set_conv_precision("bf16")
    try:
        e = oh.Engine(stem=spec["stem"], conv=spec["conv"], out=spec["out"], layers=spec["layers"], blocks=spec["blocks"], depthwise=dw,
                      max_batch=2, max_h=hw[0], max_w=hw[1])
    finally:
        oh.set_conv_precision(prev)
    assert oh.get_conv_precision() == "fp32"
    e.load_state_dict(sd)
    e.set_support(R.synth_support(0))
    e.finalize()
    return e


def _snapshot(e, body, B, hw):
    torch.cuda.synchronize()
    S = {}
    for name, k in E.buffer_names(body).items():
        S[name] = (e.buffer(name) if k is None else e.buffer(name, (B,) + hw[k])).float().cpu().clone()
    return S


@pytest.mark.parametrize("body,H,W", [("V-19-slim-eSE", 64, 96), ("V-19-slim-eSE", 90, 150), ("V-19-slim-dw-eSE", 64, 96), ("V-39-eSE", 64, 96)])
def test_every_launch_on_the_engines_own_inputs(oh, body, H, W):
    sd, x = E.case_inputs(body, H, W)
    support = R.synth_support(0)
    x_pre = torch.cat([R.preprocess(x[i]) for i in range(2)])
    hw = E.geometry(H, W)
    e = _engine(oh, body, sd, (H, W))
    try:
        xd = x.cuda()
        e.eval_forward(xd[0].contiguous(), use_graph=False)
        one = _snapshot(e, body, 1, hw)
        for _ in range(2):                                       # capture, then replay: the same bits in every checked buffer
            e.eval_forward(xd[0].contiguous(), use_graph=True)
            again = _snapshot(e, body, 1, hw)
            diff = [n for n in one if not torch.equal(one[n].view(torch.int32), again[n].view(torch.int32))]
            assert not diff, ("graph pass differs from the eager pass", diff)
        e.eval_forward_batch(xd, use_graph=False)
        two = _snapshot(e, body, 2, hw)
    finally:
        e.close()
    leds = []
    for ps, S, xp in (("one", one, x_pre[:1]), ("batch", two, x_pre)):
        led = E.Ledger(f"{body} {H}x{W} {ps}")
        E.walk(body, sd, support, xp, S, led)
        _note(body, ps, led)
        leds.append(led)
    for led in leds:
        for row in led.rows:
            print(f"{led.tag} {row['launch']} [{row['cls']}] rel_err {row['rel']:.2e} chan_err {row['chan']:.2e} twin {row['twin']} other {row['other']}")
    failed = [f for led in leds for f in led.failed]
    assert not failed, "\n".join(failed)
