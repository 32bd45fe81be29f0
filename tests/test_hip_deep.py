"""The deep VoVNet bodies (V-39-eSE, V-57-eSE, V-99-eSE) on the fused engine: the two kernels of csrc/ore_osa_residual.hip against
float64, the V-39 engine against the fixture recorded from the executed reference, every body stage by stage on the engine's own stage
inputs, the stage-output contract, the detector from configs/fsod/finetune_vovnet_v39.yaml end to end, and the refusals.

Why V-57 and V-99 are pinned stage by stage and not on the whole backbone: DESIGN.md 7 (the reference's own fp32 run is farther than
TOL / 4 from fp64 over that many blocks at every seed tried; one stage is well conditioned)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, PKG, chan_err, rel_err
from oracle import decode as odec
from oracle import ref_model as R

pytestmark = pytest.mark.gpu

NAN = float("nan")
TOL = 1e-4
V39 = "V-39-eSE"
P = "backbone.bottom_up."


@pytest.fixture(scope="module")
def oh():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import orehip
    orehip.lib()
    return orehip


def _engine(oh, body, sd, max_batch, hw, finalize=True):
    spec = R.VOVNET_SPECS[body]
    e = oh.Engine(stem=spec["stem"], conv=spec["conv"], out=spec["out"], layers=spec["layers"], blocks=spec["blocks"],
                  max_batch=max_batch, max_h=hw[0], max_w=hw[1])
    e.load_state_dict(sd)
    e.set_support(R.synth_support(0))
    if finalize:
        e.finalize()
    return e


# ---------------------------------------------------------------------------------------------------------------- 1. the two kernels
def _maps(g, rows, C, lds=(24, 40, 12), coffs=(8, 16, 4)):
    """y, x, out as channel slices of wider NaN-filled [rows, ld] buffers: (y, x, out) buffers, their offsets, and the fp32 values."""
    yv, xv = torch.relu(torch.randn(rows, C, generator=g)) * 3.0, torch.randn(rows, C, generator=g)
    bufs = []
    for v, extra, coff in ((yv, lds[0], coffs[0]), (xv, lds[1], coffs[1]), (None, lds[2], coffs[2])):
        b = torch.full((rows, C + extra), NAN, device="cuda")
        if v is not None:
            b[:, coff:coff + C] = v.cuda()
        bufs.append(b)
    return bufs, coffs, yv, xv


def _check_tail(out_buf, before, coff, C, yv, xv, gate, what):
    """|out - (y g + x)| <= 2^-22 (|y g| + |x|) with g the gate the launch used (two fp32 roundings at most), and nothing outside
    the slice written (bits: NaN stays NaN)."""
    got = out_buf[:, coff:coff + C].double().cpu()
    yg = yv.double() * gate.double().cpu()
    x = xv.double() if xv is not None else torch.zeros_like(yg)
    err, bound = (got - (yg + x)).abs(), 2.0 ** -22 * (yg.abs() + x.abs())
    assert not torch.isnan(got).any(), what
    assert bool((err <= bound).all()), (what, float((err - bound).max()))
    a, b = out_buf.clone(), before.clone()
    a[:, coff:coff + C] = 0
    b[:, coff:coff + C] = 0
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (what, "wrote outside its slice")


@pytest.mark.parametrize("P_", (1, 3))
@pytest.mark.parametrize("HW", (20, 143))
@pytest.mark.parametrize("C", (256, 1024))
def test_ese_gate_residual_vs_fp64(oh, C, HW, P_):
    g = torch.Generator().manual_seed(1000 * P_ + 10 * HW + C)
    (yb, xb, ob), (yc, xc, oc), yv, xv = _maps(g, HW, C)
    # the concat conv's column sums over P row ranges of y, as fp32 inputs; the gate's reference is fp64 arithmetic on THESE numbers
    edges = [HW * p // P_ for p in range(P_ + 1)]
    part = torch.stack([yv[edges[p]:edges[p + 1]].double().sum(0) for p in range(P_)]).float()
    fw, fb = torch.randn(C, C, generator=g) * (1.0 / C) ** 0.5, torch.randn(C, generator=g) * 0.5
    z = (part.double().sum(0) / HW) @ fw.double().t() + fb.double()
    gate_ref = (z + 3.0).clamp(0.0, 6.0) / 6.0
    before = ob.clone()
    gate = oh.ese_gate_residual(part.cuda(), fw.cuda(), fb.cuda(), yb, xb, ob, y_coff=yc, x_coff=xc, out_coff=oc)
    torch.cuda.synchronize()
    gerr = float((gate.double().cpu().view(-1) - gate_ref).abs().max())
    print(f"C {C} HW {HW} P {P_}: gate within {gerr:.2e} of fp64, gates in [{float(gate.min()):.3f}, {float(gate.max()):.3f}]")
    assert gerr < 1e-5
    _check_tail(ob, before, oc, C, yv, xv, gate.view(1, C), (C, HW, P_))
    # a second launch gives the same bits
    ob2 = before.clone()
    gate2 = oh.ese_gate_residual(part.cuda(), fw.cuda(), fb.cuda(), yb, xb, ob2, y_coff=yc, x_coff=xc, out_coff=oc)
    assert torch.equal(gate2, gate) and torch.equal(ob2.view(torch.int32), ob.view(torch.int32))
    # no identity (the tail of block 1 in front of an identity block): the plain product, one rounding, so exactly torch's
    ob3 = before.clone()
    gate3 = oh.ese_gate_residual(part.cuda(), fw.cuda(), fb.cuda(), yb, None, ob3, y_coff=yc, out_coff=oc)
    assert torch.equal(gate3, gate)
    _check_tail(ob3, before, oc, C, yv, None, gate.view(1, C), (C, HW, P_, "no identity"))
    assert torch.equal(ob3[:, oc:oc + C], yb[:, yc:yc + C] * gate.view(1, C))


@pytest.mark.parametrize("HW", (20, 143))
@pytest.mark.parametrize("C", (256, 1024))
def test_scale_residual_vs_fp64(oh, C, HW):
    B = 2
    g = torch.Generator().manual_seed(77 + 10 * HW + C)
    (yb, xb, ob), (yc, xc, oc), yv, xv = _maps(g, B * HW, C)
    gate = torch.rand(B, C, generator=g)                                   # a different gate per image
    grow = gate.repeat_interleave(HW, 0)
    yb, xb, ob = (t.view(B, HW, -1) for t in (yb, xb, ob))
    before = ob.clone()
    oh.scale_residual(yb, gate.cuda(), xb, ob, y_coff=yc, x_coff=xc, out_coff=oc)
    torch.cuda.synchronize()
    _check_tail(ob.view(B * HW, -1), before.view(B * HW, -1), oc, C, yv, xv, grow, (C, HW))
    ob2 = before.clone()
    oh.scale_residual(yb, gate.cuda(), xb, ob2, y_coff=yc, x_coff=xc, out_coff=oc)
    assert torch.equal(ob2.view(torch.int32), ob.view(torch.int32))
    ob3 = before.clone()
    oh.scale_residual(yb, gate.cuda(), None, ob3, y_coff=yc, out_coff=oc)
    _check_tail(ob3.view(B * HW, -1), before.view(B * HW, -1), oc, C, yv, None, grow, (C, HW, "no identity"))
    # the one-image form computes the same element: same gate, same maps, same bits
    part = yv[:HW].double().sum(0, keepdim=True).float()
    fw, fb = torch.randn(C, C, generator=g) * (1.0 / C) ** 0.5, torch.randn(C, generator=g) * 0.5
    o1 = before.view(B * HW, -1)[:HW].clone()
    g1 = oh.ese_gate_residual(part.cuda(), fw.cuda(), fb.cuda(), yb[0], xb[0], o1, y_coff=yc, x_coff=xc, out_coff=oc)
    o2 = before.view(B * HW, -1)[:HW].clone()
    oh.scale_residual(yb[:1], g1, xb[:1], o2.view(1, HW, -1), y_coff=yc, x_coff=xc, out_coff=oc)
    assert torch.equal(o1.view(torch.int32), o2.view(torch.int32))


def test_residual_kernels_refuse_bad_arguments(oh):
    """Every check comes before the launch: the output keeps its NaN fill."""
    C, HW = 64, 8
    L = oh.lib()
    y, x, out = (torch.full((HW, C + 16), NAN, device="cuda") for _ in range(3))
    y[:], x[:] = 1.0, 1.0
    gate, part = torch.ones(1, C, device="cuda"), torch.ones(1, C, device="cuda")
    fw, fb = torch.zeros(C, C, device="cuda"), torch.zeros(C, device="cuda")
    S = oh._stream()

    def tail(y_=y, yl=C + 16, yc=0, x_=x, xl=C + 16, xc=0, o_=out, ol=C + 16, oc=0, C_=C, o_off=0):
        return L.ore_scale_residual_fwd(y_.data_ptr(), yl, yc, gate.data_ptr(), x_.data_ptr(), xl, xc, 1, HW, C_, o_.data_ptr() + o_off, ol, oc, S)

    def fused(oc=0, C_=C, o_=out):
        return L.ore_ese_gate_residual_fwd(part.data_ptr(), 1, HW, C_, fw.data_ptr(), fb.data_ptr(), gate.data_ptr(), y.data_ptr(), C + 16, 0,
                                           x.data_ptr(), C + 16, 0, o_.data_ptr(), C + 16, oc, S)

    for what, rc in (("channels not a multiple of 4", tail(C_=C - 2)), ("offset not a multiple of 4", tail(oc=2)),
                     ("row stride not a multiple of 4", tail(ol=C + 18)), ("slice leaves its row", tail(oc=20)),
                     ("misaligned base", tail(o_off=4)), ("out is y", tail(o_=y)), ("out is x", tail(o_=x)),
                     ("fused: offset", fused(oc=2)), ("fused: slice leaves its row", fused(oc=20)), ("fused: channels", fused(C_=C - 2)),
                     ("fused: out is y", fused(o_=y))):
        assert rc != 0, what
        assert L.ore_last_error(), what
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    # side by side in the rows of ONE buffer is no overlap: x in channels [0, C), out in [C, 2C) of the same rows
    both = torch.full((HW, 2 * C), NAN, device="cuda")
    both[:, :C] = 2.0
    assert L.ore_scale_residual_fwd(y.data_ptr(), C + 16, 0, gate.data_ptr(), both.data_ptr(), 2 * C, 0, 1, HW, C, both.data_ptr(), 2 * C, C, S) == 0
    torch.cuda.synchronize()
    assert bool((both[:, C:] == 3.0).all())


# ---------------------------------------------------------------------------------------------------------------- 2. V-39 against the fixture
def _close(got, want, what):
    got = got.detach().cpu().numpy()
    assert tuple(got.shape) == tuple(want.shape), (what, got.shape, want.shape)
    r, c = rel_err(got, want), chan_err(got, want)
    print(f"{what}: rel_err {r:.2e} chan_err {c:.2e}")
    assert r < TOL and c < TOL, (what, r, c)


@pytest.fixture(scope="module")
def v39(oh, golden):
    fx = golden("backbone_fpn_v39_96x128")
    sd = R.synth_state_dict(int(fx["seed"]), V39)
    e = _engine(oh, V39, sd, 2, (96, 128))
    yield e, sd, fx
    e.close()


def test_v39_engine_reproduces_the_reference(oh, v39):
    e, sd, fx = v39
    assert e.blocks == (1, 1, 2, 2)
    x = (torch.from_numpy(fx["x"]) + torch.tensor(R.PIXEL_MEAN).view(1, 3, 1, 1)).contiguous().cuda()
    out = e.backbone(x)
    for k in ("p3", "p4", "p5"):
        _close(out[k], fx[k], "engine " + k)
    # every block's convolutions are counted: stem, then per block five 3x3 layers and the 1x1 concat conv, then the FPN
    spec = R.VOVNET_SPECS[V39]
    M = [2 * (96 >> s) * (128 >> s) for s in range(1, 6)]                  # rows at strides 2 .. 32
    want = 2.0 * M[0] * 27 * 64 + 2.0 * M[0] * 64 * 64 * 9 + 2.0 * M[1] * 64 * 128 * 9
    cin, L = 128, spec["layers"]
    for s, (c, o, nb) in enumerate(zip(spec["conv"], spec["out"], spec["blocks"])):
        m = M[s + 1]
        for b in range(nb):
            ci = cin if b == 0 else o
            want += 2.0 * m * 9 * (ci * c + (L - 1) * c * c) + 2.0 * m * (ci + L * c) * o
        cin = o
    for l, o in enumerate(spec["out"][1:]):
        want += 2.0 * M[l + 2] * o * 128 + 2.0 * M[l + 2] * 128 * 128 * 9
    assert e.last_flops() == want
    # one image through the whole pass: the graph replay equals the first call bit for bit
    img = x[1].contiguous()
    names = [f"head{l}" for l in (3, 4, 5)] + [f"p{l}" for l in (3, 4, 5)]
    e.eval_forward(img, use_graph=True)
    torch.cuda.synchronize()
    first = [e.buffer(n, (1, 96 >> int(n[-1]), 128 >> int(n[-1]))).clone() for n in names]
    e.eval_forward(img, use_graph=True)
    torch.cuda.synchronize()
    assert all(torch.equal(a, e.buffer(n, (1, 96 >> int(n[-1]), 128 >> int(n[-1])))) for a, n in zip(first, names))
    # and the one-image pass (fused column sums, one launch per identity block) agrees with that image of the batch of two
    for l, k in ((3, "p3"), (4, "p4"), (5, "p5")):
        _close(e.buffer(k, (1, 96 >> l, 128 >> l)), fx[k][1:2], "one image " + k)


# ---------------------------------------------------------------------------------------------------------------- 3. stage by stage
def _own_error():
    with open(os.path.join(GOLDEN, "deep_own_error.json")) as f:
        return json.load(f)


def _stage_out(e, k, B, h, w):
    """the stage-output contract: buffer "stageK" times buffer "gateK" """
    return e.buffer(f"stage{k}", (B, h, w)).double().cpu() * e.buffer(f"gate{k}").double().cpu().view(B, -1, 1, 1)


@pytest.mark.parametrize("body", (V39, "V-57-eSE", "V-99-eSE"))
def test_every_stage_on_the_engines_own_inputs(oh, golden, body):
    """Each stage k >= 3 against the oracle's fp64 max-pool + OSA chain applied to what the engine itself holds as stage k - 1's output:
    whatever the stages before accumulated, one stage's fp32 error apart.  Once with one image (the concat convs' fused column sums feed
    ore_ese_gate_residual_fwd) and once with a batch of two (ore_ese_gate_fwd + ore_scale_residual_fwd).

    Tolerance: max(TOL, 4 x the reference's own fp32 error of that stage) from deep_own_error.json, which was measured at unit-scale
    inputs; the image is at that scale too and was picked by the executed reference's own error alone ("stagewise_input" of the same
    file, tools/gen_golden_vovnet_deep.py has the reasons).  At the usual image amplitude the reference's own stages lie 1e-4 .. 3e-2
    from fp64 on their own inputs, and no fp32 implementation can be pinned there."""
    rec = _own_error()
    own, pick = rec.get(body, {}), rec["stagewise_input"][body]
    seed = pick["weights_seed"]
    assert seed == (own["seed"] if own else int(golden("backbone_fpn_v39_96x128")["seed"]))
    spec = R.VOVNET_SPECS[body]
    sd = R.synth_state_dict(seed, body)
    sd64 = {k: v.double() for k, v in sd.items() if k.startswith(P + "stage")}
    H, W = 64, 96
    x = torch.randn(2, 3, H, W, generator=torch.Generator().manual_seed(pick["image_seed"])) * pick["image_std"]
    x = (x + torch.tensor(R.PIXEL_MEAN).view(1, 3, 1, 1)).contiguous().cuda()
    e = _engine(oh, body, sd, 2, (H, W))
    try:
        for B in (1, 2):
            e.backbone(x[:B].contiguous())
            torch.cuda.synchronize()
            for k in (3, 4, 5):
                z = F.max_pool2d(_stage_out(e, k - 1, B, H >> (k - 1), W >> (k - 1)), 3, 2, ceil_mode=True)
                with torch.no_grad():
                    for b in range(spec["blocks"][k - 2]):
                        mod = f"OSA{k}_{b + 1}"
                        z = R.osa_module(z, sd64, f"{P}stage{k}.{mod}.", mod, spec["layers"], identity=b > 0)
                got = _stage_out(e, k, B, H >> k, W >> k).numpy()
                o = float(own.get(f"stage{k}", 0.0))
                tol = max(TOL, 4.0 * o)
                r, c = rel_err(got, z.numpy()), chan_err(got, z.numpy())
                print(f"{body} B {B} stage {k} ({spec['blocks'][k - 2]} blocks): rel_err {r:.2e} chan_err {c:.2e}; the reference's own {o:.2e}, tolerance {tol:.1e}")
                assert r < tol and c < tol, (body, B, k, r, c, tol)
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------------------- 4. the contract
def test_stage_output_contract(oh, v39):
    """A stage that ends in an identity block holds its whole output in "stageK" and ones in "gateK"; the one-block stages of the same
    engine keep their gate (folded into the max-pool and the lateral behind them)."""
    e, sd, fx = v39
    x = (torch.from_numpy(fx["x"]) + torch.tensor(R.PIXEL_MEAN).view(1, 3, 1, 1)).contiguous().cuda()
    for B in (2, 1):
        e.backbone(x[:B].contiguous())
        torch.cuda.synchronize()
        for k, nb in zip((2, 3, 4, 5), e.blocks):
            g = e.buffer(f"gate{k}")
            assert tuple(g.shape) == (B, R.VOVNET_SPECS[V39]["out"][k - 2])
            if nb > 1:
                assert bool((g == 1.0).all()), (B, k)
            else:
                assert 0.0 <= float(g.min()) and float(g.max()) <= 1.0 and float(g.max() - g.min()) > 0.1, (B, k, float(g.min()), float(g.max()))


# ---------------------------------------------------------------------------------------------------------------- 5. end to end
def _cfg(extra=()):
    from fewx.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(PKG, "configs", "fsod", "finetune_vovnet_v39.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", "cuda"] + list(extra))
    cfg.freeze()
    return cfg


def _detector():
    from detectron2.modeling import build_model
    cfg = _cfg(["INPUT.MAX_SIZE_TEST", 128, "INPUT.FS.SUPPORT_SHOT", 4])
    torch.manual_seed(0)
    m = build_model(cfg)
    sd = R.synth_roi_state(R.synth_state_dict(15, V39))
    sd["roi_heads.box_head.0.fc1.weight"] = sd["roi_heads.box_head.0.fc1.weight"] * 0.02
    sd["proposal_generator.centernet_head.agn_hm.bias"] = torch.full((1,), -2.0)
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and not missing, (missing, unexpected)
    return m.eval(), sd


def _support_dict(ids):
    d = {k: {} for k in ("p3", "p4", "p5", "rcnn_8", "rcnn_4")}
    for j, c in enumerate(ids):
        p = R.synth_support(10 + j)
        for k in ("p3", "p4", "p5"):
            d[k][c] = p[k]
        d["rcnn_8"][c] = torch.randn(6, 128, 8, 8, generator=torch.Generator().manual_seed(40 + j)) * 0.1
        d["rcnn_4"][c] = torch.zeros(6, 128, 4, 4)
    return d


def test_detector_inference(oh):
    from detectron2.structures import Instances
    m, sd = _detector()
    sup = _support_dict([7])
    m.set_support_dict(sup)
    H, W = 96, 128
    img = R.synth_image(9, H, W)
    req = {"image": img, "height": H, "width": W}
    a = m([req])[0]["instances"]
    assert isinstance(a, Instances) and len(a) > 0
    e = m._engine
    assert e.blocks == (1, 1, 2, 2)
    # the first stage of that pass against the oracle (the method of test_hip_parity.py::test_engine_eval_other_sizes_vs_oracle):
    # features and head rows at 1e-4, the detection tail bit-exact on the engine's own head outputs
    ref = R.eval_dense(img, sd, {k: sup[k][7] for k in ("p3", "p4", "p5")}, body=V39)
    hms, regs = [], []
    for l, k in enumerate(("p3", "p4", "p5")):
        hh, ww = H >> (l + 3), W >> (l + 3)
        assert rel_err(e.buffer(k, (1, hh, ww)).cpu().numpy(), ref["features"][k].numpy()) < TOL, k
        hd = e.buffer(f"head{l + 3}", (1, hh, ww)).cpu()
        assert rel_err(hd[:, :4].numpy(), ref["reg"][l].numpy()) < TOL and rel_err(hd[:, 4:5].numpy(), ref["hm"][l].numpy()) < TOL
        raw = e.buffer(f"head{l + 3}").cpu().numpy().reshape(hh, ww, 5)
        hms.append(np.ascontiguousarray(raw[..., 4]))
        regs.append(np.ascontiguousarray(raw[..., :4]))
    c = m._cfg_engine
    want = odec.decode_nms(hms, regs, tuple(c["strides"]), c["score_thresh"], c["pre_topk"], c["nms_thresh"], c["post_topk"])
    boxes, scores, keep = e.proposals()
    assert np.array_equal(keep.cpu().numpy(), want["keep"]) and np.array_equal(boxes.cpu().numpy(), want["boxes"])
    b = m.inference_many([req])[0]["instances"]
    assert torch.equal(a.pred_boxes.tensor, b.pred_boxes.tensor) and torch.equal(a.scores, b.scores)
    # N-way: every support class in one pass on the same (shared) deep backbone
    m.set_support_dict(_support_dict([3, 5]))
    m.support_classes = "all"
    n = m([req])[0]["instances"]
    assert len(n) > 0 and set(n.pred_classes.tolist()) == {3, 5}
    assert m._engine.blocks == (1, 1, 2, 2)


def _seed_weights(m, sd):
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and not missing, (missing, unexpected)
    m.set_support_dict(_support_dict([1]))
    return m.eval()


def test_default_predictor_and_trainer_test(oh, tmp_path, monkeypatch):
    """The two other entry points the yaml has to serve: DefaultPredictor(cfg)(bgr) equals the model's own raw-image request, and the
    entry script's Trainer.test runs the detector over a dataset into COCOEvaluator."""
    from detectron2.engine.defaults import DefaultPredictor
    from detectron2.evaluation import COCOEvaluator
    from test_entry_script import _load_script, _write_dataset
    _, sd = _detector()
    pred = DefaultPredictor(_cfg(["INPUT.MAX_SIZE_TEST", 128, "INPUT.MIN_SIZE_TEST", 96, "MODEL.WEIGHTS", ""]))
    _seed_weights(pred.model, sd)
    bgr = np.ascontiguousarray(R.synth_image(21, 120, 150).numpy().transpose(1, 2, 0))
    got = pred(bgr)["instances"]
    want = pred.model([{"image_raw": bgr}])[0]["instances"]
    assert len(got) > 0 and got.image_size == (120, 150)
    assert torch.equal(got.pred_boxes.tensor, want.pred_boxes.tensor) and torch.equal(got.scores, want.scores)
    assert pred.model._engine.blocks == (1, 1, 2, 2)
    # Trainer.test of the entry script on a written dataset
    monkeypatch.chdir(tmp_path)
    _write_dataset(str(tmp_path), n_img=3, per_img=2)
    m = _load_script()
    yaml = os.path.join(PKG, "configs", "fsod", "finetune_vovnet_v39.yaml")
    cfg = m.setup(m.default_argument_parser().parse_args(
        ["--config-file", yaml, "--num-gpus", "1", "OUTPUT_DIR", str(tmp_path / "out"), "MODEL.DEVICE", "cuda", "DATALOADER.NUM_WORKERS", "0",
         "INPUT.MAX_SIZE_TEST", "128", "INPUT.MIN_SIZE_TEST", "96", "MODEL.WEIGHTS", ""]))
    assert cfg.MODEL.VOVNET.CONV_BODY == V39
    name = cfg.DATASETS.TEST[0]
    ev = COCOEvaluator(name, output_dir=str(tmp_path / "eval"))
    res = m.Trainer.test(cfg, pred.model, evaluators=[ev])
    assert "bbox" in res and "AP" in res["bbox"]
    rows = json.load(open(os.path.join(str(tmp_path / "eval"), "coco_instances_results.json")))
    assert len(rows) > 0


# ---------------------------------------------------------------------------------------------------------------- 6. refusals
def test_refusals(oh):
    spec = R.VOVNET_SPECS[V39]
    kw = dict(stem=spec["stem"], conv=spec["conv"], out=spec["out"], layers=spec["layers"], max_h=64, max_w=96)
    prev = oh.set_conv_precision("bf16s")
    try:
        with pytest.raises(oh.OreError, match="bf16-storage"):
            oh.Engine(blocks=spec["blocks"], **kw)
    finally:
        oh.set_conv_precision(prev)
    with pytest.raises(oh.OreError, match="depthwise"):
        oh.Engine(stem=(64, 64, 64), conv=(64, 80, 96, 112), out=(112, 256, 384, 512), max_h=64, max_w=96, depthwise=True, blocks=(1, 1, 2, 2))
    for bad in ((1, 1, 0, 1), (1, 17, 1, 1), (1, 1, 2, -3)):
        with pytest.raises(oh.OreError, match="1 to 16"):
            oh.Engine(blocks=bad, **kw)
    # a state dict without the identity block of stage 4: finalize names the first tensor it misses
    sd = {k: v for k, v in R.synth_state_dict(0, V39).items() if "OSA4_2" not in k}
    e = _engine(oh, V39, sd, 1, (64, 96), finalize=False)
    with pytest.raises(oh.OreError, match=r"missing tensor 'backbone\.bottom_up\.stage4\.OSA4_2\.layers\.0\.OSA4_2_0/conv\.weight'"):
        e.finalize()
    e.close()
    # the module: bf16 storage on a deep body is refused before any engine exists
    m, _ = _detector()
    m.set_support_dict(_support_dict([7]))
    m.conv_operands = "bf16s"
    with pytest.raises(ValueError, match=r"V-39-eSE.*bf16s"):
        m.make_engine()
    assert m._engine is None
