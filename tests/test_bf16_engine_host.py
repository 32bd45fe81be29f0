"""tests/bf16_engine_ref.py (the float64 contract of every launch of an ORE_CONV_BF16 engine) against fp32 emulations written in torch: no
GPU.  Two things are shown for the contract functions tests/test_hip_bf16_engine.py uses:

  * a FAITHFUL fp32 emulation of every launch class -- MFMA conv, folded-input conv, weight-folded lateral, both chains, every exempt
    launch -- passes with rel_err and chan_err at most TOL_LAYER / 4, launch by launch through whole passes of the three bodies
    (`emulate` is an engine pass in torch: fp32 tensors, operands rounded to bf16 where the engine's launch rounds them, fp32 sums) and
    class by class on inputs of their own (an input fold with multiplier, addend and ReLU, which no engine launch of today takes);
  * each FAULTY emulation fails at least one check: the other lateral form, rounding before the fold instead of after it, an MFMA conv
    on unrounded operands, an exempt conv on rounded operands, a depthwise unit's pointwise on rounded operands, truncation instead of
    nearest-even, a gate applied twice (in the stored map and again in the lateral).

conv3 and the tower conv are MFMA convs of this mode (oracle/ref_model.py's definition; the engine launches them through the same
rounding conv entry as the backbone's): the "exempt conv on rounded operands" fault is therefore shown on the convs that ARE exempt in
an engine -- stem_1 and the grouped FPN output convs -- and conv3 on the other side: an unrounded conv3 fails.

Inputs: bf16_engine_ref.case_inputs at 64 x 96, the same weights and images the GPU module feeds (unit-scale noise around the pixel
mean at seed 0; V-39: the weights and image statistics tests/golden/deep_own_error.json picked for the stage-wise test).  Every chain reaches TOL_LAYER / 4 there: no bound is widened."""
import pytest
import torch
import torch.nn.functional as F

import bf16_engine_ref as E
from oracle import ref_model as R

P = E.P
QUARTER = E.TOL_LAYER / 4


def _rnd(t, faults=()):
    return E.trunc_bf16(t) if "truncate" in faults else t.bfloat16().float()


def _fold32(sd, name):
    sc = sd[name + ".weight"] * (1.0 / torch.sqrt(sd[name + ".running_var"] + 1e-5))
    return sc.view(1, -1, 1, 1), (sd[name + ".bias"] - sd[name + ".running_mean"] * sc).view(1, -1, 1, 1)


def _mconv(x, w, faults, stride=1, pad=0):
    if "mfma_unrounded" in faults:
        return F.conv2d(x, w, None, stride, pad)
    return F.conv2d(_rnd(x, faults), _rnd(w, faults), None, stride, pad)


def _conv_bn(x, sd, name, stride, pad, faults, exempt=False):
    sc, sh = _fold32(sd, name + "/norm")
    w = sd[name + "/conv.weight"]
    if exempt:
        y = F.conv2d(_rnd(x), _rnd(w), None, stride, pad) if "exempt_conv_rounded" in faults else F.conv2d(x, w, None, stride, pad)
    else:
        y = _mconv(x, w, faults, stride, pad)
    return F.relu(y * sc + sh)


def _unit(x, sd, name, stride, faults):
    sc, sh = _fold32(sd, name + "/pw_norm")
    t = F.conv2d(x, sd[name + "/dw_conv3x3.weight"], None, stride, 1, groups=x.shape[1])
    wp = sd[name + "/pw_conv1x1.weight"]
    y = F.conv2d(_rnd(t), _rnd(wp)) if "dw_pw_rounded" in faults else F.conv2d(t, wp)
    return F.relu(y * sc + sh)


def _gate32(y, fw, fb):
    return (F.relu6(F.conv2d(y.mean((2, 3), keepdim=True), fw, fb) + 3.0) / 6.0).flatten(1)


def emulate(body, sd, support, x_pre, faults=(), heads=True):
    """One engine pass in fp32 torch -> {buffer name: tensor} as tests/test_hip_bf16_engine.py reads them from the device."""
    spec, dw = E.body_spec(body)
    B, L = x_pre.shape[0], spec["layers"]
    S = {"stem1": _conv_bn(x_pre, sd, P + "stem.stem_1", 2, 1, faults, exempt=True)}
    if dw:
        S["stem2"] = _unit(S["stem1"], sd, P + "stem.stem_2", 1, faults)
        S["stem3"] = _unit(S["stem2"], sd, P + "stem.stem_3", 2, faults)
    else:
        S["stem2"] = _conv_bn(S["stem1"], sd, P + "stem.stem_2", 1, 1, faults)
        S["stem3"] = _conv_bn(S["stem2"], sd, P + "stem.stem_3", 2, 1, faults)
    x = S["stem3"]
    for k in (2, 3, 4, 5):
        cc, nblk = spec["conv"][k - 2], spec["blocks"][k - 2]
        if k > 2:
            x = F.max_pool2d(x, 3, 2, ceil_mode=True)

        def block(x, mod):
            pre = f"{P}stage{k}.{mod}."
            feats, y = [x], x
            rn = f"{pre}conv_reduction.{mod}_reduction_0"
            if dw and rn + "/conv.weight" in sd:
                y = S[f"red{k}"] = _conv_bn(x, sd, rn, 1, 0, faults)
            for i in range(L):
                nm = f"{pre}layers.{i}.{mod}_{i}"
                y = _unit(y, sd, nm, 1, faults) if dw else _conv_bn(y, sd, nm, 1, 1, faults)
                feats.append(y)
            cat = torch.cat(feats, 1)
            y = _conv_bn(cat, sd, f"{pre}concat.{mod}_concat", 1, 0, faults)
            return cat, y, _gate32(y, sd[pre + "ese.fc.weight"], sd[pre + "ese.fc.bias"])

        S[f"cat{k}"], y, g = block(x, f"OSA{k}_1")
        if nblk == 1:
            S[f"stage{k}"], S[f"gate{k}"] = y, g
            x = y * g.view(B, -1, 1, 1)
        else:
            x1 = y * g.view(B, -1, 1, 1)
            S[f"icat{k}"], y2, g2 = block(x1, f"OSA{k}_2")
            S[f"ycat{k}"] = y2
            x = S[f"stage{k}"] = y2 * g2.view(B, -1, 1, 1) + x1
            S[f"gate{k}"] = torch.ones_like(g2)
    prev = None
    for l in (5, 4, 3):
        xs, g = S[f"stage{l}"], S[f"gate{l}"].view(B, -1, 1, 1)
        w, b = sd[f"backbone.fpn_lateral{l}.weight"], sd[f"backbone.fpn_lateral{l}.bias"]
        one = (B == 1) != ("other_lateral" in faults)
        if "gate_twice" in faults:
            xs = xs * g                                      # the map was stored gated (for the pool), the lateral gates it again
        if spec["blocks"][l - 2] > 1:
            lat = _mconv(xs, w, faults)
        elif one:
            lat = torch.cat([_mconv(xs[i:i + 1], w * g[i].view(1, -1, 1, 1), faults) for i in range(B)])
        elif "round_before_fold" in faults:
            lat = F.conv2d(_rnd(_rnd(xs) * g), _rnd(w))
        else:
            lat = _mconv(xs * g, w, faults)
        lat = lat + b.view(1, -1, 1, 1)
        if prev is not None:
            lat = lat + F.interpolate(prev, scale_factor=2.0, mode="nearest")[:, :, :lat.shape[2], :lat.shape[3]]
        prev = S[f"lat{l}"] = lat
        wo, bo = sd[f"backbone.fpn_output{l}.weight"], sd[f"backbone.fpn_output{l}.bias"]
        S[f"p{l}"] = F.conv2d(_rnd(lat), _rnd(wo), bo, 1, 1) if "exempt_conv_rounded" in faults else F.conv2d(lat, wo, bo, 1, 1)
    hp = "proposal_generator.centernet_head."
    for l in (3, 4, 5) if heads else ():
        q = S[f"p{l}"]
        S[f"attn{l}"] = E.correlation(q, support[f"p{l}"]).float()
        S[f"pos{l}"] = F.relu(_mconv(torch.cat((S[f"attn{l}"], q), 1), sd["conv3.weight"], faults) + sd["conv3.bias"].view(1, -1, 1, 1))
        S[f"tower{l}"] = _mconv(S[f"pos{l}"], sd[hp + "bbox_tower.0.weight"], faults, 1, 1) + sd[hp + "bbox_tower.0.bias"].view(1, -1, 1, 1)
        t = F.relu(F.group_norm(S[f"tower{l}"], 32, sd[hp + "bbox_tower.1.weight"], sd[hp + "bbox_tower.1.bias"], eps=1e-5))
        rg = F.conv2d(t, sd[hp + "bbox_pred.weight"], sd[hp + "bbox_pred.bias"], padding=1) * sd[hp + f"scales.{l - 3}.scale"]
        S[f"head{l}"] = torch.cat((F.relu(rg), F.conv2d(t, sd[hp + "agn_hm.weight"], sd[hp + "agn_hm.bias"], padding=1)), 1)
    return S


_CASE = {}


def _case(body):
    if body not in _CASE:
        sd, x = E.case_inputs(body, 64, 96)
        _CASE[body] = (sd, R.synth_support(0), torch.cat([R.preprocess(x[i]) for i in range(2)]))
    return _CASE[body]


def _walk(body, B, faults=(), heads=True):
    sd, support, x_pre = _case(body)
    with torch.no_grad():
        S = emulate(body, sd, support, x_pre[:B], faults, heads)
        led = E.Ledger(f"{body} B={B} {sorted(faults)}")
        E.walk(body, sd, support, x_pre[:B], S, led, heads=heads)
    return led


@pytest.mark.parametrize("B", (1, 2))
@pytest.mark.parametrize("body", ("V-19-slim-eSE", "V-19-slim-dw-eSE", "V-39-eSE"))
def test_faithful_emulation_passes_every_launch_at_a_quarter_of_the_tolerance(body, B):
    led = _walk(body, B)
    led.assert_clean()
    classes = {r["cls"] for r in led.rows}
    want = {"mfma", "exempt", "fold-w" if B == 1 else "fold-in"} | ({"chain"} if body != "V-19-slim-eSE" else set())
    assert want <= classes, (want, classes)
    worst = max(led.rows, key=lambda r: max(r["rel"], r["chan"]))
    print(f"{body} B {B}: {len(led.rows)} launches, worst {worst['launch']} rel_err {worst['rel']:.2e} chan_err {worst['chan']:.2e}; "
          f"nearest unrounded twin {min(r['twin'] for r in led.rows if r['cls'] != 'exempt'):.2e}")
    over = [(r["launch"], r["rel"], r["chan"]) for r in led.rows if not (r["rel"] <= QUARTER and r["chan"] <= QUARTER)]
    assert not over, over


@pytest.mark.parametrize("fault,body,B,heads,where", [
    ("other_lateral", "V-19-slim-eSE", 1, False, "lateral"),              # the batched form in a one-image pass
    ("other_lateral", "V-19-slim-eSE", 2, False, "lateral"),              # ... and the reverse
    ("round_before_fold", "V-19-slim-eSE", 2, False, "lateral"),
    ("mfma_unrounded", "V-19-slim-eSE", 1, True, "conv3"),                # (every MFMA conv fails; conv3 is named: it is one of them)
    ("mfma_unrounded", "V-39-eSE", 1, False, "concat+tail"),              # the chain notices an unrounded first link
    ("mfma_unrounded", "V-19-slim-dw-eSE", 1, False, "reduction+unit0"),
    ("exempt_conv_rounded", "V-19-slim-eSE", 1, False, "output"),
    ("exempt_conv_rounded", "V-19-slim-eSE", 1, False, "stem_1"),
    ("dw_pw_rounded", "V-19-slim-dw-eSE", 1, False, "unit"),
    ("truncate", "V-19-slim-eSE", 1, False, "layer"),
    ("gate_twice", "V-19-slim-eSE", 1, False, "lateral"),
    ("gate_twice", "V-19-slim-eSE", 2, False, "lateral"),
])
def test_faulty_emulation_fails(fault, body, B, heads, where):
    led = _walk(body, B, {fault}, heads)
    hits = [f for f in led.failed if where in f]
    print("\n".join(led.failed[:6]))
    assert hits, (fault, where, led.failed)
    with pytest.raises(AssertionError):
        led.assert_clean()


def test_launch_classes_on_inputs_of_their_own():
    """The classes the engine walks only in one form: an input fold with multiplier, addend and ReLU (the GroupNorm fold of a conv
    launch), stride 2, the top-down add on an odd map -- faithful at a quarter of the tolerance, and the faults of each."""
    g = torch.Generator().manual_seed(7)
    B, C, Co, H, W = 2, 96, 48, 9, 11
    x = torch.randn(B, C, H, W, generator=g)
    w = torch.randn(Co, C, 3, 3, generator=g) / (9 * C) ** 0.5
    mul, add = torch.rand(B, C, generator=g) + 0.5, torch.randn(B, C, generator=g) * 0.2
    bias = torch.randn(Co, generator=g) * 0.1
    want = E.conv_fold_in(x, w, mul=mul, add_in=add, relu_in=True, shift=bias, pad=1)
    xin = F.relu(x * mul.view(B, C, 1, 1) + add.view(B, C, 1, 1))
    good = F.conv2d(_rnd(xin), _rnd(w), bias, 1, 1)
    assert max(E.errs(good, want)) <= QUARTER
    before = F.conv2d(_rnd(F.relu(_rnd(x) * mul.view(B, C, 1, 1) + add.view(B, C, 1, 1))), _rnd(w), bias, 1, 1)     # rounded before the affine
    assert E.errs(before, want)[0] > E.TOL_LAYER
    assert E.errs(F.conv2d(xin, w, bias, 1, 1), want)[0] > E.TOL_LAYER                                               # unrounded
    assert E.errs(F.conv2d(E.trunc_bf16(xin), E.trunc_bf16(w), bias, 1, 1), want)[0] > E.TOL_LAYER                  # truncated
    # stride 2 + FrozenBN + ReLU (stem_3's form)
    sc, sh = torch.rand(Co, generator=g) + 0.5, torch.randn(Co, generator=g) * 0.1
    want = E.conv(x, w, scale=sc, shift=sh, stride=2, pad=1, relu=True)
    good = F.relu(F.conv2d(_rnd(x), _rnd(w), None, 2, 1) * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))
    assert max(E.errs(good, want)) <= QUARTER
    # the two laterals with the top-down add onto an odd map (9 x 11 under 5 x 6), K = 1024
    K = 1024
    xs = F.relu(torch.randn(1, K, H, W, generator=g))
    gt = torch.rand(1, K, generator=g)
    wl = torch.randn(Co, K, 1, 1, generator=g) / K ** 0.5
    top = torch.randn(1, Co, 5, 6, generator=g)
    up = F.interpolate(top, scale_factor=2.0, mode="nearest")[:, :, :H, :W]
    one = F.conv2d(_rnd(xs), _rnd(wl * gt.view(1, K, 1, 1)), bias) + up
    bat = F.conv2d(_rnd(xs * gt.view(1, K, 1, 1)), _rnd(wl), bias) + up
    assert max(E.errs(one, E.lateral_one(xs, gt, wl, bias, top))) <= QUARTER
    assert max(E.errs(bat, E.lateral_batch(xs, gt, wl, bias, top))) <= QUARTER
    assert E.errs(one, E.lateral_batch(xs, gt, wl, bias, top))[0] > E.LATERAL_APART
    assert E.errs(bat, E.lateral_one(xs, gt, wl, bias, top))[0] > E.LATERAL_APART


def test_oracle_states_both_lateral_forms_and_the_depthwise_body():
    """oracle/ref_model.py's whole-network statement of an engine pass agrees with the launch contracts: the one-image form folds the
    gate into the lateral's weight, the batched form into its input, the FPN output convs are fp32 in both; tests/vovnet_dw_ref.py's
    statement of the mode keeps the units fp32 and rounds the reduction / concat convs."""
    sd, support, x_pre = _case("V-19-slim-eSE")
    with torch.no_grad():
        S = emulate("V-19-slim-eSE", sd, support, x_pre[:1], heads=False)
        for ps, other in (("one", "batch"), ("batch", "one")):
            with R.operand_precision("bf16", engine_pass=ps):
                feats = {f"stage{k}": R.ese(S[f"stage{k}"], sd, f"{P}stage{k}.OSA{k}_1.ese.") for k in (3, 4, 5)}
                got = R.fpn(feats, sd)
            lat = {}
            for l in (5, 4, 3):
                x, gt = S[f"stage{l}"], E.gate(S[f"stage{l}"], sd[f"{P}stage{l}.OSA{l}_1.ese.fc.weight"], sd[f"{P}stage{l}.OSA{l}_1.ese.fc.bias"]).float()
                form = E.lateral_one if ps == "one" else E.lateral_batch
                lat[l] = form(x, gt, sd[f"backbone.fpn_lateral{l}.weight"], sd[f"backbone.fpn_lateral{l}.bias"], lat.get(l + 1)).float()
                want = E.conv(lat[l], sd[f"backbone.fpn_output{l}.weight"], shift=sd[f"backbone.fpn_output{l}.bias"], pad=1, rounded=False)
                assert max(E.errs(got[f"p{l}"], want)) < E.TOL_LAYER, (ps, l)
        with R.operand_precision("bf16"):                                  # the kernels' statement: batched lateral, rounded output conv
            feats = {f"stage{k}": R.ese(S[f"stage{k}"], sd, f"{P}stage{k}.OSA{k}_1.ese.") for k in (3, 4, 5)}
            assert not hasattr(feats["stage5"], "_ore_gated")
            p5 = R.fpn(feats, sd)["p5"]
        assert E.errs(p5, E.conv(lat[5], sd["backbone.fpn_output5.weight"], shift=sd["backbone.fpn_output5.bias"], pad=1, rounded=False))[0] > E.TOL_LAYER
        import vovnet_dw_ref as DW
        sdw, _, xw = _case("V-19-slim-dw-eSE")
        Sw = emulate("V-19-slim-dw-eSE", sdw, support, xw[:1], heads=False)
        pre = f"{P}stage3.OSA3_1."
        x3 = Sw["cat3"][:, :112]
        with DW.operand_precision("bf16"):
            red = DW.conv_bn_relu(x3, sdw, pre + "conv_reduction.OSA3_1_reduction_0", 1, 0)
            u0 = DW.dw_unit(Sw["red3"], sdw, pre + "layers.0.OSA3_1_0", 1)
            cc = DW.conv_bn_relu(Sw["cat3"], sdw, pre + "concat.OSA3_1_concat", 1, 0)
            s1 = DW.conv_bn_relu(xw[:1], sdw, P + "stem.stem_1", 2, 1)
        assert max(E.errs(red, E.conv_bn(x3, sdw, pre + "conv_reduction.OSA3_1_reduction_0", 1, 0))) <= QUARTER
        assert max(E.errs(cc, E.conv_bn(Sw["cat3"], sdw, pre + "concat.OSA3_1_concat", 1, 0))) <= QUARTER
        assert max(E.errs(u0, E.dw_unit(Sw["red3"], sdw, pre + "layers.0.OSA3_1_0", 1))) <= QUARTER
        assert E.errs(u0, E.dw_unit_pw_rounded(Sw["red3"], sdw, pre + "layers.0.OSA3_1_0", 1))[0] > E.TOL_LAYER
        assert max(E.errs(s1, E.stem1(xw[:1], sdw))) <= QUARTER
        with DW.operand_precision("bf16", engine_pass="one"):            # the whole backbone runs in the mode, both engine forms
            one = DW.backbone_fpn_dw(xw[:1], sdw)
        with DW.operand_precision("bf16", engine_pass="batch"):
            bat = DW.backbone_fpn_dw(xw[:1], sdw)
        fp32 = DW.backbone_fpn_dw(xw[:1], sdw)
        for k in ("p3", "p4", "p5"):
            assert E.errs(one[k], fp32[k])[0] > E.TOL_LAYER and E.errs(one[k], bat[k])[0] > E.TOL_LAYER, k
