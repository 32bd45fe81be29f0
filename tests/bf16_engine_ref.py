"""The contract of every launch of an ORE_CONV_BF16 engine (include/ore_hip.h: fp32 tensors, both MFMA operands rounded to bf16 as they
enter a conv), in float64, on that launch's OWN input buffers.  tests/test_hip_bf16_engine.py applies it to what an engine holds after
a pass, tests/test_bf16_engine_host.py to fp32 emulations written in torch (faithful ones and faulty ones).

Launch classes
  mfma      a conv on the matrix cores: both operands rounded to bf16 (nearest even) by the contract, products and sums in float64,
            FrozenBN / bias / ReLU / the top-down add in float64 behind it.  Must ALSO lie more than TOL_LAYER from the same conv on
            unrounded operands (`twin`), so that it really is the reduced path.
  fold-in   an mfma conv whose input is relu(x * mul + add) or x * gate: the fold is computed in fp32, THEN rounded.
  fold-w    the one-image FPN lateral: conv(round(x), round(fp32(g * W))).
  exempt    fp32 launches, operands not rounded: stem_1, max-pool, the eSE gates, the depthwise units, the identity-block tails, the
            grouped FPN output convs (one per-level Winograd launch, fp32 in this mode), the correlation, GroupNorm + the head's last
            conv.  Held to TOL_LAYER against the unrounded contract, which already excludes a rounded operand.
  chain     a launch whose output is overwritten within the pass, held together with the fp32 launch behind it, no rounding between
            the links: the concat conv of block 1 of a two-block stage + its eSE tail; a depthwise stage's reduction conv + unit 0.

All tensors are NCHW; `got` buffers are fp32 torch tensors read from the engine, weights come from the state dict the engine loaded."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from conftest import chan_err, rel_err

TOL_LAYER = 1e-4        # one launch on its own inputs: fp32 summation order against float64 (tests/test_hip_bf16.py)
LATERAL_APART = 1e-3    # the two lateral forms must be told apart by at least this much (they lie 3e-3 .. 6e-3 apart)
P = "backbone.bottom_up."
D = torch.float64


def rb(t):
    """fp32 -> bf16 (nearest even) -> float64: an operand as the MFMA sees it."""
    assert t.dtype == torch.float32
    return t.bfloat16().double()


def trunc_bf16(t):
    """fp32 -> bf16 by TRUNCATION (what the mode must not do): the fault model of the host test."""
    return (t.contiguous().view(torch.int32) & -65536).view(torch.float32)


# ------------------------------------------------------------------------------------------------------------ the contracts
def bn_fold(sd, name, eps=1e-5):
    sc = sd[name + ".weight"].double() / torch.sqrt(sd[name + ".running_var"].double() + eps)
    return sc, sd[name + ".bias"].double() - sd[name + ".running_mean"].double() * sc


def _epilogue(y, scale, shift, relu, add):
    if scale is not None:
        y = y * scale.to(D).view(1, -1, 1, 1)
    if shift is not None:
        y = y + shift.to(D).view(1, -1, 1, 1)
    if add is not None:
        y = y + add.to(D)
    return F.relu(y) if relu else y


def conv(x, w, *, scale=None, shift=None, stride=1, pad=0, relu=False, add=None, rounded=True):
    """mfma (rounded=True) or its unrounded twin / an exempt conv (rounded=False).  x, w fp32 (or float64 inside a chain, then they
    are used as they are: no rounding between the links of a chain applies to its SECOND link only)."""
    xo, wo = (rb(x), rb(w)) if rounded else (x.to(D), w.to(D))
    return _epilogue(F.conv2d(xo, wo, None, stride, pad), scale, shift, relu, add)


def fold_input(x, mul=None, add_in=None, relu_in=False):
    """The input fold as the kernel stages it: fp32 arithmetic on fp32 tensors (mul, add_in: [B, C])."""
    assert x.dtype == torch.float32
    if mul is not None:
        x = x * mul.float().view(mul.shape[0], -1, 1, 1)
    if add_in is not None:
        x = x + add_in.float().view(add_in.shape[0], -1, 1, 1)
    return F.relu(x) if relu_in else x


def conv_fold_in(x, w, *, mul=None, add_in=None, relu_in=False, **kw):
    return conv(fold_input(x, mul, add_in, relu_in), w, **kw)


def upsample2(top, h, w):
    return F.interpolate(top.to(D), scale_factor=2.0, mode="nearest")[:, :, :h, :w]


def lateral_one(x, g, w, bias, top=None):
    """One image per pass: the gate folded into the weight, conv(round(x), round(fp32(g * W)))."""
    assert x.shape[0] == 1
    wg = w * g.float().view(1, -1, 1, 1)                                     # fp32 product, as the gate kernel writes it
    return conv(x, wg, shift=bias, add=None if top is None else upsample2(top, *x.shape[2:]))


def lateral_batch(x, g, w, bias, top=None):
    """More than one image: the gate as the conv's input multiplier, conv(round(fp32(x * g)), round(W))."""
    return conv_fold_in(x, w, mul=g, shift=bias, add=None if top is None else upsample2(top, *x.shape[2:]))


def gate(y, fw, fb):
    """eSE gate relu6(fc(mean(y)) + 3) / 6 -> [B, C] (float64; y of any float dtype)."""
    z = F.conv2d(y.to(D).mean((2, 3), keepdim=True), fw.to(D), fb.to(D))
    return ((z + 3.0).clamp(0.0, 6.0) / 6.0).flatten(1)


def gated(y, g):
    return y.to(D) * g.to(D).view(g.shape[0], -1, 1, 1)


def pool(x):
    return F.max_pool2d(x.to(D), 3, 2, ceil_mode=True)


def tail(y, g, idn=None):
    """The identity-block tail y * g + x."""
    out = gated(y, g)
    return out if idn is None else out + idn.to(D)


def dw_unit(x, sd, name, stride):
    """A depthwise-separable unit, fp32 whatever the mode: dw 3x3 -> pw 1x1 -> FrozenBN -> ReLU, nothing rounded."""
    sc, sh = bn_fold(sd, name + "/pw_norm")
    t = F.conv2d(x.to(D), sd[name + "/dw_conv3x3.weight"].double(), None, stride, 1, groups=x.shape[1])
    return _epilogue(F.conv2d(t, sd[name + "/pw_conv1x1.weight"].double()), sc, sh, True, None)


def dw_unit_pw_rounded(x, sd, name, stride):
    """The same unit with its pointwise operands ROUNDED: a fault the exempt contract must reject."""
    sc, sh = bn_fold(sd, name + "/pw_norm")
    t = F.conv2d(x, sd[name + "/dw_conv3x3.weight"], None, stride, 1, groups=x.shape[1])
    return _epilogue(F.conv2d(rb(t), rb(sd[name + "/pw_conv1x1.weight"])), sc, sh, True, None)


def conv_bn(x, sd, name, stride, pad, rounded=True):
    sc, sh = bn_fold(sd, name + "/norm")
    return conv(x, sd[name + "/conv.weight"], scale=sc, shift=sh, stride=stride, pad=pad, relu=True, rounded=rounded)


def correlation(q, sup):
    """attn = relu(relu(q * k11) * k11) + relu(relu(q (*) k13) (*) k31) + q, depthwise, fp32 launch (oracle/ref_model.py correlation)."""
    q, sup = q.to(D), sup.to(D)
    C = q.shape[1]
    k11 = F.adaptive_avg_pool2d(sup, (1, 1)).permute(1, 0, 2, 3)
    k13 = F.adaptive_avg_pool2d(sup, (1, 3)).permute(1, 0, 2, 3)
    k31 = F.adaptive_avg_pool2d(sup, (3, 1)).permute(1, 0, 2, 3)
    a = F.relu(F.conv2d(F.relu(F.conv2d(q, k11, groups=C)), k11, groups=C))
    b = F.relu(F.conv2d(F.relu(F.conv2d(q, k13, padding=(0, 1), groups=C)), k31, padding=(1, 0), groups=C))
    return a + b + q


def head(tower, sd, level, prefix="proposal_generator.centernet_head."):
    """GroupNorm(32) + ReLU + the (l,t,r,b | hm) conv + per-level Scale: one fp32 launch -> [B, 5, h, w] (reg | hm)."""
    t = F.relu(F.group_norm(tower.to(D), 32, sd[prefix + "bbox_tower.1.weight"].double(), sd[prefix + "bbox_tower.1.bias"].double(), eps=1e-5))
    hm = F.conv2d(t, sd[prefix + "agn_hm.weight"].double(), sd[prefix + "agn_hm.bias"].double(), padding=1)
    rg = F.conv2d(t, sd[prefix + "bbox_pred.weight"].double(), sd[prefix + "bbox_pred.bias"].double(), padding=1)
    return torch.cat((F.relu(rg * sd[prefix + f"scales.{level}.scale"].double()), hm), 1)


def stem1(x_pre, sd):
    return conv_bn(x_pre, sd, P + "stem.stem_1", 2, 1, rounded=False)


def chain_concat_tail(cat, sd, cname, fw, fb, rounded=True):
    """Block 1 of a two-block stage: the concat conv (mfma, its output map is reused by block 2) + the fp32 eSE tail without identity;
    the gate comes from the mean of the unrounded float64 conv output, nothing is rounded between the links."""
    y = conv_bn(cat, sd, cname, 1, 0, rounded=rounded)
    return gated(y, gate(y, fw, fb))


def chain_reduction_unit(x, sd, rname, uname, rounded=True):
    """A depthwise stage: the 1x1 reduction conv (mfma) + unit 0 (fp32) on its float64 output."""
    return dw_unit(conv_bn(x, sd, rname, 1, 0, rounded=rounded), sd, uname, 1)


# ------------------------------------------------------------------------------------------------------------ checking
def errs(got, want):
    got, want = got.detach().double().numpy(), want.detach().double().numpy()
    assert got.shape == want.shape, (got.shape, want.shape)
    return rel_err(got, want), chan_err(got, want)


class Ledger:
    """Collects one line per checked launch and the failures; `hold` never raises, `assert_clean` does."""

    def __init__(self, tag=""):
        self.tag, self.rows, self.failed = tag, [], []

    def hold(self, launch, cls, got, want, twin=None, other=None, tol=TOL_LAYER):
        """got against the contract `want` at `tol`; an mfma / fold / chain launch also > TOL_LAYER from `twin` (the unrounded form);
        a lateral also > LATERAL_APART from `other` (the other pass's form)."""
        r, c = errs(got, want)
        row = {"launch": launch, "cls": cls, "rel": r, "chan": c, "twin": None, "other": None}
        if not (r < tol and c < tol):
            self.failed.append(f"{self.tag} {launch} [{cls}]: rel_err {r:.2e} chan_err {c:.2e} against its contract (tolerance {tol:.1e})")
        if twin is not None:
            row["twin"] = errs(got, twin)[0]
            if not row["twin"] > TOL_LAYER:
                self.failed.append(f"{self.tag} {launch} [{cls}]: only {row['twin']:.2e} from the unrounded conv -- not the reduced path")
        if other is not None:
            row["other"] = errs(got, other)[0]
            if not row["other"] > LATERAL_APART:
                self.failed.append(f"{self.tag} {launch} [{cls}]: only {row['other']:.2e} from the other lateral form")
        self.rows.append(row)
        return row

    def assert_clean(self):
        assert not self.failed, "\n".join(self.failed)


# ------------------------------------------------------------------------------------------------------------ a whole pass
def body_spec(body):
    """(spec, depthwise, blocks) of the three bodies this module walks."""
    from oracle import ref_model as R
    if body.endswith("-dw-eSE"):
        import vovnet_dw_ref as DW
        s = DW.DW_SPECS[body]
        return dict(stem=s["stem"], conv=s["conv"], out=s["out"], layers=s["layers"], blocks=(1, 1, 1, 1)), True
    return R.VOVNET_SPECS[body], False


def case_inputs(body, H, W):
    """(state dict, two fp32 images [2,3,H,W]) of a body: what both test modules feed.  V-39: the weights and the image statistics
    tests/test_hip_deep.py::test_every_stage_on_the_engines_own_inputs uses (tests/golden/deep_own_error.json: picked by the executed
    reference's own fp32 error, so that one stage is well conditioned); the one-block bodies are well conditioned at seed 0."""
    import json
    import os
    from conftest import GOLDEN
    from oracle import ref_model as R
    if body == "V-39-eSE":
        with open(os.path.join(GOLDEN, "deep_own_error.json")) as f:
            pick = json.load(f)["stagewise_input"][body]
        sd, iseed, istd = R.synth_state_dict(pick["weights_seed"], body), pick["image_seed"], pick["image_std"]
    elif body.endswith("-dw-eSE"):
        import vovnet_dw_ref as DW
        sd, iseed, istd = DW.synth_state_dict_dw(0, body), 3, 1.0
    else:
        sd, iseed, istd = R.synth_state_dict(0, body), 3, 1.0
    x = torch.randn(2, 3, H, W, generator=torch.Generator().manual_seed(iseed)) * istd
    return sd, (x + torch.tensor(R.PIXEL_MEAN).view(1, 3, 1, 1)).contiguous()


def geometry(H, W):
    """Map sizes at strides 2 .. 32 of an image padded to a multiple of 32 (stem_3: 3x3 s2 p1; ceil-mode pools)."""
    Hp, Wp = (H + 31) // 32 * 32, (W + 31) // 32 * 32
    hw = {1: (Hp // 2, Wp // 2)}
    hw[2] = ((hw[1][0] - 1) // 2 + 1, (hw[1][1] - 1) // 2 + 1)
    for k in (3, 4, 5):
        hw[k] = tuple(int(pool(torch.zeros(1, 1, hw[k - 1][0], hw[k - 1][1])).shape[2 + i]) for i in (0, 1))
    return hw


def buffer_names(body):
    spec, dw = body_spec(body)
    names = {"stem1": 1, "stem2": 1, "stem3": 2}
    for k in (2, 3, 4, 5):
        names.update({f"cat{k}": k, f"stage{k}": k, f"gate{k}": None})
        if spec["blocks"][k - 2] > 1:
            names.update({f"ycat{k}": k, f"icat{k}": k})
        if dw and (spec["stem"][2] if k == 2 else spec["out"][k - 3]) != spec["conv"][k - 2]:
            names[f"red{k}"] = k
    for l in (3, 4, 5):
        names.update({f"lat{l}": l, f"p{l}": l, f"attn{l}": l, f"pos{l}": l, f"tower{l}": l, f"head{l}": l})
    return names


def walk(body, sd, support, x_pre, S, led, heads=True):
    """Hold every launch of one pass.  x_pre [B,3,Hp,Wp]: the preprocessed, padded images; S: {buffer name: NCHW fp32 tensor} read
    from the engine after the pass ("gateK": [B, C]); led: a Ledger.  B == 1 is the one-image pass (fused column sums, gate-scaled
    lateral weights, the pooled gated input written by the gate kernel), B > 1 the batched one."""
    spec, dw = body_spec(body)
    B = x_pre.shape[0]
    L = spec["layers"]
    assert max(spec["blocks"]) <= 2, "bodies with more than two blocks per stage overwrite their ping-pong buffers: not walked"
    led.hold("stem_1", "exempt", S["stem1"], stem1(x_pre, sd))
    if dw:
        led.hold("stem_2", "exempt", S["stem2"], dw_unit(S["stem1"], sd, P + "stem.stem_2", 1))
        led.hold("stem_3", "exempt", S["stem3"], dw_unit(S["stem2"], sd, P + "stem.stem_3", 2))
    else:
        for nm, src, dst, st in (("stem_2", "stem1", "stem2", 1), ("stem_3", "stem2", "stem3", 2)):
            led.hold(nm, "mfma", S[dst], conv_bn(S[src], sd, P + "stem." + nm, st, 1), twin=conv_bn(S[src], sd, P + "stem." + nm, st, 1, rounded=False))
    cin = spec["stem"][2]
    for k in (2, 3, 4, 5):
        cc, oc, nblk = spec["conv"][k - 2], spec["out"][k - 2], spec["blocks"][k - 2]
        cat = S[f"cat{k}"]
        assert cat.shape[1] == cin + L * cc, (k, cat.shape)
        if k > 2:
            led.hold(f"pool{k}", "exempt", cat[:, :cin], pool(gated(S[f"stage{k - 1}"], S[f"gate{k - 1}"])))

        def layers(buf, c0, mod, tag):
            pre = f"{P}stage{k}.{mod}."
            src, dst = (0, c0), c0
            if dw:
                x, first = buf[:, :c0], f"{pre}layers.0.{mod}_0"
                rn = f"{pre}conv_reduction.{mod}_reduction_0"
                if rn + "/conv.weight" in sd:
                    led.hold(f"{tag}.reduction", "mfma", S[f"red{k}"], conv_bn(x, sd, rn, 1, 0), twin=conv_bn(x, sd, rn, 1, 0, rounded=False))
                    led.hold(f"{tag}.reduction+unit0", "chain", buf[:, c0:c0 + cc], chain_reduction_unit(x, sd, rn, first),
                             twin=chain_reduction_unit(x, sd, rn, first, rounded=False))
                    x = S[f"red{k}"]
                for i in range(L):
                    led.hold(f"{tag}.unit{i}", "exempt", buf[:, dst:dst + cc], dw_unit(x, sd, f"{pre}layers.{i}.{mod}_{i}", 1))
                    x = buf[:, dst:dst + cc]
                    dst += cc
                return
            for i in range(L):
                x, nm = buf[:, src[0]:src[1]], f"{pre}layers.{i}.{mod}_{i}"
                led.hold(f"{tag}.layer{i}", "mfma", buf[:, dst:dst + cc], conv_bn(x, sd, nm, 1, 1), twin=conv_bn(x, sd, nm, 1, 1, rounded=False))
                src, dst = (dst, dst + cc), dst + cc

        mod = f"OSA{k}_1"
        pre = f"{P}stage{k}.{mod}."
        layers(cat, cin, mod, f"s{k}b1")
        cname = f"{pre}concat.{mod}_concat"
        if nblk == 1:
            led.hold(f"s{k}b1.concat", "mfma", S[f"stage{k}"], conv_bn(cat, sd, cname, 1, 0), twin=conv_bn(cat, sd, cname, 1, 0, rounded=False))
            led.hold(f"gate{k}", "exempt", S[f"gate{k}"], gate(S[f"stage{k}"], sd[pre + "ese.fc.weight"], sd[pre + "ese.fc.bias"]))
        else:
            ic = S[f"icat{k}"]
            assert ic.shape[1] == oc + L * cc
            fw, fb = sd[pre + "ese.fc.weight"], sd[pre + "ese.fc.bias"]
            led.hold(f"s{k}b1.concat+tail", "chain", ic[:, :oc], chain_concat_tail(cat, sd, cname, fw, fb),
                     twin=chain_concat_tail(cat, sd, cname, fw, fb, rounded=False))
            mod2 = f"OSA{k}_2"
            pre2 = f"{P}stage{k}.{mod2}."
            layers(ic, oc, mod2, f"s{k}b2")
            c2 = f"{pre2}concat.{mod2}_concat"
            led.hold(f"s{k}b2.concat", "mfma", S[f"ycat{k}"], conv_bn(ic, sd, c2, 1, 0), twin=conv_bn(ic, sd, c2, 1, 0, rounded=False))
            g2 = gate(S[f"ycat{k}"], sd[pre2 + "ese.fc.weight"], sd[pre2 + "ese.fc.bias"])
            led.hold(f"s{k}b2.tail", "exempt", S[f"stage{k}"], tail(S[f"ycat{k}"], g2, ic[:, :oc]))
            assert bool((S[f"gate{k}"] == 1.0).all()), f"stage {k} ends in an identity block: its gate buffer holds ones"
        cin = oc
    # FPN, top-down
    for l in (5, 4, 3):
        x, g = S[f"stage{l}"], S[f"gate{l}"]
        w, b = sd[f"backbone.fpn_lateral{l}.weight"], sd[f"backbone.fpn_lateral{l}.bias"]
        top = S[f"lat{l + 1}"] if l < 5 else None
        add = None if top is None else upsample2(top, *x.shape[2:])
        twin = conv(gated(x, g), w, shift=b, add=add, rounded=False)
        if spec["blocks"][l - 2] > 1:                      # the stage's whole output is in "stageK": a plain conv
            led.hold(f"lateral{l}", "mfma", S[f"lat{l}"], conv(x, w, shift=b, add=add), twin=twin)
        elif B == 1:
            led.hold(f"lateral{l}", "fold-w", S[f"lat{l}"], lateral_one(x, g, w, b, top), twin=twin, other=lateral_batch(x, g, w, b, top))
        else:
            led.hold(f"lateral{l}", "fold-in", S[f"lat{l}"], lateral_batch(x, g, w, b, top), twin=twin,
                     other=torch.cat([lateral_one(x[i:i + 1], g[i:i + 1], w, b, None if top is None else top[i:i + 1]) for i in range(B)]))
        wo, bo = sd[f"backbone.fpn_output{l}.weight"], sd[f"backbone.fpn_output{l}.bias"]
        row = led.hold(f"output{l}", "exempt", S[f"p{l}"], conv(S[f"lat{l}"], wo, shift=bo, pad=1, rounded=False))
        row["twin"] = errs(S[f"p{l}"], conv(S[f"lat{l}"], wo, shift=bo, pad=1))[0]      # (logged: its distance from the ROUNDED form)
    if not heads:
        return
    hp = "proposal_generator.centernet_head."
    for l in (3, 4, 5):
        q = S[f"p{l}"]
        led.hold(f"correlation{l}", "exempt", S[f"attn{l}"], correlation(q, support[f"p{l}"]))
        pc = torch.cat((S[f"attn{l}"], q), 1)
        led.hold(f"conv3.{l}", "mfma", S[f"pos{l}"], conv(pc, sd["conv3.weight"], shift=sd["conv3.bias"], relu=True),
                 twin=conv(pc, sd["conv3.weight"], shift=sd["conv3.bias"], relu=True, rounded=False))
        tw, tb = sd[hp + "bbox_tower.0.weight"], sd[hp + "bbox_tower.0.bias"]
        led.hold(f"tower{l}", "mfma", S[f"tower{l}"], conv(S[f"pos{l}"], tw, shift=tb, pad=1), twin=conv(S[f"pos{l}"], tw, shift=tb, pad=1, rounded=False))
        led.hold(f"head{l}", "exempt", S[f"head{l}"], head(S[f"tower{l}"], sd, l - 3))
