"""Plain-torch restatement of the depthwise VoVNet bodies (V-19-slim-dw-eSE, V-19-dw-eSE) and of their kernels, NCHW.

Used three ways: in fp32 it reproduces the fixtures recorded from the executed reference (tests/golden/backbone_fpn_dw_96x128.npz,
dw_units.npz; tools/gen_golden_vovnet_dw.py), in fp64 it is the reference of the HIP kernels and of the OSA block's gradients
(tests/test_hip_dw.py), and synth_state_dict_dw draws the weights both sides load.

What the bodies are (d2z:modeling/backbone/vovnet.py:28-48, 110-130, 284-332, checked against the executed reference):
  unit   X/dw_conv3x3 (groups = C, carries the stride, pad 1, no bias) -> X/pw_conv1x1 (no bias) -> X/pw_norm (FrozenBN) -> ReLU, with
         nothing between the two convs; C_in == C_out everywhere
  stem   stem_1 the ordinary 3 -> 64 3x3 stride-2 conv, stem_2 a unit at stride 1, stem_3 a unit at stride 2
  block  if in_ch != stage_ch a 1x1 conv_reduction (+ norm + ReLU) feeds layer 0 and is NOT part of the concat; three units;
         concat [x, l0, l1, l2] -> 1x1 -> eSE; ceil-mode 3x3 stride-2 max-pool in front of stages 3..5

The bf16-operand mode (include/ore_hip.h ORE_CONV_BF16) of these bodies, `with operand_precision("bf16"):` -- the units are fp32 whatever
the mode (depthwise taps AND the pointwise conv: ore_dwpw_fwd never rounds), stem_1 is fp32 as in every body, and the convs that run on
the matrix cores -- a stage's 1x1 reduction conv and its 1x1 concat conv, the FPN convs -- round both operands to bf16 where they enter
the conv.  `engine_pass="one" | "batch"` selects the statement of an engine's pass (oracle/ref_model.py: the FPN output convs fp32, the
one-image lateral with the gate folded into its weight).  Outside the scope nothing here changes.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

DW_SPECS = {
    "V-19-slim-dw-eSE": dict(stem=(64, 64, 64), conv=(64, 80, 96, 112), out=(112, 256, 384, 512), layers=3, dense="V-19-slim-eSE"),
    "V-19-dw-eSE": dict(stem=(64, 64, 64), conv=(128, 160, 192, 224), out=(256, 512, 768, 1024), layers=3, dense="V-19-eSE"),
}
P = "backbone.bottom_up."
U24 = 2.0 ** -24


# ------------------------------------------------------------------------------------------------ weights
def synth_backbone_dw(seed: int, body: str) -> Dict[str, torch.Tensor]:
    """The bottom-up weights under `backbone.bottom_up.`, drawn as oracle.ref_model.synth_state_dict draws conv_bn: He-normal convs
    (std sqrt(2 / fan_in)), FrozenBN weight and variance in [0.5, 1.5], bias and mean N(0, 0.1), eSE as there.  The one exception is the
    depthwise conv, std sqrt(1 / 9): no ReLU follows it, so the He factor 2 (which makes up for the half a ReLU removes) would double
    the variance in every unit and the activations of a 14-unit body would grow by 2^7.
    Which seed the fixtures use is recorded in them (tools/gen_golden_vovnet_dw.py explains the choice)."""
    g = torch.Generator().manual_seed(seed)
    spec = DW_SPECS[body]
    sd: Dict[str, torch.Tensor] = {}

    def randn(*shape, std=1.0):
        return torch.randn(*shape, generator=g) * std

    def rand(*shape, lo=0.0, hi=1.0):
        return torch.rand(*shape, generator=g) * (hi - lo) + lo

    def bn(name, c):
        sd[name + ".weight"] = rand(c, lo=0.5, hi=1.5)
        sd[name + ".bias"] = randn(c, std=0.1)
        sd[name + ".running_mean"] = randn(c, std=0.1)
        sd[name + ".running_var"] = rand(c, lo=0.5, hi=1.5)

    def conv_bn(name, cin, cout, k):
        sd[name + "/conv.weight"] = randn(cout, cin, k, k, std=math.sqrt(2.0 / (cin * k * k)))
        bn(name + "/norm", cout)

    def unit(name, c):
        sd[name + "/dw_conv3x3.weight"] = randn(c, 1, 3, 3, std=math.sqrt(1.0 / 9.0))
        sd[name + "/pw_conv1x1.weight"] = randn(c, c, 1, 1, std=math.sqrt(2.0 / c))
        bn(name + "/pw_norm", c)

    stem = spec["stem"]
    conv_bn(P + "stem.stem_1", 3, stem[0], 3)
    unit(P + "stem.stem_2", stem[1])
    unit(P + "stem.stem_3", stem[2])
    cin = stem[2]
    for si in range(4):
        k = si + 2
        sc, oc = spec["conv"][si], spec["out"][si]
        mod = f"OSA{k}_1"
        pre = f"{P}stage{k}.{mod}."
        for i in range(spec["layers"]):
            unit(f"{pre}layers.{i}.{mod}_{i}", sc)
        if cin != sc:
            conv_bn(f"{pre}conv_reduction.{mod}_reduction_0", cin, sc, 1)
        conv_bn(f"{pre}concat.{mod}_concat", cin + spec["layers"] * sc, oc, 1)
        sd[pre + "ese.fc.weight"] = randn(oc, oc, 1, 1, std=math.sqrt(1.0 / oc))
        sd[pre + "ese.fc.bias"] = randn(oc, std=0.5)
        cin = oc
    return sd


def synth_state_dict_dw(seed: int = 0, body: str = "V-19-slim-dw-eSE") -> Dict[str, torch.Tensor]:
    """A whole model's state dict with the depthwise bottom-up: everything outside `backbone.bottom_up.` (FPN, correlation, head) is
    oracle.ref_model.synth_state_dict's for the dense body of the same widths."""
    from oracle import ref_model as R
    sd = {k: v for k, v in R.synth_state_dict(seed, body=DW_SPECS[body]["dense"]).items() if not k.startswith(P)}
    sd.update(synth_backbone_dw(seed, body))
    return sd


# ------------------------------------------------------------------------------------------------ the network
def operand_precision(mode: str, engine_pass=None):
    """The oracle's scope (oracle.ref_model.operand_precision): one switch for the dense and the depthwise bodies."""
    from oracle import ref_model as R
    return R.operand_precision(mode, engine_pass=engine_pass)


def _bn(x, sd, name, eps=1e-5):
    sc = sd[name + ".weight"] / torch.sqrt(sd[name + ".running_var"] + eps)
    sh = sd[name + ".bias"] - sd[name + ".running_mean"] * sc
    return x * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)


def conv_bn_relu(x, sd, name, stride, pad):
    from oracle import ref_model as R
    if name.endswith("stem.stem_1"):                         # Cin = 3: fp32 in every mode
        return F.relu(_bn(F.conv2d(x, sd[name + "/conv.weight"], None, stride, pad), sd, name + "/norm"))
    return F.relu(_bn(R.dense_conv(x, sd[name + "/conv.weight"], None, stride, pad), sd, name + "/norm"))   # reduction / concat: an MFMA conv


def dw_unit(x, sd, name, stride):
    """fp32 in every operand mode: neither the taps nor the pointwise operands are rounded."""
    c = x.shape[1]
    t = F.conv2d(x, sd[name + "/dw_conv3x3.weight"], None, stride, 1, groups=c)
    return F.relu(_bn(F.conv2d(t, sd[name + "/pw_conv1x1.weight"]), sd, name + "/pw_norm"))


def ese(x, sd, prefix):
    from oracle import ref_model as R
    s = F.relu6(F.conv2d(F.adaptive_avg_pool2d(x, 1), sd[prefix + "fc.weight"], sd[prefix + "fc.bias"]) + 3.0) / 6.0
    y = x * s
    if R._ENGINE_PASS == "one":
        y._ore_gated = (x, s)                                # the one-image lateral folds the gate into its weight (ref_model.fpn)
    return y


def osa_stage_dw(x, sd, k: int, layers: int = 3, prefix: str = P):
    """_OSA_stage k (2..5) of a depthwise body: ceil-mode pooling for k > 2, then the block."""
    mod = f"OSA{k}_1"
    pre = f"{prefix}stage{k}.{mod}."
    if k != 2:
        x = F.max_pool2d(x, kernel_size=3, stride=2, ceil_mode=True)
    feats = [x]
    y = x
    red = f"{pre}conv_reduction.{mod}_reduction_0"
    if red + "/conv.weight" in sd:
        y = conv_bn_relu(y, sd, red, 1, 0)
    for i in range(layers):
        y = dw_unit(y, sd, f"{pre}layers.{i}.{mod}_{i}", 1)
        feats.append(y)
    y = conv_bn_relu(torch.cat(feats, 1), sd, f"{pre}concat.{mod}_concat", 1, 0)
    return ese(y, sd, pre + "ese.")


def vovnet_dw(x, sd, prefix: str = P) -> Dict[str, torch.Tensor]:
    x = conv_bn_relu(x, sd, prefix + "stem.stem_1", 2, 1)
    x = dw_unit(x, sd, prefix + "stem.stem_2", 1)
    x = dw_unit(x, sd, prefix + "stem.stem_3", 2)
    out = {"stem": x}
    for k in (2, 3, 4, 5):
        x = osa_stage_dw(x, sd, k, prefix=prefix)
        out[f"stage{k}"] = x
    return out


def backbone_fpn_dw(x, sd) -> Dict[str, torch.Tensor]:
    """p3 / p4 / p5 (d2z:modeling/backbone/fpn.py:113-154, TOP_LEVELS 0, fuse "sum", bias, no norm)."""
    from oracle import ref_model as R
    f = vovnet_dw(x, sd)
    if R._OPERANDS != "fp32":
        return R.fpn(f, sd)                                  # the mode's statement of the FPN is the dense bodies'
    res, prev = {}, None
    for st in (5, 4, 3):
        lat = F.conv2d(f[f"stage{st}"], sd[f"backbone.fpn_lateral{st}.weight"], sd[f"backbone.fpn_lateral{st}.bias"])
        prev = lat if prev is None else lat + F.interpolate(prev, scale_factor=2.0, mode="nearest")
        res[f"p{st}"] = F.conv2d(prev, sd[f"backbone.fpn_output{st}.weight"], sd[f"backbone.fpn_output{st}.bias"], 1, 1)
    return res


# ------------------------------------------------------------------------------------------------ kernel references (fp64) and bounds
def dw3x3_ref(x, w_dw, stride: int = 1, flip: bool = False):
    """x [B,C,H,W], w_dw [C,1,3,3] -> the depthwise conv in x's dtype; flip: mirrored taps (the data gradient at stride 1)."""
    w = w_dw.to(x.dtype)
    return F.conv2d(x, w.flip(2, 3) if flip else w, None, stride, 1, groups=x.shape[1])


def dw3x3_bound(x, w_dw, stride: int = 1, flip: bool = False):
    """12 * 2^-24 * (|W_dw| (*) |x|): 9 products and 8 additions of any order, with room for the accumulate form."""
    return 12 * U24 * dw3x3_ref(x.abs().double(), w_dw.abs().double(), stride, flip)


def dwpw_ref(x, w_dw, w_pw, scale, shift, stride: int = 1, mask=None):
    """The unit in fp64: (pre-activation, output).  mask: a given ReLU mask (output = pre * mask) instead of pre > 0."""
    d = torch.float64
    t = dw3x3_ref(x.to(d), w_dw, stride)
    pre = F.conv2d(t, w_pw.to(d)) * scale.to(d).view(1, -1, 1, 1) + shift.to(d).view(1, -1, 1, 1)
    return pre, (F.relu(pre) if mask is None else pre * mask.to(d))


def dwpw_bound(x, w_dw, w_pw, scale, shift, stride: int = 1):
    """(C + 16) * 2^-24 * (|scale| * (|W_pw| * (|W_dw| (*) |x|)) + |shift|): the worst case of any summation order of the 9 + C
    products plus the epilogue; ReLU does not increase a difference."""
    d = torch.float64
    C = x.shape[1]
    t = dw3x3_ref(x.abs().to(d), w_dw.abs(), stride)
    m = F.conv2d(t, w_pw.abs().to(d)) * scale.abs().to(d).view(1, -1, 1, 1) + shift.abs().to(d).view(1, -1, 1, 1)
    return (C + 16) * U24 * m


def dw3x3_wgrad_ref(x, dt, absolute: bool = False):
    """x, dt [B,C,H,W] fp64 -> dW [C,1,3,3] = sum_{b,y,x} x[b,c,y+ky-1,x+kx-1] * dt[b,c,y,x]; absolute: of the absolute values."""
    x, dt = x.double(), dt.double()
    if absolute:
        x, dt = x.abs(), dt.abs()
    B, C, H, W = x.shape
    xp = F.pad(x, (1, 1, 1, 1))
    out = torch.empty(C, 1, 3, 3, dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            out[:, 0, ky, kx] = (xp[:, :, ky:ky + H, kx:kx + W] * dt).sum((0, 2, 3))
    return out


def dw3x3_wgrad_bound(x, dt):
    """(n + 8) * 2^-24 * sum |x| |dT| per tap, n = B * H * W summed terms (any order; the kernel's plan -- 16 lanes x 16 pixels, 16
    lanes, then the parts of 256 pixels in order -- is one such order and has no tighter closed form worth restating)."""
    n = x.shape[0] * x.shape[2] * x.shape[3]
    return (n + 8) * U24 * dw3x3_wgrad_ref(x, dt, absolute=True)


# ------------------------------------------------------------------------------------------------ one OSA block with given masks (fp64)
def osa_block_dw_ref(x, reduction, layers, concat, masks: Optional[Sequence[torch.Tensor]] = None):
    """x [B,in_ch,H,W] fp64; reduction (w, scale, shift) | None; layers [(w_dw, w_pw, scale, shift)]; concat (w, scale, shift).
    masks: the ReLU masks to use, in the order [reduction?, layer 0.., concat] (each [B,C,H,W], 0/1); None = the sign of the
    pre-activation.  Returns (y, [pre-activations in the same order])."""
    pres: List[torch.Tensor] = []
    it = iter(masks) if masks is not None else None

    def act(pre):
        pres.append(pre)
        return F.relu(pre) if it is None else pre * next(it).to(pre.dtype)

    def affine(z, sc, sh):
        return z * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)

    y = x
    if reduction is not None:
        w, sc, sh = reduction
        y = act(affine(F.conv2d(x, w), sc, sh))
    feats = [x]
    for w_dw, w_pw, sc, sh in layers:
        y = act(affine(F.conv2d(dw3x3_ref(y, w_dw), w_pw), sc, sh))
        feats.append(y)
    w, sc, sh = concat
    return act(affine(F.conv2d(torch.cat(feats, 1), w), sc, sh)), pres


def conv1x1_pre_and_bound(x, w, scale, shift):
    """A 1x1 conv + affine in fp64 on x [B,Cin,H,W] and what an fp32 launch on the same input can be off by:
    (Cin + 16) * 2^-24 * (|scale| * (|W| * |x|) + |shift|)."""
    d = torch.float64
    sc, sh = scale.to(d).view(1, -1, 1, 1), shift.to(d).view(1, -1, 1, 1)
    pre = F.conv2d(x.to(d), w.to(d)) * sc + sh
    return pre, (w.shape[1] + 16) * U24 * (F.conv2d(x.abs().to(d), w.abs().to(d)) * sc.abs() + sh.abs())


# Every orehip call orehip/autograd_dw.py makes, with the test that holds it to float64 (the training-path guarantee of
# tests/trainops_ref.py, kept for the depthwise block: tests/test_vovnet_dw_host.py::test_every_autograd_dw_call_is_listed).
OSA_DW_CALLS = {
    "dwpw": "tests/test_hip_dw.py: element-wise against fp64, bound dwpw_bound",
    "dw3x3": "tests/test_hip_dw.py: forward and flipped-tap data gradient element-wise against fp64, bound dw3x3_bound",
    "dw3x3_wgrad": "tests/test_hip_dw.py: element-wise against fp64, bound dw3x3_wgrad_bound",
    "conv2d": "the 1x1 convs and their data gradients: tests/dgrad_ref.py, tests/test_hip_dgrad.py",
    "conv2d_wgrad": "the 1x1 weight gradients: tests/wgrad_ref.py, tests/test_hip_wgrad.py",
    "relu_affine_bwd": "ReLU / FrozenBN masks, bitwise: tests/test_hip_dgrad.py",
}
