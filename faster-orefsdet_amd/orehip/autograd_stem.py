"""torch.autograd bindings of the stride-2 convolutions and of the VoVNet stem (MODEL.BACKBONE.FREEZE_AT: 0), part of orehip.autograd's
interface like autograd_dw.py.

    ConvS2Fn   conv 3x3 / stride 2 / pad 1 (+ FrozenBN scale / shift or bias, + ReLU): ore_conv2d_fwd | ore_relu_affine_bwd,
               ore_conv2d_wgrad_s2_fwd, ore_conv2d_dgrad_s2_fwd (ore_colsum_fwd for a bias)
    StemFn     stem_1 -> stem_2 -> stem_3 of a dense body as one node.  The forward issues the launches of the frozen stem
               (ore_stem1_fwd from the raw or normalised image, the stem_2 conv launch, the stem_3 conv launch into the first slice of
               stage 2's concat buffer), so its output is bit-equal to the frozen path's; the backward chains stem_3 (the two stride-2
               kernels), stem_2 (the stride-1 kernels of ConvFn) and stem_1 (ore_stem1_wgrad_fwd: no data gradient, the image is a leaf).
Every weight gradient honours direct_grad (accumulated by the kernel into the flat bucket's `.grad` with beta = 1)."""
from __future__ import annotations

import torch
from torch.autograd import Function

import orehip
from orehip.autograd import _c16, _conv_backward, direct_grad, packed, packed_wino


def _wgrad_s2(x, dz, weight, **kw):
    """dW of a stride-2 conv: into the parameter's gradient where allowed (-> None), else returned to autograd."""
    dg = direct_grad(weight)
    if dg is not None:
        orehip.conv2d_wgrad_s2(x, dz, out=dg.view(weight.shape), beta=1.0, **kw)
        return None
    return orehip.conv2d_wgrad_s2(x, dz, **kw)


class ConvS2Fn(Function):
    """y = act(conv(x, W) * scale + shift) or act(conv(x, W) + bias); x [B,H,W,Cin] NHWC, W [Cout,Cin,3,3], stride 2, pad 1."""

    @staticmethod
    def forward(ctx, x, weight, scale, shift, relu: bool, bias=None):
        x = x.contiguous()
        Cout, Cin = weight.shape[:2]
        assert tuple(weight.shape[2:]) == (3, 3) and Cin % 16 == 0 and Cout % 4 == 0 and x.shape[-1] == Cin, (tuple(weight.shape), tuple(x.shape))
        co16 = _c16(Cout)
        B, H, W, _ = x.shape
        out = None
        if co16 != Cout:
            out = torch.zeros(B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, co16, device=x.device, dtype=torch.float32)
        sh = shift if shift is not None else (bias.detach().contiguous() if bias is not None else None)
        y = orehip.conv2d(x, packed(weight, False), Cout, 3, 2, 1, scale=scale, shift=sh, relu_cout=Cout if relu else 0, out=out)
        ctx.save_for_backward(x, weight, scale, y if relu else None)
        ctx.bias_ref = bias
        ctx.meta = (relu, Cout, Cin, co16)
        return y if co16 == Cout else y[..., :Cout]

    @staticmethod
    def backward(ctx, dy):
        x, weight, scale, y = ctx.saved_tensors
        relu, Cout, Cin, co16 = ctx.meta
        # dZ over the Cout real channels only (scale has Cout entries; y is co16 wide when the forward padded its output)
        dy = dy.contiguous()
        if relu:
            dz = orehip.relu_affine_bwd(dy, y, scale, Cc=Cout)
        elif scale is not None:
            dz = dy * scale
        else:
            dz = dy
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = orehip.conv2d_dgrad_s2(dz, weight.detach().contiguous(), x.shape[1], x.shape[2])
        if ctx.needs_input_grad[1]:
            gw = _wgrad_s2(x, dz, weight)
        if ctx.bias_ref is not None and ctx.needs_input_grad[5]:
            dgb = direct_grad(ctx.bias_ref)
            if dgb is not None:
                orehip.colsum(dz, out=dgb, beta=1.0)
            else:
                gb = orehip.colsum(dz)
        return gx, gw, None, None, None, gb


def conv_s2(x, weight, scale=None, shift=None, relu=False, bias=None):
    return ConvS2Fn.apply(x, weight, scale, shift, relu, bias)


class StemFn(Function):
    """The three stem layers of a dense VoVNet body with trainable weights.  img: [B,3,H,W], raw (uint8 / fp32, raw_norm = (mean, std, Hp,
    Wp)) or normalised and padded (raw_norm None).  fold2 / fold3: (scale, shift) of the folded FrozenBN of stem_2 / stem_3; stem_1 goes
    through `stem1`, the module's own launch (VoVNet.stem_hip).  cat_ch: width of stage 2's first concat buffer, whose first slice stem_3
    writes as in the frozen path.  Returns that slice as a contiguous [B,H/4,W/4,C3] tensor."""

    @staticmethod
    def forward(ctx, img, stem1, raw_norm, cat_ch: int, scale1, w1, w2, scale2, shift2, w3, scale3, shift3):
        y1 = stem1(img, raw_norm)
        C2, C3 = w2.shape[0], w3.shape[0]
        y2 = orehip.conv2d(y1, packed(w2, False), C2, 3, 1, 1, scale=scale2, shift=shift2, relu_cout=C2, w_wino=packed_wino(w2, False))
        B, H, W, _ = y2.shape
        # The cat_ch-wide buffer exists only for launch identity: stem_3 writes rows of cat_ch floats exactly as in the frozen path (the conv
        # plan depends on out_ld), and the slice is copied out as VoVNet._stage_train does there.  Writing a C3-wide tensor directly would be one
        # copy less and could change the launch -- and with it the bit-equality tests/test_hip_freeze_at.py holds the model to.
        cat = torch.empty(B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, cat_ch, device=y2.device, dtype=torch.float32)
        orehip.conv2d(y2, packed(w3, False), C3, 3, 2, 1, scale=scale3, shift=shift3, relu_cout=C3, out=cat, out_coff=0)
        y3 = cat[..., :C3].contiguous()
        ctx.save_for_backward(img, y1, y2, y3, w1, w2, w3, scale1, scale2, scale3)
        if raw_norm is not None:
            mean, std, Hp, Wp = raw_norm
            ctx.norm = (tuple(mean), tuple(std), int(Hp), int(Wp))
        else:
            ctx.norm = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), img.shape[2], img.shape[3])
        return y3

    @staticmethod
    def backward(ctx, dy):
        img, y1, y2, y3, w1, w2, w3, sc1, sc2, sc3 = ctx.saved_tensors
        need1, need2, need3 = ctx.needs_input_grad[5], ctx.needs_input_grad[6], ctx.needs_input_grad[9]
        g1 = g2 = g3 = None
        dz3 = orehip.relu_affine_bwd(dy.contiguous(), y3, sc3)
        if need3:
            g3 = _wgrad_s2(y2, dz3, w3)
        if need1 or need2:
            dy2 = orehip.conv2d_dgrad_s2(dz3, w3.detach().contiguous(), y2.shape[1], y2.shape[2])
            dz2 = orehip.relu_affine_bwd(dy2, y2, sc2)
            dy1, g2, _ = _conv_backward(y1, 0, y1.shape[-1], w2, dz2, 3, need1, need2, False)
            if need1:
                dz1 = orehip.relu_affine_bwd(dy1, y1, sc1)
                mean, std, Hp, Wp = ctx.norm
                img = img.contiguous()                       # what VoVNet.stem_hip handed the forward kernel
                if img.dtype not in (torch.uint8, torch.float32):
                    img = img.float()
                dg = direct_grad(w1)
                if dg is not None:
                    orehip.stem1_wgrad(img, Hp, Wp, mean, std, dz1, out=dg.view(w1.shape), beta=1.0)
                else:
                    g1 = orehip.stem1_wgrad(img, Hp, Wp, mean, std, dz1)
        return None, None, None, None, None, g1, g2, None, None, g3, None, None


def stem(img, stem1, raw_norm, cat_ch, scale1, w1, fold2, fold3):
    """fold2 = (w2, scale2, shift2), fold3 = (w3, scale3, shift3)."""
    return StemFn.apply(img, stem1, raw_norm, cat_ch, scale1, w1, *fold2, *fold3)
