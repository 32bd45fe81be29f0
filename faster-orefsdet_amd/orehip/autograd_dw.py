"""torch.autograd binding of one OSA block of the depthwise VoVNet bodies (V-19-slim-dw-eSE, V-19-dw-eSE), beside OSAFn and with
its conventions: one concat buffer, ore_relu_affine_bwd on its slices, direct_grad.  Re-exported by orehip.autograd (OSADwFn,
osa_block_dw).  Every orehip call made here is listed with the test that holds it to float64 (tests/vovnet_dw_ref.py OSA_DW_CALLS,
tests/test_vovnet_dw_host.py::test_every_autograd_dw_call_is_listed), the way tests/trainops_ref.py lists those of orehip/autograd.py."""
from __future__ import annotations

from typing import List, Optional

import torch
from torch.autograd import Function

import orehip


def packed(w, dgrad):
    from orehip import autograd as A          # (at call time: orehip.autograd imports this module at its end)
    return A.packed(w, dgrad)


def direct_grad(p):
    from orehip import autograd as A
    return A.direct_grad(p)


class OSADwFn(Function):
    """One OSA block of the depthwise bodies up to (not including) eSE (d2z:modeling/backbone/vovnet.py:110-130, 284-332): an optional
    1x1 `conv_reduction` (+ FrozenBN + ReLU) into its OWN buffer -- it feeds layer 0 and is not part of the concat -- then n x
    [depthwise 3x3 -> pointwise 1x1 -> FrozenBN -> ReLU] (orehip.dwpw, one launch each) chained through the channel slices of one concat
    buffer, then conv1x1 + FrozenBN + ReLU over the buffer.  args: x_in, has_reduction, then the reduction's (weight, scale, shift) if
    any, per layer (w_dw, w_pw, scale, shift), the concat conv's (weight, scale, shift).
    The backward recomputes each unit's depthwise output (the X of the pointwise weight gradient) instead of storing it."""

    @staticmethod
    def forward(ctx, x_in, has_red: bool, *args):
        red = args[:3] if has_red else None
        rest = args[3:] if has_red else args
        n = (len(rest) - 3) // 4
        wdw, wpw, scs, shs = rest[0:4 * n:4], rest[1:4 * n:4], rest[2:4 * n:4], rest[3:4 * n:4]
        wc, scc, shc = rest[4 * n:]
        x_in = x_in.contiguous()
        B, H, W, in_ch = x_in.shape
        C = wdw[0].shape[0]
        assert has_red or in_ch == C, "a block whose input width differs from its stage width has a conv_reduction"
        cat = torch.empty(B, H, W, in_ch + n * C, device=x_in.device, dtype=torch.float32)
        cat[..., :in_ch] = x_in
        r = None
        if has_red:
            r = orehip.conv2d(cat, packed(red[0], False), C, 1, 1, 0, in_coff=0, Cin=in_ch, scale=red[1], shift=red[2], relu_cout=C)
        for i in range(n):
            src_buf, src = (r, 0) if (i == 0 and has_red) else (cat, in_ch + (i - 1) * C if i else 0)
            orehip.dwpw(src_buf, wdw[i], packed(wpw[i], False), C, 1, scs[i], shs[i], in_coff=src, out=cat, out_coff=in_ch + i * C)
        y = orehip.conv2d(cat, packed(wc, False), wc.shape[0], 1, 1, 0, scale=scc, shift=shc, relu_cout=wc.shape[0])
        ctx.save_for_backward(cat, y, r, scc, wc, *(red[:2] if has_red else ()), *wdw, *wpw, *scs)
        ctx.meta = (n, in_ch, C, has_red)
        return y

    @staticmethod
    def backward(ctx, dy):
        n, in_ch, C, has_red = ctx.meta
        saved = ctx.saved_tensors
        cat, y, r, scc, wc = saved[:5]
        o = 5
        if has_red:
            wr, scr = saved[5:7]
            o = 7
        wdw, wpw, scs = saved[o:o + n], saved[o + n:o + 2 * n], saved[o + 2 * n:o + 3 * n]
        a0 = 2 + (3 if has_red else 0)                         # index of the first layer tensor among forward's inputs
        need = ctx.needs_input_grad
        grads: List[Optional[torch.Tensor]] = [None] * (len(need) - 2)

        def pw_wgrad(w, xbuf, dzi, **kw):                      # 1x1 weight gradient: into the parameter's gradient where allowed
            dg = direct_grad(w)
            if dg is not None:
                orehip.conv2d_wgrad(xbuf, dzi, 1, out=dg, beta=1.0, **kw)
                return None
            return orehip.conv2d_wgrad(xbuf, dzi, 1, **kw)

        def dw_wgrad(w, xbuf, dt, x_coff):
            dg = direct_grad(w)
            if dg is not None:
                orehip.dw3x3_wgrad(xbuf, dt, C, x_coff=x_coff, out=dg, beta=1.0)
                return None
            return orehip.dw3x3_wgrad(xbuf, dt, C, x_coff=x_coff)

        dz = orehip.relu_affine_bwd(dy.contiguous(), y, scc)
        if need[a0 + 4 * n]:
            grads[a0 - 2 + 4 * n] = pw_wgrad(wc, cat, dz)
        dcat = orehip.conv2d(dz, packed(wc, True), cat.shape[-1], 1, 1, 0)              # gradient of every concat slice
        for i in range(n - 1, -1, -1):
            dst = in_ch + i * C
            via_red = i == 0 and has_red
            src_buf, src = (r, 0) if via_red else (cat, dst - C if i else 0)
            dzi = orehip.relu_affine_bwd(dcat, cat, scs[i], dy_coff=dst, y_coff=dst, Cc=C)
            gi = a0 - 2 + 4 * i
            if need[a0 + 4 * i + 1]:
                t = orehip.dw3x3(src_buf, wdw[i], C, 1, in_coff=src)                    # the depthwise output, recomputed
                grads[gi + 1] = pw_wgrad(wpw[i], t, dzi)
            dt = orehip.conv2d(dzi, packed(wpw[i], True), C, 1, 1, 0)
            if need[a0 + 4 * i]:
                grads[gi] = dw_wgrad(wdw[i], src_buf, dt, src)
            if via_red:
                dzr = orehip.relu_affine_bwd(orehip.dw3x3(dt, wdw[i], C, 1, dgrad=True), r, scr)
                if need[2]:
                    grads[0] = pw_wgrad(wr, cat, dzr, x_coff=0, Cin=in_ch)
                if need[0]:
                    dcat[..., :in_ch].add_(orehip.conv2d(dzr, packed(wr, True), in_ch, 1, 1, 0))
            elif i > 0 or need[0]:
                orehip.dw3x3(dt, wdw[i], C, 1, dgrad=True, out=dcat, out_coff=src, accumulate=True)
        gx = dcat[..., :in_ch].contiguous() if need[0] else None
        return (gx, None, *grads)


def osa_block_dw(x_in, reduction, layers, concat):
    """reduction: (weight, scale, shift) or None; layers: [(w_dw, w_pw, scale, shift)]; concat: (weight, scale, shift)."""
    flat = list(reduction or ()) + [t for quad in layers for t in quad] + list(concat)
    return OSADwFn.apply(x_in, reduction is not None, *flat)
