"""CPU: tests/optim_ref.py restates torch.nn.utils.clip_grad_norm_ + torch.optim.SGD(nesterov=...), its fp32 emulation passes the
bounds, the faults a norm-clip kernel can have fail them, build_optimizer builds every mode the reference's solver has, and the special
values behave as the installed torch's."""
import math
import os
import re

import numpy as np
import pytest
import torch

import optim_ref as O
import trainloss_ref as TL
from conftest import PKG

INF = float("inf")
NUMELS = [1, 255, 256, 257, 700, 256 * O.GN_G + 1, 5, 300]          # small: the CPU tests need no more than two partials


def _t64(a):
    return torch.as_tensor(np.asarray(a, dtype=np.float64))


def _ok(got, x):
    h, r = TL.hold(_t64(got), x)
    return h <= 1 and r <= 1


def _torch_steps(p, g_steps, buf, numels, lr, wd, lr_scale, momentum, clip, gs, clip_type, norm_type, nesterov, dtype):
    """clip_grad_norm_ (per parameter, or over all) + torch.optim.SGD in `dtype` on the parameters cut out of the bucket -> per step
    (list of parameters, list of momentum buffers, norms)."""
    offs, _ = O.layout(numels)
    ps = [torch.nn.Parameter(p[o:o + n].to(dtype).clone()) for o, n in zip(offs, numels)]
    groups = []
    for q, o in zip(ps, offs):                                          # lr / wd change per chunk: one group per chunk-sized piece is not
        groups.append({"params": [q], "lr": 0.0, "weight_decay": 0.0})  # expressible, so the inputs keep them constant per parameter
    opt = torch.optim.SGD(groups, lr=0.1, momentum=float(np.float32(momentum)), nesterov=nesterov)
    for gi, (q, o) in enumerate(zip(ps, offs)):
        opt.param_groups[gi]["lr"] = float(np.float32(lr[o // 256]) * np.float32(lr_scale)) if dtype == torch.float32 else \
            float(np.float64(np.float32(lr[o // 256])) * np.float64(np.float32(lr_scale)))
        opt.param_groups[gi]["weight_decay"] = float(wd[o // 256])
        opt.state[q]["momentum_buffer"] = buf[o:o + numels[gi]].to(dtype).clone()
    out = []
    for g in g_steps:
        for q, o, n in zip(ps, offs, numels):
            q.grad = g[o:o + n].to(dtype) * float(np.float32(gs))
        if clip_type == "norm":
            norms = [torch.nn.utils.clip_grad_norm_(q, clip, norm_type) for q in ps]
        elif clip_type == "full_model":
            norms = [torch.nn.utils.clip_grad_norm_(ps, clip, norm_type)]
        else:
            norms = []
            torch.nn.utils.clip_grad_value_(ps, clip)
        opt.step()
        out.append(([q.detach().clone() for q in ps], [opt.state[q]["momentum_buffer"].clone() for q in ps], [float(v) for v in norms]))
    return out


def _per_param_const(numels, lr, wd):
    """lr / wd constant inside a parameter (torch.optim has one value per group)."""
    offs, _ = O.layout(numels)
    for o, n in zip(offs, numels):
        c0, nc = o // 256, -(-n // 256)
        lr[c0:c0 + nc], wd[c0:c0 + nc] = lr[c0], wd[c0]
    return lr, wd


MODES = [("norm", 2.0, False), ("norm", 1.0, True), ("norm", INF, True), ("full_model", 2.0, True), ("full_model", 1.0, False),
         ("full_model", INF, False), ("value", 2.0, True)]


@pytest.mark.parametrize("clip_type,norm_type,nesterov", MODES)
def test_restatement_is_torch(clip_type, norm_type, nesterov):
    """1. float64 restatement == clip_grad_norm_ + torch.optim.SGD(nesterov) in float64, three steps, 1e-12 relative;
    2. the fp32 emulation holds against it."""
    p, g, buf, lr, wd = O.bucket_inputs(NUMELS, 11)
    lr, wd = _per_param_const(NUMELS, lr, wd)
    gsteps = [g] + [O.bucket_inputs(NUMELS, 12 + s)[1] for s in range(2)]
    clip, gs, mom, ls = 3.0, 0.5, 0.9, 0.37
    pe, be = p, buf
    for step in range(3):
        # each step starts from the fp32 state the emulation left: the float64 statements are compared on the same tensors
        wp, wb, wn = _torch_steps(pe, [gsteps[step]], be, NUMELS, lr, wd, ls, mom, clip, gs, clip_type, norm_type, nesterov, torch.float64)[0]
        x = O.optim_step_ref(pe, gsteps[step], be, NUMELS, lr, wd, ls, mom, clip, gs, clip_type, norm_type, nesterov)
        for i in range(len(NUMELS)):
            for got, w in ((x["p"][i], wp[i]), (x["buf"][i], wb[i])):
                assert np.abs(got.v - w.numpy()).max() <= 1e-12 * max(1.0, float(w.abs().max())), (step, i)
                assert (got.m >= np.abs(got.v) * (1 - 1e-12)).all()          # float64 evaluation of m and v associates differently
        if clip_type == "norm":
            for i in range(len(NUMELS)):
                assert abs(float(x["norm"][i].v) - wn[i]) <= 1e-12 * wn[i], (step, i)
        elif clip_type == "full_model":
            assert abs(float(x["total"].v) - wn[0]) <= 1e-12 * wn[0], step
        e = O.optim_step_ref(pe, gsteps[step], be, NUMELS, lr, wd, ls, mom, clip, gs, clip_type, norm_type, nesterov, emulate=True)
        assert e["p_flat"].dtype == np.float32
        for i in range(len(NUMELS)):
            assert _ok(e["p"][i].v, x["p"][i]) and _ok(e["buf"][i].v, x["buf"][i]), (step, i)
            if clip_type != "value":
                assert _ok(e["norm"][i].v, x["norm"][i]) and _ok(e["coef"][i].v, x["coef"][i]), (step, i)
        if clip_type == "full_model":
            assert _ok(e["total"].v, x["total"])
        pe, be = torch.as_tensor(e["p_flat"]), torch.as_tensor(e["buf_flat"])


def _fault_case(fault):
    """Inputs on which the fault must show, with the mode it belongs to."""
    numels = list(NUMELS)
    p, g, buf, lr, wd = O.bucket_inputs(numels, 21, pad_fill=3.0)
    kw = dict(lr_scale=1.0, momentum=0.9, clip=0.5, grad_scale=0.5, clip_type="norm", norm_type=2.0, nesterov=False)
    if fault == "no_eps":                                                # a parameter whose norm is about 1e-5: 1e-6 is a tenth of it
        offs, _ = O.layout(numels)
        g[offs[2]:offs[2] + 256] = torch.randn(256, generator=torch.Generator().manual_seed(5)) * 1.25e-6
        kw["clip"] = 1e-6
    elif fault == "max_signed":                                          # the largest modulus of a parameter is negative
        offs, _ = O.layout(numels)
        g[offs[3] + 7] = -5e5
        kw["norm_type"] = INF
    elif fault == "nesterov_old_buf":
        kw["nesterov"] = True
    elif fault == "full_per_param":
        kw["clip_type"] = "full_model"
    return numels, p, g, buf, lr, wd, kw


@pytest.mark.parametrize("fault", O.FAULTS)
def test_faults_fail(fault):
    numels, p, g, buf, lr, wd, kw = _fault_case(fault)
    x = O.optim_step_ref(p, g, buf, numels, lr, wd, **kw)
    good = O.optim_step_ref(p, g, buf, numels, lr, wd, emulate=True, **kw)
    bad = O.optim_step_ref(p, g, buf, numels, lr, wd, emulate=True, fault=fault, **kw)
    assert all(_ok(good["p"][i].v, x["p"][i]) and _ok(good["buf"][i].v, x["buf"][i]) for i in range(len(numels)))
    assert not all(_ok(bad["p"][i].v, x["p"][i]) and _ok(bad["buf"][i].v, x["buf"][i]) for i in range(len(numels))), fault
    if fault not in ("no_coef", "nesterov_old_buf"):                     # the others are faults of the norm pass: coef shows them too
        assert not all(_ok(bad["coef"][i].v, x["coef"][i]) for i in range(len(numels))), fault


# ---- build_optimizer ------------------------------------------------------------------------------------------------------------------
class _Toy(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.backbone = torch.nn.Sequential(torch.nn.Linear(37, 300), torch.nn.ReLU(), torch.nn.Linear(300, 129))
        self.box_predictor = torch.nn.Linear(129, 5)

    def forward(self, x):
        return self.box_predictor(self.backbone(x)).square().sum() * 40.0


def _cfg(clip_type, norm_type, nesterov, momentum=0.9, clip=0.7):
    from fewx.config import get_cfg
    cfg = get_cfg()
    cfg.SOLVER.BASE_LR, cfg.SOLVER.MOMENTUM, cfg.SOLVER.NESTEROV = 0.01, momentum, nesterov
    cfg.SOLVER.CLIP_GRADIENTS.ENABLED, cfg.SOLVER.CLIP_GRADIENTS.CLIP_TYPE = True, clip_type
    cfg.SOLVER.CLIP_GRADIENTS.CLIP_VALUE, cfg.SOLVER.CLIP_GRADIENTS.NORM_TYPE = clip, norm_type
    return cfg


def emulation_apply(b, lr_factor, momentum, clip, scale, clip_type="value", norm_type=2.0, nesterov=False):
    """The CPU stand-in for the HIP launches (FlatSGD's apply_fn): the fp32 emulation over the bucket."""
    e = O.optim_step_ref(b.params, b.grads, b.momentum, b.numels, b.chunk_lr, b.chunk_wd, lr_factor, momentum, clip, scale, clip_type,
                         norm_type, nesterov, emulate=True)
    b.params.copy_(torch.as_tensor(e["p_flat"]))
    b.momentum.copy_(torch.as_tensor(e["buf_flat"]))


@pytest.mark.parametrize("clip_type,norm_type,nesterov", [("norm", 2.0, False), ("norm", 1.0, False), ("norm", INF, True),
                                                          ("full_model", 2.0, True), ("full_model", 1.0, False),
                                                          ("full_model", INF, False), ("value", 2.0, True)])
def test_build_optimizer_every_mode(clip_type, norm_type, nesterov):
    """build_optimizer(cfg) returns an optimizer for every CLIP_TYPE x NORM_TYPE and for NESTEROV; stepping it through an injected
    apply_fn reproduces clip_grad_norm_ / clip_grad_value_ + torch.optim.SGD.  (Before the norm clip and Nesterov were built both calls
    raised NotImplementedError.)"""
    from fewx.solver import build_optimizer, param_groups_like_reference
    cfg = _cfg(clip_type, norm_type, nesterov)
    torch.manual_seed(3)
    m, ref = _Toy(), _Toy()
    ref.load_state_dict(m.state_dict())
    groups = [{"params": [q], "lr": lr, "weight_decay": wd} for _, q, lr, wd in param_groups_like_reference(cfg, ref)]
    ropt = torch.optim.SGD(groups, cfg.SOLVER.BASE_LR, momentum=cfg.SOLVER.MOMENTUM, nesterov=nesterov)
    opt = build_optimizer(cfg, m)
    assert (opt.clip_type, opt.nesterov) == (clip_type, nesterov) and (clip_type == "value" or opt.norm_type == norm_type)
    opt._apply = emulation_apply
    assert set(opt.state_dict()) == {"momentum", "names", "lr_factor"}
    for step in range(3):
        x = torch.randn(6, 37, generator=torch.Generator().manual_seed(50 + step))
        for mod, o in ((m, opt), (ref, ropt)):
            o.zero_grad()
            mod(x).backward()
        rp = [q for g in ropt.param_groups for q in g["params"]]
        if clip_type == "norm":
            for q in rp:
                torch.nn.utils.clip_grad_norm_(q, cfg.SOLVER.CLIP_GRADIENTS.CLIP_VALUE, norm_type)
        elif clip_type == "full_model":
            torch.nn.utils.clip_grad_norm_(rp, cfg.SOLVER.CLIP_GRADIENTS.CLIP_VALUE, norm_type)
        else:
            torch.nn.utils.clip_grad_value_(rp, cfg.SOLVER.CLIP_GRADIENTS.CLIP_VALUE)
        ropt.step()
        opt.step()
        for (k, a), (_, b) in zip(m.state_dict().items(), ref.state_dict().items()):
            assert torch.allclose(a, b, rtol=2e-5, atol=2e-6), (step, k, float((a - b).abs().max()))


def test_build_optimizer_refusals():
    from fewx.solver import build_optimizer
    with pytest.raises(NotImplementedError, match="powf"):
        build_optimizer(_cfg("norm", 3.0, False), _Toy())
    with pytest.raises(ValueError, match="CLIP_TYPE"):
        build_optimizer(_cfg("median", 2.0, False), _Toy())
    with pytest.raises(ValueError, match="Nesterov"):
        build_optimizer(_cfg("value", 2.0, True, momentum=0.0), _Toy())
    with pytest.raises(ValueError):                                       # the words are torch.optim.SGD's
        torch.optim.SGD(_Toy().parameters(), lr=0.1, momentum=0.0, nesterov=True)


def test_value_form_keeps_its_five_positional_arguments():
    """Value clipping without Nesterov calls apply_fn exactly as before: five positional arguments, no keyword."""
    from fewx.solver import build_optimizer
    seen = []
    opt = build_optimizer(_cfg("value", 2.0, False), _Toy())
    opt._apply = lambda *a, **k: seen.append((len(a), k))
    opt.step()
    assert seen == [(5, {})]


# ---- special values ---------------------------------------------------------------------------------------------------------------------
def _special(kind, clip_type):
    numels = [300, 5, 257]
    p, g, buf, lr, wd = O.bucket_inputs(numels, 31)
    g = g * 1e-3
    lr, wd = _per_param_const(numels, lr, wd)
    offs, _ = O.layout(numels)
    if kind == "nan":
        g[offs[1] + 2] = float("nan")
    elif kind == "inf":
        g[offs[1] + 2] = -INF
    elif kind == "zero":
        g[offs[1]:offs[1] + 5] = 0.0
    elif kind == "overflow":
        g[offs[1] + 2] = 1e30                                           # its square overflows fp32
    return numels, offs, p, g, buf, lr, wd


@pytest.mark.parametrize("clip_type", ["norm", "full_model"])
@pytest.mark.parametrize("kind", ["nan", "inf", "zero", "overflow"])
def test_special_values_follow_torch(kind, clip_type):
    """The table of special values: the fp32 emulation against clip_grad_norm_ + torch.optim.SGD of the installed torch in fp32."""
    numels, offs, p, g, buf, lr, wd = _special(kind, clip_type)
    e = O.optim_step_ref(p, g, buf, numels, lr, wd, 1.0, 0.9, 0.5, 1.0, clip_type, 2.0, False, emulate=True)
    tp, tb, tn = _torch_steps(p, [g], buf, numels, lr, wd, 1.0, 0.9, 0.5, 1.0, clip_type, 2.0, False, torch.float32)[0]
    hit = [1] if clip_type == "norm" else [0, 1, 2]
    nrm = float(e["norm"][1].v) if clip_type == "norm" else float(e["total"].v)
    c = float(e["coef"][1].v)
    if kind == "nan":
        assert math.isnan(nrm) and math.isnan(c) and math.isnan(tn[1 if clip_type == "norm" else 0])
    elif kind in ("inf", "overflow"):
        assert nrm == INF and c == 0.0 and tn[1 if clip_type == "norm" else 0] == INF
    else:
        assert float(e["norm"][1].v) == 0.0 and (clip_type == "full_model" or c == 1.0)
    for i in range(3):
        ep, eb = e["p"][i].v, e["buf"][i].v
        assert np.array_equal(np.isnan(ep), torch.isnan(tp[i]).numpy()) and np.array_equal(np.isnan(eb), torch.isnan(tb[i]).numpy()), i
        ok = ~np.isnan(ep)
        assert np.allclose(ep[ok], tp[i].numpy()[ok], rtol=1e-5, atol=1e-7) and np.allclose(eb[~np.isnan(eb)], tb[i].numpy()[~np.isnan(eb)], rtol=1e-5, atol=1e-7)
        if kind == "nan":
            assert np.isnan(ep).all() == (i in hit) and np.isnan(ep).any() == (i in hit)
        elif kind == "inf":
            n_nan = int(np.isnan(ep).sum())
            assert n_nan == (1 if i == 1 else 0)                           # 0 * inf; everything else of S takes the weight-decay step only
            if i in hit:
                keep = ~np.isnan(eb)
                o, n = offs[i], numels[i]
                wdv, pv, bv = wd[o // 256].numpy(), p[o:o + n].numpy(), buf[o:o + n].numpy()
                assert np.array_equal(eb[keep], (np.float32(0.9) * bv + (np.float32(0) + wdv * pv))[keep])
        else:
            assert not np.isnan(ep).any() and not np.isnan(eb).any()


# ---- coverage -----------------------------------------------------------------------------------------------------------------------------
def test_every_optim_kernel_is_in_the_table():
    with open(os.path.join(PKG, "csrc", "ore_optim.hip")) as f:
        src = f.read()
    names = set(re.findall(r"__global__.*?void\s+(\w+)\s*\(", src))
    assert names == set(O.KERNELS), names ^ set(O.KERNELS)
    with open(os.path.join(os.path.dirname(__file__), "test_hip_optim.py")) as f:
        tests = f.read()
    for k, (entry, test) in O.KERNELS.items():
        assert ("def " + test + "(") in tests and entry in src, (k, test)
    assert int(re.search(r"constexpr int GN_G = (\d+);", src)[1]) == O.GN_G and int(re.search(r"constexpr int GN_W = (\d+);", src)[1]) == O.GN_W
