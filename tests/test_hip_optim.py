"""The kernels of csrc/ore_optim.hip (gradient norms of the flat bucket, clip coefficients, SGD update with or without Nesterov
momentum) against float64 and the fp32 emulation of tests/optim_ref.py; tests/test_optim_host.py shows on the CPU that the restatement
is clip_grad_norm_ + torch.optim.SGD, that the emulation passes and that the faults such kernels can have fail.

Every launch runs twice and is compared bit for bit; every floating output is held to |got - ref| <= 2 d u mag per element and to the
block rms bound (trainloss_ref.hold) and equals the emulation bit for bit; outputs start NaN-filled.  The bucket has parameters of 1,
255, 256, 257, 256 G, 256 G + 1 and 256 G W + 1 elements (G chunks per partial, W partials per pass) and more single-chunk parameters
than one block of the per-parameter kernel serves."""
import math

import numpy as np
import pytest
import torch

import optim_ref as O
import trainloss_ref as TL

pytestmark = pytest.mark.gpu

DEV = "cuda"
INF = float("inf")
NUMELS = O.bucket_numels()
GS = 0.5
CLIPS = {2.0: 2e4, 1.0: 2e4, INF: 2e3}          # between the norms of the small and of the large parameters of the bucket


@pytest.fixture(scope="module")
def oh():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import orehip
    orehip.lib()
    assert orehip.grad_norm_geometry() == (O.GN_G, O.GN_W), "tests/optim_ref.py restates other constants than csrc/ore_optim.hip has"
    return orehip


@pytest.fixture(scope="module")
def bucket(oh):
    """The shared inputs (never modified: every test clones what it steps) and the device tables of the bucket."""
    offs, size = O.layout(NUMELS)
    p, g, buf, lr, wd = O.bucket_inputs(NUMELS, 7, pad_fill=1e30)
    g2 = [O.bucket_inputs(NUMELS, 8 + s, pad_fill=1e30)[1] for s in range(2)]
    tab = {"chunk_param": torch.tensor([i for i, n in enumerate(NUMELS) for _ in range(-(-n // 256))], dtype=torch.int32, device=DEV),
           "numel": torch.tensor(NUMELS, dtype=torch.int64, device=DEV),
           "chunk0": torch.tensor([o // 256 for o in offs], dtype=torch.int64, device=DEV),
           "ws": oh.grad_norm_workspace(NUMELS, DEV)}
    assert tab["ws"]["n_chunks"] * 256 == size and tab["ws"]["n_parts"] == sum(O.n_parts(n) for n in NUMELS)
    return {"p": p, "g": [g] + g2, "buf": buf, "lr": lr, "wd": wd, "lr_d": lr.to(DEV), "wd_d": wd.to(DEV), "offs": offs, "size": size, **tab}


def _hold(name, got, x, what):
    h, r = TL.hold(got, x)
    print(f"{name} {what}: hard {h:.3e} rms {r:.3e} d {x.d}")
    assert h <= 1 and r <= 1, (name, what, {"hard": h, "rms": r, "d": x.d})


def _bits(t):
    return t.contiguous().view(torch.int32)


def _twice(fn):
    a, b = fn(), fn()
    for x, y in zip(a, b):
        assert torch.equal(_bits(x), _bits(y)), "two identical launches differ"
    return a


def _same_bits(got, want):
    g = got.detach().cpu().numpy().reshape(-1)
    w = np.asarray(want, dtype=np.float32).reshape(-1)
    nan = np.isnan(w)
    return np.array_equal(np.isnan(g), nan) and np.array_equal(g[~nan].view(np.int32), w[~nan].view(np.int32))


def _stack(xs):
    return np.array([np.asarray(x.v).reshape(()) for x in xs], dtype=np.float32)


def _run_norms(oh, bk, g_dev, norm_type, full_model, clip, gs=GS):
    ws = bk["ws"]
    for k in ("partial", "acc", "norm", "coef", "total"):
        ws[k].fill_(float("nan"))
    n, c, t = oh.grad_norms(g_dev, bk["numel"], bk["chunk0"], ws, norm_type, full_model, clip, gs)
    return n.clone(), c.clone(), t.clone()


def _check_norms(got, ref_e, ref_x, full_model, what):
    n, c, t = got
    assert _same_bits(n, _stack(ref_e["norm"])) and _same_bits(c, _stack(ref_e["coef"])), (what, "differs from the fp32 emulation")
    for i in range(len(NUMELS)):
        _hold("grad_norm norm", n[i:i + 1], ref_x["norm"][i], (what, NUMELS[i]))
        _hold("grad_norm coef", c[i:i + 1], ref_x["coef"][i], (what, NUMELS[i]))
    if full_model:
        assert _same_bits(t, np.asarray(ref_e["total"].v))
        _hold("grad_norm total", t, ref_x["total"], what)
    else:
        assert bool(torch.isnan(t).all())                                   # total is the full-model output only


# ---- 1. the norm pass alone ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("full_model", [False, True])
@pytest.mark.parametrize("norm_type", [2.0, 1.0, INF])
def test_grad_norms(oh, bucket, norm_type, full_model):
    """Norms, coefficients and (full model) the total; the padding holds 1e30 and is in no norm."""
    g = bucket["g"][0]
    gd = g.to(DEV)
    clip = CLIPS[norm_type]
    got = _twice(lambda: _run_norms(oh, bucket, gd, norm_type, full_model, clip))
    e = O.grad_norms_ref(g, NUMELS, clip, GS, norm_type, full_model, emulate=True)
    x = O.grad_norms_ref(g, NUMELS, clip, GS, norm_type, full_model)
    assert all(np.isfinite(v.v) for v in x["norm"]) and float(max(v.v for v in x["norm"])) < 1e12      # no 1e30 got in
    if not full_model:
        cs = _stack(e["coef"])
        assert (cs == 1.0).any() and (cs < 1.0).any()
    _check_norms(got, e, x, full_model, (norm_type, full_model))
    # the same gradients with a clean padding give the same bits: the padding moved nothing
    g0 = g.clone()
    for o, n in zip(bucket["offs"], NUMELS):
        g0[o + n:o + -(-n // 256) * 256] = 0.0
    again = _run_norms(oh, bucket, g0.to(DEV), norm_type, full_model, clip)
    for a, b in zip(got[:2], again[:2]):
        assert torch.equal(_bits(a), _bits(b))


# ---- 2. three consecutive steps ----------------------------------------------------------------------------------------------------------
def _step(oh, bk, pd, gd, bd, clip_type, norm_type, nesterov, clip, scale, sd, momentum=0.9, gs=GS):
    coef, got = None, None
    if clip_type != "value":
        got = _run_norms(oh, bk, gd, norm_type, clip_type == "full_model", clip, gs)
        coef = bk["ws"]["coef"]
    oh.sgd_step_norm(pd, gd, bd, bk["lr_d"], bk["wd_d"], bk["chunk_param"], bk["numel"], bk["chunk0"], coef,
                     lr_scale=(123.0 if sd is not None else scale), momentum=momentum, clip_value=clip, grad_scale=gs, nesterov=nesterov,
                     lr_scale_dev=sd)
    return got


STEP_CASES = [(ct, nt, nes, False, CLIPS[nt]) for ct, nt in (("norm", 2.0), ("norm", INF), ("full_model", 2.0), ("full_model", 1.0))
              for nes in (False, True)] + [
    ("value", 2.0, True, False, 1.0),            # value clip + Nesterov: the new update kernel without a norm pass
    ("norm", 2.0, True, True, 2e4),              # the LR factor comes from the device
    ("norm", 1.0, False, False, 1e12),           # every coefficient is 1
    ("full_model", INF, True, False, 1e-3),      # every coefficient bites
]


@pytest.mark.parametrize("clip_type,norm_type,nesterov,dev_scale,clip", STEP_CASES)
def test_three_steps(oh, bucket, clip_type, norm_type, nesterov, dev_scale, clip):
    """Three consecutive steps on the bucket of test_grad_norms, each bit-equal to the emulation and within the float64 bound."""
    scale = 0.37
    sd = torch.tensor([scale], device=DEV) if dev_scale else None
    p, buf = bucket["p"], bucket["buf"]
    for step in range(3):
        g = bucket["g"][step]
        gd = g.to(DEV)

        def run():
            pd, bd = p.to(DEV).clone(), buf.to(DEV).clone()
            nrm = _step(oh, bucket, pd, gd, bd, clip_type, norm_type, nesterov, clip, scale, sd)
            return (pd, bd) + (tuple(nrm[:2]) if nrm is not None else ())
        out = _twice(run)
        pd, bd = out[0], out[1]
        args = (p, g, buf, NUMELS, bucket["lr"], bucket["wd"], scale, 0.9, clip, GS, clip_type, norm_type, nesterov)
        e = O.optim_step_ref(*args, emulate=True)
        x = O.optim_step_ref(*args)
        assert _same_bits(pd, e["p_flat"]) and _same_bits(bd, e["buf_flat"]), (step, "differs from the fp32 emulation")
        if clip_type != "value":
            cs = _stack(e["coef"])
            assert _same_bits(out[3], cs)
            if clip == 1e12:
                assert (cs == 1.0).all()
            if clip == 1e-3:
                assert (cs < 1.0).all()
        for i, (o, n) in enumerate(zip(bucket["offs"], NUMELS)):
            assert np.isfinite(x["p"][i].v).all() and np.isfinite(x["buf"][i].v).all()
            _hold("step p", pd[o:o + n], x["p"][i], (clip_type, norm_type, nesterov, step, n))
            _hold("step buf", bd[o:o + n], x["buf"][i], (clip_type, norm_type, nesterov, step, n))
        p, buf = pd.cpu(), bd.cpu()


# ---- 3. special values --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip_type", ["norm", "full_model"])
@pytest.mark.parametrize("kind", ["nan", "inf", "zero", "overflow"])
def test_special_values(oh, bucket, kind, clip_type):
    """A NaN element: norm and coefficient NaN, every element of S NaN.  A +-Inf element: norm inf, coefficient 0, that element NaN
    (0 * inf), the rest of S takes the weight-decay step only.  An all-zero gradient: norm 0, coefficient 1, no NaN.  Squares that
    overflow fp32: norm inf.  Per-parameter mode: every other parameter is bit-equal to the emulation, so none of it leaks."""
    tgt = 3                                                              # the 257-element parameter: two chunks, one padded
    o, n = bucket["offs"][tgt], NUMELS[tgt]
    g = bucket["g"][0].clone() * 1e-3
    if kind == "nan":
        g[o + 256] = float("nan")
    elif kind == "inf":
        g[o + 256] = -INF
    elif kind == "zero":
        g[o:o + n] = 0.0
    else:
        g[o + 5] = 1e30
    gd = g.to(DEV)
    p, buf = bucket["p"], bucket["buf"]

    def run():
        pd, bd = p.to(DEV).clone(), buf.to(DEV).clone()
        nrm = _step(oh, bucket, pd, gd, bd, clip_type, 2.0, False, 0.5, 1.0, None, gs=1.0)
        return (pd, bd) + tuple(nrm)
    pd, bd, nrm, coef, total = _twice(run)
    e = O.optim_step_ref(p, g, buf, NUMELS, bucket["lr"], bucket["wd"], 1.0, 0.9, 0.5, 1.0, clip_type, 2.0, False, emulate=True)
    assert _same_bits(pd, e["p_flat"]) and _same_bits(bd, e["buf_flat"]) and _same_bits(nrm, _stack(e["norm"])) and _same_bits(coef, _stack(e["coef"]))
    full = clip_type == "full_model"
    S = torch.zeros(bucket["size"], dtype=torch.bool)
    for i, (oo, nn) in enumerate(zip(bucket["offs"], NUMELS)):
        if full or i == tgt:
            S[oo:oo + nn] = True
    nv, cv = float(total if full else nrm[tgt]), float(coef[tgt])
    pn, bn = torch.isnan(pd.cpu()), torch.isnan(bd.cpu())
    if kind == "nan":
        assert math.isnan(nv) and math.isnan(cv)
        assert torch.equal(pn, S) and torch.equal(bn, S)                    # all of S, nothing else, no padding
    elif kind in ("inf", "overflow"):
        assert nv == INF and cv == 0.0
        if kind == "inf":
            one = torch.zeros_like(S)
            one[o + 256] = True
            assert torch.equal(pn, one) and torch.equal(bn, one)
        else:
            assert not pn.any() and not bn.any()
        rest = S & ~pn
        want = np.float32(0.9) * buf.numpy() + (np.float32(0) + np.repeat(bucket["wd"].numpy(), 256) * p.numpy())
        assert np.array_equal(bd.cpu().numpy()[rest.numpy()], want[rest.numpy()])     # a gradient of +-0: the weight-decay step only
    else:
        assert float(nrm[tgt]) == 0.0 and (full or cv == 1.0) and not pn.any() and not bn.any()


# ---- 4. against torch on the device's result -------------------------------------------------------------------------------------------------
def _flat_model(shapes, lrs, wds, seed):
    import torch.nn as nn
    from fewx.solver.build import FlatBucket
    torch.manual_seed(seed)
    cpu_p = [nn.Parameter(torch.randn(*s)) for s in shapes]
    gpu_p = [nn.Parameter(q.detach().clone().cuda()) for q in cpu_p]
    b = FlatBucket([("p%d" % i, q, lr, wd) for i, (q, lr, wd) in enumerate(zip(gpu_p, lrs, wds))], n_slices=2, min_slice_bytes=1024)
    return cpu_p, b


@pytest.mark.parametrize("nesterov", [False, True])
@pytest.mark.parametrize("clip_type,norm_type", [("norm", 2.0), ("full_model", 2.0), ("norm", INF)])
def test_step_matches_torch_optim(oh, clip_type, norm_type, nesterov):
    """FlatSGD in the norm modes == clip_grad_norm_ + torch.optim.SGD(momentum, per-group lr / weight decay, nesterov) over 3 steps."""
    from fewx.solver.build import FlatSGD
    shapes = [(300, 37), (300,), (5, 129), (129, 3, 3, 3), (1,)]
    lrs, wds = [0.01, 0.01, 0.02, 0.01, 0.02], [1e-4, 0.0, 1e-4, 1e-2, 1e-4]
    cpu_p, bucket = _flat_model(shapes, lrs, wds, 3)
    ref = torch.optim.SGD([{"params": [q], "lr": lr, "weight_decay": wd} for q, lr, wd in zip(cpu_p, lrs, wds)], 0.01, momentum=0.9,
                          nesterov=nesterov)
    clip = 20.0                                                          # bites for the large parameters, not for the small ones
    opt = FlatSGD(bucket, 0.01, 0.9, clip, nesterov=nesterov, clip_type=clip_type, norm_type=norm_type)
    by_name = dict(zip(bucket.names, bucket.tensors))
    for step in range(3):
        f = [0.5, 1.0, 0.1][step]
        opt.set_lr_factor(f)
        for g, lr in zip(ref.param_groups, lrs):
            g["lr"] = lr * f
        opt.zero_grad()
        for i, q in enumerate(cpu_p):
            gr = torch.randn(q.shape) * 3.0
            q.grad = gr.clone()
            by_name["p%d" % i].grad.add_(2.0 * gr.cuda())                # "sum over 2 ranks", averaged by grad_scale
        bucket.grad_scale = 0.5
        if clip_type == "norm":
            norms = [float(torch.nn.utils.clip_grad_norm_(q, clip, norm_type)) for q in cpu_p]
        else:
            norms = [float(torch.nn.utils.clip_grad_norm_(cpu_p, clip, norm_type))]
        ref.step()
        opt.step()
        for i, q in enumerate(cpu_p):
            got = by_name["p%d" % i].detach().cpu()
            assert (got - q.detach()).abs().max() <= 2e-7 * max(1.0, float(q.detach().abs().max())), (step, i)
        gn = opt.grad_norm_dev
        if clip_type == "norm":
            want = torch.tensor([norms[int(n[1:])] for n in bucket.names])
            assert torch.allclose(gn["norm"].cpu(), want, rtol=1e-5)
        else:
            assert abs(float(gn["total"]) - norms[0]) <= 1e-5 * norms[0]
    assert float(bucket.params[bucket.offsets[bucket.names.index("p1")] + 300:bucket.offsets[bucket.names.index("p1")] + 512].abs().max()) == 0.0


# ---- 6. grad_norm_dev ---------------------------------------------------------------------------------------------------------------------
def test_grad_norm_dev_is_the_norm_of_the_bucket_gradients(oh, bucket):
    """After a full-model step, FlatSGD.grad_norm_dev holds the float64 norms of bucket.grads over each parameter's first numel
    elements (grad_scale folded in), within the bound of the reduction."""
    from fewx.solver.build import FlatSGD
    shapes = [(n,) for n in NUMELS]
    cpu_p, b = _flat_model(shapes, [0.01] * len(NUMELS), [1e-4] * len(NUMELS), 5)
    order = [int(n[1:]) for n in b.names]
    numels = [NUMELS[i] for i in order]
    opt = FlatSGD(b, 0.01, 0.9, 1.0, nesterov=True, clip_type="full_model", norm_type=2.0)
    opt.zero_grad()
    b.grads.copy_(O.bucket_inputs(numels, 9, pad_fill=1e30)[1].to(DEV))     # what backward and the exchange left, padding poisoned
    b.grad_scale = 0.5
    g = b.grads.detach().cpu()
    opt.step()
    x = O.grad_norms_ref(g, numels, 1.0, 0.5, 2.0, True)
    gn = opt.grad_norm_dev
    for i in range(len(numels)):
        _hold("grad_norm_dev norm", gn["norm"][i:i + 1], x["norm"][i], numels[i])
    _hold("grad_norm_dev total", gn["total"], x["total"], "total")
    want = math.sqrt(sum(float((g[o:o + n].double() * 0.5).square().sum()) for o, n in zip(b.offsets, b.numels)))
    assert abs(float(x["total"].v) - want) <= 1e-12 * want
    assert set(opt.state_dict()) == {"momentum", "names", "lr_factor"}


# ---- 5. the whole step, captured ------------------------------------------------------------------------------------------------------------
def test_whole_step_graph_matches_eager_full_model_nesterov(oh, monkeypatch):
    """tests/test_hip_train.py::test_whole_step_graph_matches_eager with CLIP_TYPE full_model, NESTEROV and a CLIP_VALUE below the
    gradient norm: three eager + three replayed iterations give the parameters of six eager ones (the same bars), so the norm pass
    and the update are capturable and nothing in step() reads the device."""
    from oracle import ref_train as T
    from detectron2.structures import Boxes, Instances
    from fewx.solver import GraphedTrainStep, build_optimizer
    from test_hip_train import _train_model
    shots, B = 4, 2
    items = []
    for b in range(B):
        img, gt, sup, sbox = T.synth_train_inputs(2 + b, (256, 320), n_gt=5 + b, shots=shots, support_hw=96)
        inst = Instances((256, 320))
        inst.gt_boxes, inst.gt_classes = Boxes(gt.cuda()), torch.zeros(len(gt), dtype=torch.int64).cuda()
        items.append({"image": img.cuda(), "instances": inst, "support_images": sup.cuda(), "support_bboxes": sbox.cuda()})
    keys = torch.rand(B, 16384, generator=torch.Generator().manual_seed(3)).cuda()
    real_rand = torch.rand

    def fixed_rand(*shape, **kw):                           # the fg / bg subsample draws its keys here: the same for both runs
        if len(shape) == 2 and kw.get("device") is not None and torch.device(kw["device"]).type == "cuda":
            return keys[:shape[0], :shape[1]].clone()
        return real_rand(*shape, **kw)

    monkeypatch.setattr(torch, "rand", fixed_rand)
    clip = 1.0
    res = {}
    for mode in ("eager", "graph"):
        m, sd, cfg = _train_model(shots)
        cfg.defrost()
        cfg.SOLVER.CLIP_GRADIENTS.ENABLED, cfg.SOLVER.CLIP_GRADIENTS.CLIP_TYPE = True, "full_model"
        cfg.SOLVER.CLIP_GRADIENTS.CLIP_VALUE, cfg.SOLVER.CLIP_GRADIENTS.NORM_TYPE, cfg.SOLVER.NESTEROV = clip, 2.0, True
        opt = build_optimizer(cfg, m)
        assert opt.clip_type == "full_model" and opt.nesterov
        stepper = GraphedTrainStep(m, opt, warmup=3) if mode == "graph" else None
        losses_log, totals = [], []
        for it in range(6):
            opt.set_lr_factor(0.02 * (1.0 + 0.25 * it))     # a schedule that moves every iteration
            if stepper is not None:
                losses = stepper(items)
            else:
                losses = m(items)
                opt.zero_grad()
                sum(losses.values()).backward()
                opt.step()
            losses_log.append({k: float(v.detach()) for k, v in losses.items()})
            totals.append(float(opt.grad_norm_dev["total"]))
        torch.cuda.synchronize()
        if stepper is not None:
            assert stepper.error is None, stepper.error
            assert stepper.eager_steps == 3 and stepper.replays == 3
        print(mode, "gradient norms", totals)
        assert all(t > clip for t in totals), totals        # the clip bites at every step
        res[mode] = (losses_log, opt.bucket.params.detach().clone(), opt.bucket.momentum.detach().clone(), totals)
    for it in range(6):
        for k, v in res["eager"][0][it].items():
            assert abs(v - res["graph"][0][it][k]) <= 1e-5 * max(abs(v), 1e-3), (it, k, v, res["graph"][0][it][k])
    pe, pg = res["eager"][1], res["graph"][1]
    assert float((pe - pg).abs().max()) <= 1e-6 * float(pe.abs().max()), float((pe - pg).abs().max())
    assert float((res["eager"][2] - res["graph"][2]).abs().max()) <= 1e-5 * float(res["eager"][2].abs().max())
