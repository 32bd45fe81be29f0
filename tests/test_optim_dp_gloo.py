"""CPU: two gloo ranks run the flat-bucket gradient exchange + full-model 2-norm clip + SGD and must land on the parameters a single
process gets from clip_grad_norm_ over all parameters + torch.optim.SGD on the rank-averaged gradients (what DDP computes): the norm
is that of the AVERAGED gradient (grad_scale = 1 / world is inside the norm).  Modelled on tests/test_train_dp_gloo.py."""
import os
import sys

import torch
import torch.multiprocessing as mp

from test_train_dp_gloo import ROOT, _Toy, _cfg, _data, _free_port

CLIP = 50.0          # below the norm of the averaged gradient (asserted), above it for none of the three steps


def _norm_cfg():
    cfg = _cfg()
    cfg.SOLVER.CLIP_GRADIENTS.CLIP_TYPE, cfg.SOLVER.CLIP_GRADIENTS.CLIP_VALUE, cfg.SOLVER.CLIP_GRADIENTS.NORM_TYPE = "full_model", CLIP, 2.0
    return cfg


def _emulation_apply(b, lr_factor, momentum, clip, scale, clip_type="value", norm_type=2.0, nesterov=False):
    """CPU test: the update comes from the fp32 emulation of the kernels (tests/optim_ref.py); the product path is the HIP launches."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import optim_ref as O
    e = O.optim_step_ref(b.params, b.grads, b.momentum, b.numels, b.chunk_lr, b.chunk_wd, lr_factor, momentum, clip, scale, clip_type,
                         norm_type, nesterov, emulate=True)
    b.params.copy_(torch.as_tensor(e["p_flat"]))
    b.momentum.copy_(torch.as_tensor(e["buf_flat"]))
    b.seen_norms = getattr(b, "seen_norms", []) + [float(e["total"].v)]
    assert (clip_type, norm_type, nesterov) == ("full_model", 2.0, False)


def _worker(rank, world, port, q, steps):
    sys.path.insert(0, os.path.join(ROOT, "faster-orefsdet_amd"))
    import torch.distributed as dist
    from fewx.solver import FlatDataParallel, build_lr_scheduler, build_optimizer
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.manual_seed(7 + rank)
        cfg = _norm_cfg()
        model = FlatDataParallel(_Toy(), cfg, overlap=True)
        opt = build_optimizer(cfg, model)
        opt._apply = _emulation_apply
        sched = build_lr_scheduler(cfg, opt)
        for s in range(steps):
            loss = model(_data(rank, s))
            opt.zero_grad()
            loss.backward()
            opt.step()
            sched.step()
        sd = {k: v.detach().numpy().copy() for k, v in model.module.state_dict().items()}
        q.put((rank, sd, model.bucket.seen_norms))
    finally:
        dist.destroy_process_group()


def _single_process_reference(world, steps):
    sys.path.insert(0, os.path.join(ROOT, "faster-orefsdet_amd"))
    from fewx.solver import param_groups_like_reference, warmup_factor_at_iter
    torch.manual_seed(7)
    cfg = _norm_cfg()
    m = _Toy()
    groups = [{"params": [p], "lr": lr, "weight_decay": wd} for _, p, lr, wd in param_groups_like_reference(cfg, m)]
    opt = torch.optim.SGD(groups, cfg.SOLVER.BASE_LR, momentum=cfg.SOLVER.MOMENTUM)
    base = [g["lr"] for g in opt.param_groups]
    norms = []
    for s in range(steps):
        f = warmup_factor_at_iter("linear", s, cfg.SOLVER.WARMUP_ITERS, cfg.SOLVER.WARMUP_FACTOR) * \
            cfg.SOLVER.GAMMA ** sum(1 for ms in cfg.SOLVER.STEPS if ms <= s)
        for g, b in zip(opt.param_groups, base):
            g["lr"] = b * f
        opt.zero_grad(set_to_none=True)
        loss = sum(m(_data(r, s)) for r in range(world)) / world          # DDP: mean of the per-rank gradients
        loss.backward()
        live = [p for g in opt.param_groups for p in g["params"] if p.grad is not None]
        norms.append(float(torch.nn.utils.clip_grad_norm_(live, CLIP, 2.0)))
        opt.step()
    return m.state_dict(), norms


def test_two_rank_full_model_norm_clip_matches_ddp_semantics():
    world, steps, port = 2, 3, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_worker, args=(r, world, port, q, steps)) for r in range(world)]
    for p in ps:
        p.start()
    res = sorted((q.get(timeout=180) for _ in range(world)), key=lambda t: t[0])
    for p in ps:
        p.join(60)
        assert p.exitcode == 0
    (_, sd0, n0), (_, sd1, n1) = res
    ref, want_norms = _single_process_reference(world, steps)
    assert all(n > CLIP for n in want_norms), want_norms                  # the clip bites: a norm of the SUMMED gradient would be twice this
    assert n0 == n1 and all(abs(a - b) <= 1e-5 * b for a, b in zip(n0, want_norms)), (n0, want_norms)
    for k in ref:
        a, b = torch.from_numpy(sd0[k]), torch.from_numpy(sd1[k])
        assert torch.equal(a, b), k                                       # ranks stay bit-identical
        assert torch.allclose(a, ref[k], rtol=2e-5, atol=2e-6), (k, (a - ref[k]).abs().max())
