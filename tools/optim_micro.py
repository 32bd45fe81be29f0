#!/usr/bin/env python3
"""Norm pass, update and a device copy of the gradient bucket of finetune_vovnet.yaml, launched in loops on one stream.

    python tools/optim_micro.py                                   # host-side time per call (event timed; launch-bound)
    ITERS=20 rocprofv3 --kernel-trace --stats -- python tools/optim_micro.py   # kernel times: what profiles/optim_bench.json quotes
Prints one JSON line."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "faster-orefsdet_amd"))
import torch
from fewx.config import get_cfg
from detectron2.modeling import build_model
from fewx.solver import build_optimizer
import orehip

cfg = get_cfg()
cfg.merge_from_file(os.path.join(ROOT, "faster-orefsdet_amd", "configs", "fsod", "finetune_vovnet.yaml"))
cfg.merge_from_list(["MODEL.DEVICE", "cuda"])
cfg.SOLVER.CLIP_GRADIENTS.CLIP_TYPE = "full_model"
torch.manual_seed(0)
m = build_model(cfg).train()
opt = build_optimizer(cfg, m)
b = opt.bucket
b.grads.normal_()
tmp = torch.empty_like(b.grads)
ws = opt._norm_ws
N = int(os.environ.get("ITERS", "200"))

def timed(fn):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(N):
        fn()
    e1.record(); torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / N          # us per call

res = {"bucket_floats": b.size, "parameters": len(b.numels), "partials": ws["n_parts"], "iters": N}
for rep in range(3):
    r = {}
    r["copy_us"] = timed(lambda: tmp.copy_(b.grads))
    r["norm_per_param_us"] = timed(lambda: orehip.grad_norms(b.grads, b.param_numel, b.param_chunk0, ws, 2.0, False, 1.0, 1.0))
    r["norm_full_model_us"] = timed(lambda: orehip.grad_norms(b.grads, b.param_numel, b.param_chunk0, ws, 2.0, True, 1.0, 1.0))
    r["norm_inf_us"] = timed(lambda: orehip.grad_norms(b.grads, b.param_numel, b.param_chunk0, ws, float("inf"), False, 1.0, 1.0))
    r["update_value_us"] = timed(lambda: orehip.sgd_step(b.params, b.grads, b.momentum, b.chunk_lr, b.chunk_wd, 0.0, 0.9, 1.0, 1.0))
    r["update_norm_us"] = timed(lambda: orehip.sgd_step_norm(b.params, b.grads, b.momentum, b.chunk_lr, b.chunk_wd, b.chunk_param, b.param_numel,
                                                             b.param_chunk0, ws["coef"], 0.0, 0.9, 1.0, 1.0, True))
    r["empty_launch_us"] = timed(lambda: orehip.sgd_step_norm(b.params[:256], b.grads[:256], b.momentum[:256], b.chunk_lr[:1], b.chunk_wd[:1],
                                                              b.chunk_param[:1], b.param_numel, b.param_chunk0, ws["coef"], 0.0, 0.9, 1.0, 1.0, True))
    by = 4.0 * b.size
    r["copy_GBps_read"] = by / r["copy_us"] / 1e3
    r["norm_per_param_GBps"] = by / r["norm_per_param_us"] / 1e3
    res["rep%d" % rep] = r
print(json.dumps(res))
