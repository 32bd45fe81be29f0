"""float64 restatement and fp32 emulation of csrc/ore_optim.hip: the gradient norms of the flat bucket, the clip coefficients and the
SGD update with or without Nesterov momentum (torch.nn.utils.clip_grad_norm_ + torch.optim.SGD).

    g^ = grad_scale g;  norm = ||g^ over S||_p, p in {2, 1, inf};  coef = min(clip / (norm + 1e-6), 1);  g' = g^ coef
    g' += wd p;  buf = momentum buf + g';  p -= lr (g' + momentum buf)  [Nesterov]   or   p -= lr buf
S is one parameter (clip_type "norm") or every parameter of the bucket ("full_model"); "value" is the clamp of k_sgd_step.

Bounds: the running-error number X = (v, m, d) and the two checks of tests/trainloss_ref.py (`hold`).  Charges:
  * fp32 inputs and the fp32 scalars (clip, grad_scale, momentum, 1e-6 as the kernel's constant 1e-6f) are exact at input;
  * + - * / cost one rounding each; sqrtf one (ore_optim.hip is compiled like ore_train.hip: -O3 -ffp-contract=off and nothing that
    relaxes division or sqrt; trainloss_ref measured 0.5 ULP for both);
  * a sum of n terms is charged the chain depth of the kernels, read off csrc/ore_optim.hip (GN_G, GN_W and the block sizes are restated
    below; tests/test_hip_optim.py compares them with the library's own answer, ore_grad_norm_geometry):
        d_param_sum(numel)   GN_G thread chain + 6 butterfly + 3 waves in order  (k_grad_norm_partial)
                             + ceil(parts / GN_W) lane chain + 6 butterfly        (k_grad_norm_param),  parts = ceil(ceil(numel / 256) / GN_G)
        d_total_sum(numels)  max over parameters of the above + ceil(P / 256) + 6 + 3   (k_grad_norm_total)
  * clamp(max = 1) and max |.| are selections: no rounding; min(1, r) is continuous in r, so the restatement needs no margin from
    r = 1 (whichever side fp32 lands on, the value differs from the float64 one by the error of r at most).
Per-parameter results carry their own depth, so they are returned as one X per parameter, never as one array with the deepest d.

fp32 emulation (emulate=True): numpy float32 in the kernels' order; the kernels must equal it bit for bit, NaN and Inf included.

Test infrastructure (used by tests/ only)."""
import numpy as np

import trainloss_ref as TL
from trainloss_ref import F32, F64, X, _cdiv, _np, xwhere

GN_G = 16            # csrc/ore_optim.hip: chunks of 256 floats per partial
GN_W = 64            # partials one pass of the per-parameter wave takes
GN_T = 256           # threads of k_grad_norm_total
CHUNK = 256
FAULTS = ("no_coef", "segment", "padding", "no_scale_norm", "no_eps", "max_signed", "nesterov_old_buf", "full_per_param")

# kernel of csrc/ore_optim.hip -> the entry point that launches it and the test of tests/test_hip_optim.py that holds it
KERNELS = {
    "k_grad_norm_partial": ("ore_grad_norm_fwd", "test_grad_norms"),
    "k_grad_norm_param": ("ore_grad_norm_fwd", "test_grad_norms"),
    "k_grad_norm_total": ("ore_grad_norm_fwd", "test_grad_norms"),
    "k_sgd_step_norm": ("ore_sgd_step_clipnorm_fwd", "test_three_steps"),
}


def layout(numels):
    """(offsets, size) of parameters padded to whole chunks, as fewx.solver.FlatBucket lays them out."""
    offs, o = [], 0
    for n in numels:
        offs.append(o)
        o += _cdiv(n, CHUNK) * CHUNK
    return offs, o


def n_parts(numel):
    return _cdiv(_cdiv(numel, CHUNK), GN_G)


def d_param_sum(numel):
    return GN_G + 6 + 3 + _cdiv(n_parts(numel), GN_W) + 6


def d_total_sum(numels):
    return max(d_param_sum(n) for n in numels) + _cdiv(len(numels), GN_T) + 6 + 3


# ---- the kernels' summation order, in the dtype of the terms -----------------------------------------------------------------------
def _join(a, b, mx):
    if not mx:
        return a + b
    with np.errstate(invalid="ignore"):
        return np.where((b > a) | np.isnan(b), b, a)


def _butterfly(v, mx):
    for d in (32, 16, 8, 4, 2, 1):
        v = _join(v, v[..., np.arange(64) ^ d], mx)
    return v[..., 0]


def _waves(w, mx):
    return _join(_join(_join(w[..., 0], w[..., 1], mx), w[..., 2], mx), w[..., 3], mx)


def _param_acc_order(terms, mx):
    """k_grad_norm_partial + k_grad_norm_param over the terms of one parameter (elements beyond numel are not in `terms`: a skipped
    join leaves the accumulator, which is what joining a +0 does to a sum of non-negative terms or a maximum that started at 0)."""
    n = len(terms)
    parts = n_parts(n)
    pad = np.zeros(parts * GN_G * CHUNK, dtype=terms.dtype)
    pad[:n] = terms
    t = pad.reshape(parts, GN_G // 4, 256, 4)
    acc = np.zeros((parts, 256), dtype=terms.dtype)
    for j in range(GN_G // 4):
        for c in range(4):
            acc = _join(acc, t[:, j, :, c], mx)
    partial = _waves(_butterfly(acc.reshape(parts, 4, 64), mx), mx)                       # [parts]
    pp = np.zeros(_cdiv(parts, GN_W) * GN_W, dtype=terms.dtype)
    pp[:parts] = partial
    lanes = np.zeros(GN_W, dtype=terms.dtype)
    for row in pp.reshape(-1, GN_W):
        lanes = _join(lanes, row, mx)
    return _butterfly(lanes, mx)


def _total_order(accs, mx):
    """k_grad_norm_total over the per-parameter sums (maxima)."""
    P = len(accs)
    pad = np.zeros(_cdiv(P, GN_T) * GN_T, dtype=accs.dtype)
    pad[:P] = accs
    th = np.zeros(GN_T, dtype=accs.dtype)
    for row in pad.reshape(-1, GN_T):
        th = _join(th, row, mx)
    return _waves(_butterfly(th.reshape(4, 64), mx), mx)


def _sqrt(a):
    with np.errstate(invalid="ignore", divide="ignore"):
        v = np.sqrt(a.v)
        m = np.where(np.asarray(a.v) > 0, np.maximum(np.abs(v).astype(F64), a.m / (2.0 * np.abs(v).astype(F64))), 0.0)
    return X(v, m, a.d + 1)


def _scalar(v, t):
    return X(np.asarray(F32(v), dtype=t))


# ---- the norms ------------------------------------------------------------------------------------------------------------------------
def grad_norms_ref(g, numels, clip=1.0, grad_scale=1.0, norm_type=2.0, full_model=False, emulate=False, fault=None):
    """ore_grad_norm_fwd over the bucket `g` (padding included, laid out by `layout(numels)`) ->
    dict(acc, norm, coef: one scalar X per parameter; total: scalar X, full model only).  coef is the coefficient the update of that
    parameter uses.  fault: see optim_step_ref."""
    t = F32 if emulate else F64
    g = _np(g).astype(F32)
    offs, size = layout(numels)
    assert g.size == size, (g.size, size)
    mx, l2 = norm_type == float("inf"), norm_type == 2.0
    assert mx or l2 or norm_type == 1.0, norm_type
    gs = _scalar(1.0 if fault == "no_scale_norm" else grad_scale, t)
    accs = []
    for i, (o, n) in enumerate(zip(offs, numels)):
        take = _cdiv(n, CHUNK) * CHUNK if fault == "padding" else n
        el = g[o:o + take]
        if fault == "segment" and i + 1 < len(numels):                  # the run goes one chunk too far: into the neighbour
            el = np.concatenate([el, g[offs[i + 1]:offs[i + 1] + min(numels[i + 1], CHUNK)]])
        with np.errstate(over="ignore", invalid="ignore"):
            gh = X(el.astype(t)) * gs
            term = gh * gh if l2 else (gh if (mx and fault == "max_signed") else gh.abs())
            if emulate:
                acc = X(_param_acc_order(term.v, mx), None, term.d + (0 if mx else d_param_sum(len(el))))
            elif mx:
                k = int(np.argmax(term.v)) if not np.isnan(term.v).any() else int(np.argmax(np.isnan(term.v)))
                acc = X(np.maximum(term.v[k], 0.0) if fault == "max_signed" else term.v[k], term.m[k], term.d)
            else:
                acc = term.sum(d_param_sum(len(el)))
        accs.append(acc)
    norms = [_sqrt(a) if l2 else a for a in accs]
    eps = _scalar(1e-6, t)
    cl = _scalar(clip, t)
    one = _scalar(1.0, t)

    def coef_of(nrm):
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            r = cl / (nrm if fault == "no_eps" else nrm + eps)
            return xwhere(r.v > one.v, one, r)
    out = {"acc": accs, "norm": norms, "total": None}
    if full_model:
        av = np.array([a.v for a in accs], dtype=t)
        with np.errstate(over="ignore", invalid="ignore"):
            if emulate:
                tot = X(_total_order(av, mx), None, max(a.d for a in accs) + (0 if mx else _cdiv(len(numels), GN_T) + 9))
            elif mx:
                k = int(np.argmax(av)) if not np.isnan(av).any() else int(np.argmax(np.isnan(av)))
                tot = accs[k]
            else:
                tot = X(av.sum(), sum(float(a.m) for a in accs), accs[0].d - d_param_sum(numels[0]) + d_total_sum(numels))
        out["total"] = _sqrt(tot) if l2 else tot
        out["coef"] = [coef_of(nrm) for nrm in norms] if fault == "full_per_param" else [coef_of(out["total"])] * len(numels)
    else:
        out["coef"] = [coef_of(nrm) for nrm in norms]
    return out


# ---- the step -------------------------------------------------------------------------------------------------------------------------
def optim_step_ref(p, g, buf, numels, chunk_lr, chunk_wd, lr_scale=1.0, momentum=0.9, clip=1.0, grad_scale=1.0, clip_type="norm",
                   norm_type=2.0, nesterov=False, emulate=False, fault=None):
    """FlatSGD.step in a norm mode or with Nesterov momentum over the bucket (p, g, buf with padding; chunk_lr / chunk_wd per chunk) ->
    dict(p, buf: one X per parameter over its numel elements; norm, coef, acc, total as grad_norms_ref; p_flat, buf_flat: the whole
    bucket after the step, padding untouched).  emulate: numpy float32 in the kernels' order.
    fault -- what a kernel of this shape can get wrong:
        "no_coef"           the coefficient is not applied
        "segment"           a segment boundary is one chunk off: the norm takes in the neighbour's first chunk
        "padding"           the padding of the last chunk is in the norm
        "no_scale_norm"     grad_scale is missing from the norm but present in the update
        "no_eps"            the 1e-6 is omitted
        "max_signed"        the maximum is taken without the modulus
        "nesterov_old_buf"  the Nesterov look-ahead uses the momentum buffer from before the step
        "full_per_param"    full-model mode uses per-parameter coefficients"""
    assert fault is None or fault in FAULTS, fault
    t = F32 if emulate else F64
    p32, g32, b32 = (_np(a).astype(F32) for a in (p, g, buf))
    offs, size = layout(numels)
    out = {"norm": None, "coef": None, "acc": None, "total": None}
    if clip_type != "value":
        out.update(grad_norms_ref(g32, numels, clip, grad_scale, norm_type, clip_type == "full_model", emulate, fault))
    clr, cwd = _np(chunk_lr).astype(F32), _np(chunk_wd).astype(F32)
    mom, gs, cl, ls = (_scalar(v, t) for v in (momentum, grad_scale, clip, lr_scale))
    pf, bf = p32.astype(t), b32.astype(t)
    out["p"], out["buf"] = [], []
    for i, (o, n) in enumerate(zip(offs, numels)):
        c0, nc = o // CHUNK, _cdiv(n, CHUNK)
        lr = X(np.repeat(clr[c0:c0 + nc], CHUNK)[:n].astype(t)) * ls
        wd = X(np.repeat(cwd[c0:c0 + nc], CHUNK)[:n].astype(t))
        P, G, Bf = X(p32[o:o + n].astype(t)), X(g32[o:o + n].astype(t)), X(b32[o:o + n].astype(t))
        with np.errstate(invalid="ignore", over="ignore"):
            gi = G * gs
            if clip_type != "value":
                if fault != "no_coef":
                    c = out["coef"][i]
                    gi = gi * X(np.broadcast_to(c.v, gi.v.shape), np.broadcast_to(c.m, gi.v.shape), c.d)
            elif clip > 0:
                gi = xwhere(gi.v > cl.v, cl, xwhere(gi.v < -cl.v, -cl, gi))
            gi = gi + wd * P
            b = mom * Bf + gi
            if nesterov:
                newp = P - lr * (gi + mom * (Bf if fault == "nesterov_old_buf" else b))
            else:
                newp = P - lr * b
        out["p"].append(newp); out["buf"].append(b)
        pf[o:o + n], bf[o:o + n] = newp.v, b.v
    out["p_flat"], out["buf_flat"] = pf, bf
    return out


# ---- the bucket of the GPU tests ---------------------------------------------------------------------------------------------------------
def bucket_numels(small=6):
    """1, 255, 256, 257, 256 G, 256 G + 1, 256 G W + 1 and `small` more single-chunk parameters: with the first three, more single-chunk
    parameters than one block of k_grad_norm_param (four waves, four parameters) serves."""
    return [1, 255, 256, 257, 256 * GN_G, 256 * GN_G + 1, 256 * GN_G * GN_W + 1] + [3 + 40 * k for k in range(small)]


def bucket_inputs(numels, seed, pad_fill=None):
    """(p, g, buf [size], chunk_lr, chunk_wd [chunks]) fp32 torch tensors: gradients over six decades (10^-2 .. 10^4 times a normal
    draw, as _sgd_inputs of tests/test_hip_trainloss.py draws them), parameters over three, lr and wd changing with the chunk; the
    padding of g holds pad_fill (None: 0)."""
    import torch
    offs, size = layout(numels)
    gen = torch.Generator().manual_seed(seed)
    p = (torch.randn(size, generator=gen) * 10.0 ** (torch.rand(size, generator=gen) * 3 - 2)).float()
    g = (torch.randn(size, generator=gen) * 10.0 ** (torch.rand(size, generator=gen) * 6 - 2)).float()
    buf = (torch.randn(size, generator=gen) * 0.1).float()
    chunks = size // CHUNK
    lr = (torch.rand(chunks, generator=gen) * 0.1 + 1e-3).float()
    wd = torch.where(torch.arange(chunks) % 3 == 0, torch.zeros(chunks), torch.rand(chunks, generator=gen) * 1e-2).float()
    for o, n in zip(offs, numels):
        e = o + _cdiv(n, CHUNK) * CHUNK
        p[o + n:e], buf[o + n:e] = 0.0, 0.0
        g[o + n:e] = 0.0 if pad_fill is None else pad_fill
    return p, g, buf, lr, wd


hold = TL.hold
