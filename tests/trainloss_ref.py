"""float64 restatements of the nine kernels of csrc/ore_train.hip (CenterNet targets, loss sums and loss gradient, the second stage's
two losses, ROI sampling, the fused clip + SGD step), their chain depths, and the operands the tests feed them.

Bounds.  As in tests/trainops_ref.py every floating output is held to the two checks of dgrad_ref.check with u = 2^-24, C_S = 1:
    every element                     |got - ref| <= 2 d u mag
    every 16-row x 16-channel block   rms((got - ref) / mag) <= C_S u sqrt(d)
Integer outputs, and floating outputs that are a copy, a selection or an exactly representable value, are compared exactly.

Running-error form.  The loss kernels are not sums of products: a rounded intermediate goes through 1 - x, a division, logf, powf and
expf.  Every restatement here is therefore written ONCE, over the small number class X = (v, m, d):
    v   the float64 value;
    m   its magnitude: first-order  |fl(v) - v| <= d u m  for the fp32 evaluation in the kernel's order;
    d   the number of roundings charged along the longest chain behind it (a Python int: the same for every element of an array).
An fp32 input is exact: (x, |x|, 0).  The rules (a, b operands; every rule keeps m >= |v|):
    a + b, a - b   (va +- vb,  ma + mb,                        max(da, db) + 1)   sums of moduli: the cancelling steps 1 - pred,
                                                                                    ta + pa - ai, ac - au, 1 - (iou - ...) are these
    a * b          (va vb,     ma mb,                           da + db + 1)
    a / b          (va / vb,   (ma / |vb|) (mb / |vb|),         da + db + 1)       mb / |vb| >= 1: the condition number of 1 / b
    f(a)           (f(va),     max(|f(va)|, |f'(va)| ma),       da + c_f)          f in expf, logf, powf(., e): the relative bound so
                                                                                    far times the condition number va f' / f of the step
    min, max, select   the selected operand's (v, m); d = the larger one; no rounding (fminf / fmaxf / ?: return an operand)
    -a, |a|, a * 2^k   no rounding
Induction on the rules gives the first-order bound; the factor 2 of the hard check covers the second-order terms ((1 + u)^d - 1 <=
2 d u, and the curvature of f over an interval of relative width d u m / |v| << 1).  A product, quotient or expf whose value is
below the smallest normal fp32 number is charged against FLT_MIN = 2^-126 instead (m >= 2^-126 after these steps: the device may
flush or round denormals; expf(-100) is such a value) -- an absolute allowance of 2 d u 2^-126 ~ 1e-43 d, nothing a loss can see.
A sum of n such terms in a chain of depth r has (sum v, sum m, d_term + r).

Roundings charged to the library functions (c_f above, in units of u: a function within K ULP has relative error <= 2 K u, so
c_f = 2 K).  Division and sqrtf: csrc/Makefile compiles ore_train.hip with -O3 -ffp-contract=off and nothing that relaxes them
(hipcc's default is correctly rounded fp32 division and sqrt), so they cost 1 like + - *; tools/ulp_probe.hip confirms 0.5 ULP.
ROCm on the build machine ships no HIP math-API accuracy table, so expf / logf / powf were measured ONCE on the MI355X against
double with tools/ulp_probe.hip (4 M arguments per sweep, the arguments these kernels see) and are charged TWICE the worst error
seen, rounded up to an integer number of ULPs:
    function   arguments swept                                          worst seen (ULP)   charged K   c_f = 2 K
    expf       [-87, 88], [-20, 20], [-1, 0]                            0.8389             2           4
    logf       [1e-5, 16] log-uniform, [0.5, 2], [0.99, 1.01]           1.8831             4           8
    powf       x in [0, 1] and [1e-5, 1] log-uniform, e in {1, 2, 4}    1.3185             3           6
               (gamma = 2, gamma - 1 = 1, beta = 4)
The figures are the constants ULP_MEASURED below.  They never come from a kernel of ore_train.hip agreeing with itself.

Chain depths of the reductions (read off the kernels):
  d_cn_sum(rows)      k_cn_loss_partial: nb = min(ceil(rows / 256), 256) blocks; a thread adds ceil(rows / (nb * 256)) terms in one
                      chain, 6 butterfly steps over the wave, (r0 + r1) + (r2 + r3) (2); k_cn_loss_final: lane chains over
                      ceil(nb / 64) partials, 6 butterfly steps.  d = term + ceil(rows / (nb 256)) + 6 + 2 + ceil(nb / 64) + 6.
  d_cn_pos(np)        k_cn_loss_final: lane chains over ceil(np / 64) positives, 6 butterfly steps.
  d_roi_sum(RT)       k_roi_losses: a thread adds ceil(RT / 256) terms, then 8 tree steps over LDS.
  the loss gradient   elementwise: the depth is the d of the expression; column 4 takes one more addition per entry of pos_inds that
                      names the row (atomicAdd; equal addends, so the order cannot matter and the result is reproducible).
  k_sgd_step          elementwise; it is ALSO reproduced bit for bit by sgd_step_ref(emulate=True): numpy float32 in the kernel's
                      operation order (-ffp-contract=off: every operation rounds once; the clip is a selection).

Headroom of the heat map.  On the MI355X the worst 16-location block of hm_targets reaches 0.99 of the rms bound (0.23 of the element
bound).  The rms bound models independent roundings, but r2 = max(delta2x2 * area, min_radius2) is ONE rounded number per object: its
two roundings move -d2 / r2 the same way at every location the object owns, so a block inside one object's Gaussian sees them as a
common offset of up to 2 u |d2 / r2| (|d2 / r2| up to ln 1e4 = 9.2), not as noise.  The element bound charges them in full and is
the rigorous one; the rms figure has no slack left against a ROCm whose expf is less accurate than the 0.84 ULP measured, and a
failure of it alone on this output should first be read against that.

Discrete decisions.  Every decision is evaluated in float64 on the fp32 inputs; a generator keeps a relative margin from every
discontinuity that sits behind ROUNDED quantities and re-draws from the next seed what misses it (never drops an input; REDRAWS counts
them).  A comparison between two fp32 INPUTS (pred against target in the GIoU gradient, max(target) >= 0, key against key) is exact in
either arithmetic and needs no margin.  Hand-written cases sit exactly on the discontinuities with values for which fp32 is exact.
    in_box > 0, centre 3x3         l, t, r, b, ddx, ddy are exact for boxes on the 1/8 px grid: exact comparisons, no margin; cases with a
                                   box side on a grid centre (in_box false at 0) and |ddx| == stride (inside)
    size of interest               crit = sqrt(sw^2 + sh^2) / 2 against soi: margin CN_MARGIN, and 3-4-5 boxes ON the limits
                                   (48 x 64 -> 40, 96 x 128 -> 80: sums of squares and sqrtf are exact)
    arg-min owner                  smallest against second-smallest eligible distance: margin CN_MARGIN, or an exact tie (identical
                                   boxes, or two objects whose discretised centre is this location: both distances are the literal 0):
                                   the first one wins
    heat-map cut 1e-4              | hmin - ln 1e4 | >= HM_MARGIN * ln 1e4 (1e-5 relative) at every location
    inside the sigmoid clamp       | s - clamp | and | s - (1 - clamp) | relative margin S_MARGIN; exact case: clamp = 0.5 and logit 0,
    pred < ignore_high_fp          where s = pred = 0.5 exactly = ignore_high_fp
    IoU >= thr, first maximum      margin IOU_MARGIN on |iou - thr| and between the best and second-best ground truth, or an exact
                                   tie (identical ground-truth boxes / all IoUs 0)
    sign(deltas - target)          |df| >= twice its own error bound 2 d u m, or the row with boxes == gt and deltas == 0 (df = 0 - 0)

NOT_REACHED (deliberately outside this file): see the dict of that name at the end.

Test infrastructure (used by tests/ only)."""
import math

import numpy as np
import torch

import inferops_ref as IR
import trainops_ref as TR
from trainops_ref import C_S, U, _cdiv, check2  # noqa: F401  (re-exported)

F64 = np.float64
F32 = np.float32
FLT_MIN = 2.0 ** -126

# worst error seen by tools/ulp_probe.hip on the MI355X, in ULPs of the fp32 result (one run, 4 M arguments per sweep)
ULP_MEASURED = {
    "expf": 0.8389,                                   # at 1.646 ([-87, 88]); 0.8334 on [-20, 20], 0.8367 on [-1, 0]
    "logf": 1.8831,                                   # at 4.8e-4; 1.7939 on [0.5, 2], 1.7517 on [0.99, 1.01]
    "powf": 1.3185,                                   # e = 4 at 0.0304; 1.2997 for e = 2, 1.0000 for e = 1
    "sigmoid": 2.5647,                                # 1 / (1 + expf(-x)) on [-20, 20], for the record: 2 K_EXP + 2 roundings cover it
    "sqrtf": 0.5,
    "div": 0.5,
}
K_EXP, K_LOG, K_POW = 2, 4, 3                         # charged: twice the worst seen, rounded up to an integer
C_EXP, C_LOG, C_POW = 2 * K_EXP, 2 * K_LOG, 2 * K_POW

CN_INF = 100000000.0
CN_MARGIN, HM_MARGIN, S_MARGIN, IOU_MARGIN = 1e-4, 1e-5, 2e-5, 1e-5
LN_1E4 = math.log(1e4)
REDRAWS = {}                                          # generator -> [inputs drawn, inputs re-drawn]


def _count(name, drawn, redrawn):
    a = REDRAWS.setdefault(name, [0, 0])
    a[0] += int(drawn); a[1] += int(redrawn)


# ---- the running-error number ----------------------------------------------------------------------------------------------------
class X:
    """(v, m, d) as the module docstring defines them.  v is float64, or float32 in an emulation (every operation then rounds once,
    numpy's float32 arithmetic being correctly rounded; m is not meaningful then)."""
    __slots__ = ("v", "m", "d")

    def __init__(self, v, m=None, d=0):
        self.v = np.asarray(v)
        self.m = np.abs(self.v).astype(F64) if m is None else m
        self.d = d

    def _c(self, o):
        return o if isinstance(o, X) else X(np.asarray(o, dtype=self.v.dtype))

    def __add__(self, o):
        o = self._c(o)
        return X(self.v + o.v, self.m + o.m, max(self.d, o.d) + 1)

    __radd__ = __add__

    def __sub__(self, o):
        o = self._c(o)
        return X(self.v - o.v, self.m + o.m, max(self.d, o.d) + 1)

    def __rsub__(self, o):
        return self._c(o) - self

    def __neg__(self):
        return X(-self.v, self.m, self.d)

    def __mul__(self, o):
        o = self._c(o)
        with np.errstate(over="ignore", invalid="ignore"):
            return X(self.v * o.v, np.maximum(self.m * o.m, FLT_MIN), self.d + o.d + 1)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = self._c(o)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            b = np.abs(o.v).astype(F64)
            return X(self.v / o.v, np.maximum(self.m / b * (o.m / b), FLT_MIN), self.d + o.d + 1)

    def __rtruediv__(self, o):
        return self._c(o) / self

    def scale2(self, k):
        """* 2^k: exact."""
        return X(self.v * self.v.dtype.type(2.0 ** k), self.m * 2.0 ** k, self.d)

    def abs(self):
        return X(np.abs(self.v), self.m, self.d)

    def exp(self):
        with np.errstate(over="ignore", under="ignore"):
            f = np.exp(self.v)
            fa = np.abs(f).astype(F64)
            return X(f, np.maximum(fa * np.maximum(1.0, self.m) if self.d else fa, FLT_MIN), self.d + C_EXP)

    def log(self):
        with np.errstate(divide="ignore", invalid="ignore"):
            f = np.log(self.v)
            return X(f, np.maximum(np.abs(f).astype(F64), self.m / np.abs(self.v).astype(F64)), self.d + C_LOG)

    def powc(self, e):
        """powf(., e) for a constant e >= 1 and a base >= 0."""
        t = self.v.dtype.type
        with np.errstate(invalid="ignore"):
            f = np.power(self.v, t(e))
            fp = abs(e) * np.power(np.abs(self.v).astype(F64), e - 1.0)
            return X(f, np.maximum(np.maximum(np.abs(f).astype(F64), fp * self.m), 0.0), self.d + C_POW)

    def sum(self, chain):
        """All elements as one reduction whose longest chain has `chain` additions."""
        return X(self.v.astype(F64).sum(), self.m.sum(), self.d + chain)


def xwhere(mask, a, b):
    a = a if isinstance(a, X) else b._c(a)
    b = b if isinstance(b, X) else a._c(b)
    return X(np.where(mask, a.v, b.v), np.where(mask, a.m, b.m), max(a.d, b.d))


def xmin(a, b):
    return xwhere(a.v <= b.v, a, b)


def xmax(a, b):
    return xwhere(a.v >= b.v, a, b)


def _np(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def _xin(t, emulate):
    a = _np(t).astype(F32)
    return X(a if emulate else a.astype(F64))


def to_t(a, device="cpu"):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device)


def hold(got, x, extra_d=0):
    """(hard ratio, rms ratio) of got against the X `x` (a scalar X is one element)."""
    ref = torch.as_tensor(np.asarray(x.v, dtype=F64))
    mag = torch.as_tensor(np.asarray(x.m, dtype=F64))
    if ref.dim() == 0:
        ref, mag = ref.reshape(1, 1), mag.reshape(1, 1)
    elif ref.dim() == 1:
        ref, mag = ref.reshape(-1, 1), mag.reshape(-1, 1)
    return check2(got.detach().cpu().reshape(ref.shape), ref, mag, max(x.d + extra_d, 1))


# ---- chain depths ----------------------------------------------------------------------------------------------------------------
def cn_loss_blocks(rows):
    return min(_cdiv(rows, 256), 256)


def d_cn_sum(rows):
    nb = cn_loss_blocks(rows)
    return _cdiv(rows, nb * 256) + 6 + 2 + _cdiv(nb, 64) + 6


def d_cn_pos(npos):
    return _cdiv(max(npos, 1), 64) + 6


def d_roi_sum(RT):
    return _cdiv(RT, 256) + 8


# ---- fused clip + SGD ----------------------------------------------------------------------------------------------------------------
def sgd_step_ref(p, g, buf, chunk_lr, chunk_wd, lr_scale=1.0, momentum=0.9, clip=1.0, grad_scale=1.0, emulate=False, fault=None):
    """ore_sgd_step_fwd: torch.nn.utils.clip_grad_value_ then torch.optim.SGD.step over 256-element chunks,
        g' = clamp(grad_scale g, -clip, clip) (clip > 0; a NaN stays a NaN, like torch.clamp);  g' += wd p;  buf = momentum buf + g';
        p -= lr buf,   lr = chunk_lr * lr_scale
    -> (p, buf) as X.  emulate: numpy float32 in the kernel's operation order, which the kernel must equal bit for bit.
    fault (tests/test_trainloss_host.py): "wd_first": weight decay before the clip; "lr_next": lr of the neighbouring chunk."""
    t = F32 if emulate else F64
    P, G, Bf = _xin(p, emulate), _xin(g, emulate), _xin(buf, emulate)
    clr = _np(chunk_lr).astype(F32)
    if fault == "lr_next":
        clr = np.roll(clr, -1)
    lr = X(np.repeat(clr, 256).astype(t)) * X(np.asarray(F32(lr_scale), dtype=t))
    wd = X(np.repeat(_np(chunk_wd).astype(F32), 256).astype(t))
    mom, gs, cl = (X(np.asarray(F32(v), dtype=t)) for v in (momentum, grad_scale, clip))

    def clamp(x):
        if not clip > 0:
            return x
        with np.errstate(invalid="ignore"):
            return xwhere(x.v > cl.v, cl, xwhere(x.v < -cl.v, -cl, x))
    gi = G * gs
    if fault == "wd_first":
        gi = clamp(gi + wd * P)
    else:
        gi = clamp(gi) + wd * P
    b = mom * Bf + gi
    return P - lr * b, b


# ---- the second stage's two losses -------------------------------------------------------------------------------------------------
def roi_losses_ref(scores, deltas, boxes, gt, labels, valid, B, R, reg_weights, emulate=False, fault=None):
    """ore_roi_losses_fwd (see csrc/ore_train.hip): w_i = valid_i / (n_b B), n_b = max(#valid rows of image b, 1);
        loss_cls = sum w_i (logsumexp(s_i) - s_i[label_i]);  dscores = w_i (softmax(s_i) - onehot(label_i))
        loss_box = sum_{valid fg} w_i sum_k |d_ik - tgt_ik|;  ddeltas = w_i sign(d_ik - tgt_ik)   (0 off the foreground)
    -> dict(loss_cls, loss_box: scalar X; dscores: X [RT,2]; ddeltas: exact float32 [RT,4]; df_margin: min over foreground elements
    with df != 0 of |df| / (2 d u m), which the inputs keep >= 2).
    fault: "no_B": w = 1 / n_b;  "count_invalid": invalid rows weigh like valid ones."""
    t = F32 if emulate else F64
    RT = B * R
    lab = _np(labels).reshape(RT)
    v = _np(valid).reshape(RT).astype(bool)
    nb = np.maximum(v.reshape(B, R).sum(1), 1).astype(F32)
    den = nb if fault == "no_B" else nb * F32(B)                              # exact: small integers
    w_img = X(np.asarray(1.0, dtype=t)) / X(den.astype(t))
    w32 = np.repeat(F32(1.0) / den, R)                                         # the kernel's own fp32 weight (correctly rounded)
    vv = np.ones_like(v) if fault == "count_invalid" else v
    w = xwhere(vv, X(np.repeat(w_img.v, R), np.repeat(w_img.m, R), w_img.d), 0.0)
    w32 = np.where(vv, w32, F32(0))
    s = _xin(scores, emulate)
    s0, s1 = X(s.v[:, 0]), X(s.v[:, 1])
    m = xmax(s0, s1)
    e0, e1 = (s0 - m).exp(), (s1 - m).exp()
    se = e0 + e1
    lse = m + se.log()
    is0 = lab == 0
    lc_t = w * (lse - xwhere(is0, s0, s1))
    lc = lc_t.sum(d_roi_sum(RT))
    one, zero = np.asarray(1.0, dtype=t), np.asarray(0.0, dtype=t)
    d0 = w * (e0 / se - xwhere(is0, X(one), X(zero)))
    d1 = w * (e1 / se - xwhere(is0, X(zero), X(one)))
    ds = X(np.stack([d0.v, d1.v], 1), np.stack([d0.m, d1.m], 1), max(d0.d, d1.d))
    fg = vv & is0
    bx, g, dl = _xin(boxes, emulate), _xin(gt, emulate), _xin(deltas, emulate)
    col = lambda a, k: X(a.v[:, k])                                            # noqa: E731
    sw, sh = col(bx, 2) - col(bx, 0), col(bx, 3) - col(bx, 1)
    sx, sy = col(bx, 0) + sw.scale2(-1), col(bx, 1) + sh.scale2(-1)
    tw, th = col(g, 2) - col(g, 0), col(g, 3) - col(g, 1)
    tx, ty = col(g, 0) + tw.scale2(-1), col(g, 1) + th.scale2(-1)
    rw = [X(np.asarray(F32(r), dtype=t)) for r in reg_weights]
    with np.errstate(divide="ignore", invalid="ignore"):
        tgt = [rw[0] * (tx - sx) / sw, rw[1] * (ty - sy) / sh, rw[2] * (tw / sw).log(), rw[3] * (th / sh).log()]
    acc, sign, margin, row_margin = None, [], math.inf, np.full(RT, np.inf)
    for k in range(4):
        df = col(dl, k) - tgt[k]
        a = xwhere(fg, df.abs(), 0.0)
        acc = a if acc is None else acc + a
        sign.append(np.where(fg, np.sign(df.v), 0.0))
        nz = fg & (df.v != 0)
        if nz.any():
            row_margin[nz] = np.minimum(row_margin[nz], np.abs(df.v[nz]) / (2 * df.d * U * df.m[nz]))
            margin = float(row_margin.min())
    acc.d += 1                                                                 # the kernel's chain starts with 0 + |df_0|
    lb_t = w * acc
    lb = lb_t.sum(d_roi_sum(RT))
    dd = (np.stack(sign, 1).astype(F32) * w32[:, None]).astype(F32)
    return dict(loss_cls=lc, loss_box=lb, dscores=ds, ddeltas=dd, df_margin=margin, row_margin=row_margin, loss_cls_terms=lc_t.v,
                loss_box_terms=lb_t.v)


def roi_loss_inputs(B, R, seed, device="cpu", mode=None):
    """(scores [RT,2], deltas, boxes, gt [RT,4], labels [RT] int64, valid [RT] bool) fp32: score pairs with per-row scales 1e-3..1e3
    and gaps of exactly +-100 on some rows; boxes inside a 640 px image, gt = the box jittered; per image a random valid prefix and
    foreground share.  Fixed rows: image 0 has rows with boxes == gt and deltas == 0 (target and gradient exactly 0).  mode: "edges" makes
    the first three images (as far as B goes) one with no valid row, one with no foreground, one all valid foreground.  Rows whose
    sign(deltas - target) has less than twice its error bound are re-drawn from the next seed."""
    RT = B * R
    s = seed
    rng = np.random.default_rng(s)
    sc = 10.0 ** rng.uniform(-3, 3, (RT, 1))
    scores = (rng.standard_normal((RT, 2)) * sc).astype(F32)
    k = np.arange(RT)
    scores[k % 7 == 3] = np.array([50.0, -50.0], dtype=F32)               # gaps of +-100
    scores[k % 7 == 5] = np.array([-37.0, 63.0], dtype=F32)
    wh = np.exp(rng.uniform(math.log(8.0), math.log(300.0), (RT, 2)))
    xy = rng.uniform(0, 1, (RT, 2)) * (640.0 - wh)
    boxes = np.concatenate([xy, xy + wh], 1).astype(F32)
    jit = rng.uniform(-0.2, 0.2, (RT, 4)) * np.concatenate([wh, wh], 1)
    gt = (boxes + jit).astype(F32)
    deltas = (rng.standard_normal((RT, 4)) * 10.0 ** rng.uniform(-2, 1, (RT, 1))).astype(F32)
    labels = (rng.uniform(0, 1, RT) < 0.7).astype(np.int64)                # 1 = background
    nv = rng.integers(1, R + 1, B)
    valid = (np.arange(R)[None, :] < nv[:, None]).reshape(RT)
    if mode == "edges":
        if B > 0:
            valid[:R] = False
        if B > 1:
            labels[R:2 * R] = 1
        if B > 2:
            labels[2 * R:3 * R] = 0; valid[2 * R:3 * R] = True
    z = np.arange(min(3, R))
    if mode != "edges":
        gt[z] = boxes[z]; deltas[z] = 0.0; labels[z] = 0; valid[z] = True
    elif B > 2:
        zz = 2 * R + z
        gt[zz] = boxes[zz]; deltas[zz] = 0.0
    redrawn = 0
    while True:
        bad = roi_losses_ref(scores, deltas, boxes, gt, labels, valid, B, R, (10.0, 10.0, 5.0, 5.0))["row_margin"] < 2.0
        if not bad.any():
            break
        s += 1000003
        redrawn += int(bad.sum())
        r2 = np.random.default_rng(s)
        deltas[bad] = (r2.standard_normal((int(bad.sum()), 4)) * 10.0 ** r2.uniform(-2, 1, (int(bad.sum()), 1))).astype(F32)
    _count("roi_loss_inputs", RT, redrawn)
    dev = device
    return (to_t(scores, dev), to_t(deltas, dev), to_t(boxes, dev), to_t(gt, dev), to_t(labels, dev), to_t(valid, dev))


# ---- CenterNet losses ------------------------------------------------------------------------------------------------------------------
def _cn_common(head, reg_targets, hm_targets, clamp, ignore_high_fp, emulate):
    t = F32 if emulate else F64
    h = _np(head).astype(F32)[:, :5]
    h = np.where(np.isnan(h), F32(0), h)
    H = h.astype(t)
    T = _np(reg_targets).astype(F32).astype(t)
    hm = X(_np(hm_targets).astype(F32).astype(t))
    reg = T.max(1) >= 0
    lo, hi = F32(clamp), F32(1.0) - F32(clamp)                                 # the kernel's own fp32 constants: exact operands
    with np.errstate(over="ignore"):
        s = 1.0 / (1.0 + (-X(H[:, 4])).exp())
    s64 = 1.0 / (1.0 + np.exp(-h[:, 4].astype(F64)))
    inside = (s64 >= F64(lo)) & (s64 <= F64(hi))
    pred = xwhere(s64 < F64(lo), X(np.asarray(lo, dtype=t)), xwhere(s64 > F64(hi), X(np.asarray(hi, dtype=t)), s))
    p64 = np.clip(s64, F64(lo), F64(hi))
    ign = (ignore_high_fp > 0) & ~(p64 < F64(F32(ignore_high_fp)))
    return t, H, T, hm, reg, s, inside, pred, ign, s64, p64, lo, hi


def cn_margins(head, clamp, ignore_high_fp):
    """Per row: the smallest relative distance of the float64 sigmoid from the clamp limits and, of the clamped value, from
    ignore_high_fp (inf where the row sits exactly on one: the hand-written cases)."""
    h = _np(head).astype(F32)[:, 4].astype(F64)
    lo, hi = F64(F32(clamp)), F64(F32(1.0) - F32(clamp))
    with np.errstate(over="ignore"):
        s = 1.0 / (1.0 + np.exp(-h))
    m = np.minimum(np.abs(s / lo - 1.0), np.abs(s / hi - 1.0))
    if ignore_high_fp > 0:
        m = np.minimum(m, np.abs(np.clip(s, lo, hi) / F64(F32(ignore_high_fp)) - 1.0))
    return np.where(m == 0, np.inf, m)


def _giou_parts(H, T):
    pl, pt, pr, pb = (X(H[:, k]) for k in range(4))
    tl, tt, tr, tb = (X(T[:, k]) for k in range(4))
    ta, pa = (tl + tr) * (tt + tb), (pl + pr) * (pt + pb)
    wi, hi_ = xmin(pl, tl) + xmin(pr, tr), xmin(pb, tb) + xmin(pt, tt)
    gw, gh = xmax(pl, tl) + xmax(pr, tr), xmax(pb, tb) + xmax(pt, tt)
    ac, ai = gw * gh, wi * hi_
    au = ta + pa - ai
    return (pl, pt, pr, pb), (tl, tt, tr, tb), wi, hi_, gw, gh, ac, ai, au


def centernet_losses_ref(head, reg_targets, hm_targets, pos_inds, pos_count, gamma=2.0, beta=4.0, clamp=1e-4, ignore_high_fp=0.85,
                         emulate=False, fault=None):
    """ore_centernet_losses_fwd -> dict(giou, pos, neg: scalar X; count: exact int).  Rows with max(reg_target) >= 0 add
    1 - ((ai + 1) / (au + 1) - (ac - au) / ac) (GIoU on ltrb distances); every row adds log(1 - p) p^gamma (1 - hm)^beta unless
    p >= ignore_high_fp > 0; every entry of pos_inds (repeats count again) adds log(p) (1 - p)^gamma; p = clamp(sigmoid(logit)).
    emulate: fp32 terms summed in the kernels' order.  fault: "trip2": rows of the second grid-stride trip dropped; "wave": the partial
    of wave 3 of block 0 dropped; "clamp_open"; "ignore_le"."""
    t, H, T, hm, reg, s, inside, pred, ign, s64, p64, lo, hi = _cn_common(head, reg_targets, hm_targets, clamp, ignore_high_fp, emulate)
    if fault == "ignore_le":
        ign = (ignore_high_fp > 0) & ~(p64 <= F64(F32(ignore_high_fp)))
    rows = H.shape[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        _, _, wi, hi_, gw, gh, ac, ai, au = _giou_parts(H, T)
        iou = (ai + 1.0) / (au + 1.0)
        gterm = xwhere(reg, 1.0 - (iou - (ac - au) / ac), 0.0)
        nw = (1.0 - hm).powc(beta)
        nl = xwhere(ign, 0.0, (1.0 - pred).log() * pred.powc(gamma) * nw)
    nl.m = np.where(ign, 0.0, nl.m)
    gterm.m = np.where(reg, gterm.m, 0.0)
    npos = int(_np(pos_count).reshape(-1)[0])
    pi = _np(pos_inds).reshape(-1)[:npos].astype(np.int64)
    pp = X(pred.v[pi], pred.m[pi], pred.d)
    with np.errstate(divide="ignore", invalid="ignore"):
        pterm = pp.log() * (1.0 - pp).powc(gamma)
    out = {"count": int(reg.sum())}
    if emulate or fault in ("trip2", "wave"):
        out["giou"] = X(_cn_sum_order(gterm.v, rows, fault), gterm.m.sum(), gterm.d + 1 + d_cn_sum(rows))
        out["neg"] = X(_cn_sum_order(nl.v, rows, fault), nl.m.sum(), nl.d + d_cn_sum(rows))
        out["pos"] = X(_lanes64(pterm.v), pterm.m.sum(), pterm.d + d_cn_pos(npos))
    else:
        out["giou"] = gterm.sum(d_cn_sum(rows))
        out["neg"] = nl.sum(d_cn_sum(rows))
        out["pos"] = pterm.sum(d_cn_pos(npos))
    return out


def _butterfly(v):
    """v [..., 64] -> the lane-0 value of six xor-shuffle additions (every lane ends with the same bits: a + b is commutative)."""
    for d in (32, 16, 8, 4, 2, 1):
        idx = np.arange(64) ^ d
        v = v + v[..., idx]
    return v[..., 0]


def _lanes64(x):
    """k_cn_loss_final's sum of a list: lane l adds entries l, l + 64, ... in order, then the butterfly."""
    n = len(x)
    pad = np.zeros(_cdiv(max(n, 1), 64) * 64, dtype=x.dtype)
    pad[:n] = x
    acc = np.zeros(64, dtype=x.dtype)
    for r in pad.reshape(-1, 64):
        acc = acc + r
    return _butterfly(acc)


def _cn_sum_order(x, rows, fault=None):
    """The sum of per-row terms in the order of k_cn_loss_partial / k_cn_loss_final, in the dtype of x."""
    nb = cn_loss_blocks(rows)
    trips = _cdiv(rows, nb * 256)
    pad = np.zeros(trips * nb * 256, dtype=x.dtype)
    pad[:rows] = x
    pad = pad.reshape(trips, nb, 4, 64)
    if fault == "trip2":
        pad = pad[:1]
    acc = np.zeros((nb, 4, 64), dtype=x.dtype)
    for tr in pad:
        acc = acc + tr
    wv = _butterfly(acc)                                                       # [nb, 4]
    if fault == "wave":
        wv[0, 3] = 0
    part = (wv[:, 0] + wv[:, 1]) + (wv[:, 2] + wv[:, 3])
    return _lanes64(part)


def centernet_loss_grad_ref(head, reg_targets, hm_targets, pos_inds, pos_count, coef3, gamma=2.0, beta=4.0, clamp=1e-4,
                            ignore_high_fp=0.85, emulate=False, fault=None):
    """ore_centernet_losses_bwd -> X [rows, 5]: coef3[0] d(giou sum) + coef3[2] d(-neg sum) + coef3[1] d(-pos sum) w.r.t. head[:, :5].
    min / max ties split 0.5 / 0.5 (torch.minimum / maximum), the clamp passes the gradient on the closed interval (torch.clamp), a row
    named k times by pos_inds takes k positive terms.  fault: "tie10": ties give 1 / 0; "clamp_open"; "ignore_le"; "dup_once"."""
    t, H, T, hm, reg, s, inside, pred, ign, s64, p64, lo, hi = _cn_common(head, reg_targets, hm_targets, clamp, ignore_high_fp, emulate)
    if fault == "ignore_le":
        ign = (ignore_high_fp > 0) & ~(p64 <= F64(F32(ignore_high_fp)))
    if fault == "clamp_open":
        inside = (s64 > F64(lo)) & (s64 < F64(hi))
    c = _np(coef3).astype(F32).astype(t)
    c0, c1, c2 = (X(np.asarray(v, dtype=t)) for v in c)
    half = 1.0 if fault == "tie10" else 0.5
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        (pl, pt, pr, pb), (tl, tt, tr, tb), wi, hi_, gw, gh, ac, ai, au = _giou_parts(H, T)
        inv_u, inv_c = 1.0 / (au + 1.0), 1.0 / ac
        dai_, dau_, dac_ = -inv_u, (ai + 1.0) * inv_u * inv_u - inv_c, au * inv_c * inv_c

        def gradv(dpa, side, pv, tv):
            lt, eq, gt_ = pv.v < tv.v, pv.v == tv.v, pv.v > tv.v
            dmin = np.where(lt, 1.0, np.where(eq, half, 0.0)).astype(t)
            dmax = np.where(gt_, 1.0, np.where(eq, 1.0 - half if fault == "tie10" else half, 0.0)).astype(t)
            dai, dac = side[0] * X(dmin), side[1] * X(dmax)
            return xwhere(reg, c0 * (dai_ * dai + dau_ * (dpa - dai) + dac_ * dac), 0.0)
        g0 = gradv(pt + pb, (hi_, gh), pl, tl)
        g2 = gradv(pt + pb, (hi_, gh), pr, tr)
        g1 = gradv(pl + pr, (wi, gw), pt, tt)
        g3 = gradv(pl + pr, (wi, gw), pb, tb)
        nw = (1.0 - hm).powc(beta)
        omp = 1.0 - pred
        dg = nw * (-(pred.powc(gamma)) / omp + X(np.asarray(F32(gamma), dtype=t)) * pred.powc(gamma - 1.0) * omp.log())
        gx = xwhere(inside & ~ign, -c2 * dg * s * (1.0 - s), 0.0)
        df = (1.0 - s).powc(gamma) / s - X(np.asarray(F32(gamma), dtype=t)) * s.log() * (1.0 - s).powc(gamma - 1.0)
        pg = -c1 * df * s * (1.0 - s)
    rows = H.shape[0]
    npos = int(_np(pos_count).reshape(-1)[0])
    pi = _np(pos_inds).reshape(-1)[:npos].astype(np.int64)
    if fault == "dup_once":
        pi = np.unique(pi)
    k = np.bincount(pi, minlength=rows) * inside
    kmax = int(k.max()) if rows else 0
    v4, m4 = gx.v.copy(), np.where(inside & ~ign, gx.m, 0.0)
    for j in range(kmax):                                                      # one atomicAdd per naming, equal addends
        sel = k > j
        v4 = np.where(sel, v4 + pg.v, v4)
        m4 = np.where(sel, m4 + pg.m, m4)
    cols = [g0, g1, g2, g3]
    v = np.stack([np.where(reg, g.v, 0.0) for g in cols] + [v4], 1)
    m = np.stack([np.where(reg, g.m, 0.0) for g in cols] + [m4], 1)
    return X(v, m, max(max(g.d for g in cols), max(gx.d, pg.d) + kmax))


def cn_loss_inputs(rows, seed, ld=5, clamp=1e-4, ignore_high_fp=0.85, device="cpu", n_pos=None):
    """(head [rows, ld], reg_targets [rows, 4], hm_targets [rows], pos_inds int64, pos_count int32) fp32.  A third of the rows carry a
    regression target (>= 0; the rest -CN_INF / 8); predictions are >= 0 with per-row scales 1e-2..1e2.  The FIRST rows are the edge rows
    (as many as fit): an exact-0 prediction; pred == target on one, two and four sides; logits +-12, +-20, +-100; hm_targets exactly 0 and
    1.  pos_inds has a repeated row.  Columns 5.. of a wider head are NaN.  Logits whose sigmoid is closer than S_MARGIN (relative) to a
    clamp limit or to ignore_high_fp are re-drawn from the next seed."""
    rng = np.random.default_rng(seed)
    sc = 10.0 ** rng.uniform(-2, 2, (rows, 1))
    tgt = (np.abs(rng.standard_normal((rows, 4))) * sc + 0.01 * sc).astype(F32)
    pred = (tgt * np.exp(rng.uniform(-1, 1, (rows, 4)))).astype(F32)
    has = rng.uniform(0, 1, rows) < 1.0 / 3
    logit = (rng.standard_normal(rows) * 4.0).astype(F32)
    hm = np.where(rng.uniform(0, 1, rows) < 0.5, 0.0, rng.uniform(0, 1, rows) ** 3).astype(F32)
    edges = [("zero", None), ("tie1", None), ("tie2", None), ("tie4", None), ("l", 12.0), ("l", -12.0), ("l", 20.0), ("l", -20.0),
             ("l", 100.0), ("l", -100.0), ("hm", 0.0), ("hm", 1.0)]
    for i, (kind, val) in enumerate(edges[:rows]):
        has[i] = True
        if kind == "zero":
            pred[i, 0] = 0.0
        elif kind == "tie1":
            pred[i, 1] = tgt[i, 1]
        elif kind == "tie2":
            pred[i, [0, 3]] = tgt[i, [0, 3]]
        elif kind == "tie4":
            pred[i] = tgt[i]
        elif kind == "l":
            logit[i] = val
        elif kind == "hm":
            hm[i] = val; has[i] = False
    if rows > len(edges):                                                      # the last row (a grid-stride trip of its own at 65 537) counts
        has[-1], logit[-1], hm[-1] = True, 1.0, 0.0
    tgt[~has] = F32(-CN_INF / 8.0)
    redrawn, s = 0, seed
    while True:
        bad = cn_margins(np.concatenate([pred, logit[:, None]], 1), clamp, ignore_high_fp) < S_MARGIN
        if not bad.any():
            break
        s += 1000003
        redrawn += int(bad.sum())
        logit[bad] = (np.random.default_rng(s).standard_normal(int(bad.sum())) * 4.0).astype(F32)
    _count("cn_loss_inputs", rows, redrawn)
    head = np.full((rows, ld), np.nan, dtype=F32)
    head[:, :4], head[:, 4] = pred, logit
    n_pos = min(rows, 40) if n_pos is None else n_pos
    pi = rng.integers(0, rows, max(n_pos, 1)).astype(np.int64)
    if n_pos >= 3:
        pi[2] = pi[0]                                                          # a repeated row
        pi[1] = min(4, rows - 1)                                               # logit 12: outside the clamp, no positive gradient
    if n_pos >= 4 and rows > 11:
        pi[3] = 11                                                             # the hm == 1 row
    return (to_t(head, device), to_t(tgt, device), to_t(hm, device), to_t(pi, device),
            to_t(np.array([n_pos], dtype=np.int32), device))


# ---- CenterNet targets -----------------------------------------------------------------------------------------------------------------
def centernet_targets_ref(gt, counts, shapes, strides=(8, 16, 32), soi=((0, 64), (48, 192), (128, 1000000)), hm_min_overlap=0.8,
                          min_radius=4.0, fault=None):
    """ore_centernet_targets_fwd for gt [B, max_n, 4] fp32 boxes on the 1/8 px grid, counts [B] -> dict(reg_targets: exact float32
    [rows, 4]; hm: X [rows] (exact 0 below the cut); pos_inds int64, pos_count; margins: dict of the smallest margin per decision).
    Rows are level-major [level][image][y][x].  fault: "owner_le": the LAST minimum owns a location; "in_box_ge": in_box with >= 0;
    "half7": stride 16's half-cell offset taken as 7."""
    gt = _np(gt).astype(F32)
    counts = _np(counts).astype(np.int64)
    B, max_n = gt.shape[0], gt.shape[1]
    L = len(strides)
    delta = (1.0 - float(hm_min_overlap)) / (1.0 + float(hm_min_overlap))
    delta2x2, minr2 = F64(F32(delta * delta * 2.0)), F64(F32(float(min_radius) * float(min_radius)))
    regs, hv, hmg, pos = [], [], [], []
    mg = {"soi": math.inf, "owner": math.inf, "hm_cut": math.inf}
    hd = 0
    for l in range(L):
        Hl, Wl = shapes[l]
        st = strides[l]
        fs = F64(st)
        half = 7.0 if (fault == "half7" and st == 16) else float(st // 2)
        ii = np.arange(Hl * Wl)
        gx = ((ii % Wl) * st).astype(F64) + half
        gy = ((ii // Wl) * st).astype(F64) + half
        lo_, hi_ = F64(F32(soi[l][0])), F64(F32(soi[l][1]))
        for b in range(B):
            N = int(min(counts[b], max_n, 128))
            M = Hl * Wl
            if N == 0:
                regs.append(np.full((M, 4), F32(-CN_INF) / F32(st), dtype=F32))
                hv.append(np.zeros(M)); hmg.append(np.zeros(M))
                continue
            bx = gt[b, :N].astype(F64)                                         # every expression below is exact on the 1/8 px grid
            x1, y1, x2, y2 = (bx[:, k][None, :] for k in range(4))
            l_, t_, r_, b_ = gx[:, None] - x1, gy[:, None] - y1, x2 - gx[:, None], y2 - gy[:, None]
            scx, scy = (x1 + x2) / 2.0, (y1 + y2) / 2.0
            cdx = np.trunc(scx / fs) * fs + fs / 2.0
            cdy = np.trunc(scy / fs) * fs + fs / 2.0
            ddx, ddy = gx[:, None] - cdx, gy[:, None] - cdy
            is_peak = (ddx == 0) & (ddy == 0)
            mn = np.minimum(np.minimum(l_, t_), np.minimum(r_, b_))
            in_box = (mn >= 0) if fault == "in_box_ge" else (mn > 0)
            c33 = (np.abs(ddx) <= fs) & (np.abs(ddy) <= fs) & in_box
            sw, sh = l_ + r_, t_ + b_
            crit = np.sqrt(sw * sw + sh * sh) / 2.0
            cared = (crit >= lo_) & (crit <= hi_)
            for lim in (lo_, hi_):
                rel = np.abs(crit / max(lim, 1e-30) - 1.0) if lim > 0 else np.full_like(crit, np.inf)
                rel = np.where(crit == lim, np.inf, rel)                       # exactly on the limit: 3-4-5 boxes, exact in fp32
                mg["soi"] = min(mg["soi"], float(rel.min()))
            area = X((x2 - x1)[0]) * X((y2 - y1)[0])
            sr2 = xmax(X(np.asarray(delta2x2)) * area, X(np.asarray(minr2)))
            ex, ey = X(np.broadcast_to(gx[:, None] - scx, (M, N)).copy()), X(np.broadcast_to(gy[:, None] - scy, (M, N)).copy())
            d2 = xwhere(is_peak, 0.0, ex * ex + ey * ey)
            d2.m = np.where(is_peak, 0.0, d2.m)
            wd = d2 / X(np.broadcast_to(sr2.v, (M, N)), np.broadcast_to(sr2.m, (M, N)), sr2.d)
            wd.m = np.where(is_peak, 0.0, wd.m)
            hd = max(hd, wd.d)
            hi_idx = wd.v.argmin(1)
            hmin = wd.v[ii, hi_idx]
            hv.append(hmin); hmg.append(wd.m[ii, hi_idx])
            mg["hm_cut"] = min(mg["hm_cut"], float(np.abs(hmin / LN_1E4 - 1.0).min()))
            dm = np.where(c33 & cared, wd.v, np.inf)
            if fault == "owner_le":
                own = N - 1 - dm[:, ::-1].argmin(1)
            else:
                own = dm.argmin(1)                                             # the first minimum
            best = dm[ii, own]
            if N > 1:                                                          # owner margin: second smallest against smallest
                srt = np.sort(dm, 1)
                a0, a1 = srt[:, 0], srt[:, 1]
                both = np.isfinite(a1)
                o2 = np.where(dm == a0[:, None], np.arange(N)[None, :], -1).max(1)      # the last index holding the minimum
                same = (gt[b, own] == gt[b, np.maximum(o2, 0)]).all(1) | (a1 == 0)      # identical boxes, or two literal zeros
                with np.errstate(invalid="ignore", divide="ignore"):
                    rel = np.where(both, np.where((a1 == a0) & same, np.inf, (a1 - a0) / np.maximum(a1, 1e-300)), np.inf)
                mg["owner"] = min(mg["owner"], float(rel.min()))
            rt = np.stack([l_[ii, own], t_[ii, own], r_[ii, own], b_[ii, own]], 1) / fs
            rt = np.where(np.isfinite(best)[:, None], rt, F64(F32(-CN_INF) / F32(st)))
            regs.append(rt.astype(F32))
    hmin, hmag = np.concatenate(hv), np.concatenate(hmg)
    nz = np.concatenate([np.full(shapes[l][0] * shapes[l][1], min(counts[b], max_n, 128) > 0) for l in range(L) for b in range(B)])
    hx = (-X(hmin, hmag, hd)).exp()
    keep = nz & (hmin < LN_1E4)
    hm = X(np.where(keep, hx.v, 0.0), np.where(keep, hx.m, 0.0), hx.d)
    # positives: (image, object, level) order
    row0 = np.cumsum([0] + [B * h * w for h, w in shapes])
    for b in range(B):
        for n in range(int(min(counts[b], max_n))):
            x1, y1, x2, y2 = (F64(v) for v in gt[b, n])
            crit = math.sqrt((x2 - x1) ** 2 + (y2 - y1) ** 2) / 2.0
            for l in range(L):
                if F64(F32(soi[l][0])) <= crit <= F64(F32(soi[l][1])):
                    fs = float(strides[l])
                    cx, cy = int(((x1 + x2) / 2.0) / fs), int(((y1 + y2) / 2.0) / fs)
                    pos.append(int(row0[l]) + b * shapes[l][0] * shapes[l][1] + cy * shapes[l][1] + cx)
    return dict(reg_targets=np.concatenate(regs), hm=hm, pos_inds=np.array(pos, dtype=np.int64), pos_count=len(pos), margins=mg)


CN_SOI = ((0, 40), (40, 80), (80, 1000000))         # limits that 3-4-5 boxes hit exactly: 48 x 64 -> 40, 96 x 128 -> 80
CN_EXACT_BOXES = [
    (16.0, 24.0, 64.0, 88.0),           # 48 x 64: crit = 40 exactly, on both the upper limit of level 0 and the lower one of level 1
    (16.0, 24.0, 64.0, 88.0),           # the same box again: every location is an exact tie, the first one owns it
    (100.0, 20.0, 228.0, 116.0),        # 128 x 96: crit = 80 exactly; its left side x = 100 lies on stride 8's grid centres (in_box false at 0)
    (32.0, 32.0, 40.0, 40.0),           # centred on the stride-8 grid point (36, 36): the peak; its discretised centre equals the centre
    (48.0, 40.0, 80.0, 56.0),           # centred on (64, 48): a cell border of every level
    (4.0, 4.0, 52.0, 68.0),             # 48 x 64 again, elsewhere
    (30.0, 30.0, 40.0, 44.0),           # centre (35, 37): the same stride-8 cell as the 8 x 8 box above, so both distances are the literal 0 at
                                        # (36, 36): an exact tie between DIFFERENT boxes, the earlier one owns the location
    (188.0, 62.0, 202.0, 74.0),         # its left side x = 188 is a stride-8 grid centre one cell left of its centre cell (196, 68): l = 0 there,
                                        # inside the centre 3x3 but not in_box
]


def cn_target_boxes(B, counts, hw, seed, shapes, strides=(8, 16, 32), soi=CN_SOI):
    """gt [B, max_n, 4] fp32 on the 1/8 px grid inside the hw = (H, W) image, counts[b] boxes in image b, the first of them
    CN_EXACT_BOXES (as many as fit and lie inside the image).  A draw that leaves a margin of centernet_targets_ref below CN_MARGIN /
    HM_MARGIN is made again from the next seed for the images concerned.  -> (gt, counts int32, seeds tried)."""
    Himg, Wimg = hw
    max_n = max(1, max(counts))
    gt = np.zeros((B, max_n, 4), dtype=F32)
    tried = 0
    for b in range(B):
        n = counts[b]
        if n == 0:
            continue
        s = seed * 7919 + b
        while True:
            tried += 1
            rng = np.random.default_rng(s)
            fixed = [bx for bx in CN_EXACT_BOXES if bx[2] <= Wimg and bx[3] <= Himg][:n]
            for i, bx in enumerate(fixed):
                gt[b, i] = bx
            k = n - len(fixed)
            if k:
                wh = np.exp(rng.uniform(math.log(6.0), math.log(min(Himg, Wimg) * 0.9), (k, 2)))
                xy = rng.uniform(0, 1, (k, 2)) * (np.array([Wimg, Himg]) - wh)
                q = np.round(np.concatenate([xy, xy + wh], 1) * 8.0) / 8.0
                gt[b, len(fixed):n] = q
            one = np.zeros((1, max_n, 4), dtype=F32)
            one[0] = gt[b]
            mg = centernet_targets_ref(one, [n], shapes, strides, soi)["margins"]
            if mg["soi"] >= CN_MARGIN and mg["owner"] >= CN_MARGIN and mg["hm_cut"] >= HM_MARGIN:
                break
            s += 1000003
    _count("cn_target_boxes", tried, tried - sum(1 for c in counts if c))
    return gt, np.asarray(counts, dtype=np.int32), tried


# ---- ROI sampling ----------------------------------------------------------------------------------------------------------------------
def _iou64(c, g):
    """IoU [N, G] of fp32 boxes in float64, by the kernel's expression."""
    c, g = c.astype(F64), g.astype(F64)
    ag = (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1])
    ac = (c[:, 2] - c[:, 0]) * (c[:, 3] - c[:, 1])
    w = np.maximum(np.minimum(g[None, :, 2], c[:, None, 2]) - np.maximum(g[None, :, 0], c[:, None, 0]), 0.0)
    h = np.maximum(np.minimum(g[None, :, 3], c[:, None, 3]) - np.maximum(g[None, :, 1], c[:, None, 1]), 0.0)
    inter = w * h
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(inter > 0, inter / (ag[None, :] + ac[:, None] - inter), 0.0)


def sample_match(prop, prop_n, gtp, gt_n, append_gt, thr):
    """The matcher of ore_sample_rois_fwd in float64 -> (label [B,N] in {0 fg, 1 bg, 2 not a candidate}, matched gt index [B,N],
    the smallest margin: |iou - thr| / thr, and (best - second best) / best unless the two ground-truth boxes are identical or both
    IoUs are 0)."""
    prop, gtp = _np(prop).astype(F32), _np(gtp).astype(F32)
    pn, gn = _np(prop_n).astype(np.int64), _np(gt_n).astype(np.int64)
    B, cap, G = prop.shape[0], prop.shape[1], gtp.shape[1]
    N = cap + (G if append_gt else 0)
    lab = np.full((B, N), 2, dtype=np.int64)
    mi = np.zeros((B, N), dtype=np.int64)
    margin = math.inf
    th = F64(F32(thr))
    for b in range(B):
        p, g = min(int(pn[b]), cap), min(int(gn[b]), G)
        cand = np.concatenate([prop[b], gtp[b]], 0) if append_gt else prop[b]
        cv = np.concatenate([np.arange(cap) < p, np.arange(G) < g]) if append_gt else np.arange(cap) < p
        if g == 0:
            lab[b] = np.where(cv, 1, 2)
            continue
        iou = _iou64(cand, gtp[b, :g])
        bi = iou.argmax(1)                                                     # the first maximum
        best = iou[np.arange(N), bi]
        lab[b] = np.where(cv, np.where(best >= th, 0, 1), 2)
        mi[b] = bi
        margin = min(margin, float(np.abs(best[cv] / th - 1.0).min()) if cv.any() else math.inf)
        if g > 1:
            tmp = iou.copy()
            tmp[np.arange(N), bi] = -1.0
            b2 = tmp.argmax(1)
            sec = tmp[np.arange(N), b2]
            same = (gtp[b, bi] == gtp[b, b2]).all(1) | (best == 0)
            with np.errstate(divide="ignore", invalid="ignore"):
                rel = np.where(same & (sec == best), np.inf, (best - sec) / np.maximum(best, 1e-300))
            margin = min(margin, float(rel[cv].min()) if cv.any() else math.inf)
    return lab, mi, margin


def sample_rois_ref(prop, prop_n, gtp, gt_n, keys, R, P, thr, append_gt=True, tie_high=False):
    """ore_sample_rois_fwd, every output exact: per image n_pos = min(#fg, P) foreground candidates then n_neg = min(#bg, R - n_pos)
    background ones, each group the smallest keys in ascending (key, candidate index) order; the remaining rows are padding (box
    (0, 0, 8, 8), label 1, gt 0, valid 0).  -> (boxes [B,R,4] f32, labels [B,R] i64, gt [B,R,4] f32, valid [B,R] bool, matcher margin).
    tie_high (a fault for tests/test_trainloss_host.py): equal keys go to the higher index first."""
    prop_, gtp_, keys_ = _np(prop).astype(F32), _np(gtp).astype(F32), _np(keys).astype(F32)
    lab, mi, margin = sample_match(prop, prop_n, gtp, gt_n, append_gt, thr)
    B, N = lab.shape
    boxes = np.tile(np.array([0, 0, 8, 8], dtype=F32), (B, R, 1))
    gt = np.zeros((B, R, 4), dtype=F32)
    labels = np.ones((B, R), dtype=np.int64)
    valid = np.zeros((B, R), dtype=bool)
    for b in range(B):
        cand = np.concatenate([prop_[b], gtp_[b]], 0) if append_gt else prop_[b]
        j = 0
        for L_ in (0, 1):
            idx = np.nonzero(lab[b] == L_)[0]
            lim = min(len(idx), P) if L_ == 0 else min(len(idx), R - j)
            order = np.lexsort((-idx if tie_high else idx, keys_[b, idx]))
            pick = idx[order][:lim]
            boxes[b, j:j + lim] = cand[pick]
            gt[b, j:j + lim] = gtp_[b, mi[b, pick]]
            labels[b, j:j + lim] = L_
            valid[b, j:j + lim] = True
            j += lim
    return boxes, labels, gt, valid, margin


def sample_rois_histogram(lab, keys, R, P, wrap=False):
    """The kernel's selection by histogram, for one image: lab [N], keys [N] -> the candidate index of every output row (-1 padding).
    wrap (a fault): the bin of key 1.0 is 256 & 255 = 0 instead of min(255, .)."""
    keys = keys.astype(F32)
    q = (keys * F32(256.0)).astype(np.int64)
    bins = (q & 255) if wrap else np.clip(q, 0, 255)
    out, j = np.full(R, -1, dtype=np.int64), 0
    for L_ in (0, 1):
        idx = np.nonzero(lab == L_)[0]
        lim = min(len(idx), P) if L_ == 0 else min(len(idx), R - j)
        if lim > 0:
            hist = np.bincount(bins[idx], minlength=256)
            cut = int(np.argmax(np.cumsum(hist) >= lim))
            el = idx[bins[idx] <= cut]
            order = np.lexsort((el, keys[el]))
            pick = el[order][:lim]
            out[j:j + len(pick)] = pick
        j += lim
    return out


def sample_inputs(B, cap, G, append_gt, seed, thr=0.5, keys="uniform", device="cpu"):
    """(prop [B,cap,4], prop_n [B] int64, gtp [B,G,4], gt_n [B] int64, keys [B,N]) fp32: ground truth inside a 640 px image (with one
    duplicated box where G >= 3), a third of the proposals jittered copies of a ground-truth box (IoU on either side of thr), the rest
    anywhere.  Images cycle through: everything valid; gt_n = 0; prop_n = 0; 5 proposals only.  A draw whose matcher margin is below
    IOU_MARGIN is made again from the next seed."""
    N = cap + (G if append_gt else 0)
    s = seed
    while True:
        rng = np.random.default_rng(s)
        gwh = np.exp(rng.uniform(math.log(16.0), math.log(300.0), (B, G, 2)))
        gxy = rng.uniform(0, 1, (B, G, 2)) * (640.0 - gwh)
        gtp = np.concatenate([gxy, gxy + gwh], 2).astype(F32)
        if G >= 3:
            gtp[:, 2] = gtp[:, 0]
        src = rng.integers(0, G, (B, cap))
        base = np.take_along_axis(gtp, src[:, :, None].repeat(4, 2), 1).astype(F64)
        size = np.concatenate([base[..., 2:] - base[..., :2]] * 2, 2)
        near = base + rng.uniform(-0.25, 0.25, (B, cap, 4)) * size
        pwh = np.exp(rng.uniform(math.log(8.0), math.log(400.0), (B, cap, 2)))
        pxy = rng.uniform(0, 1, (B, cap, 2)) * (640.0 - pwh)
        far = np.concatenate([pxy, pxy + pwh], 2)
        prop = np.where((rng.uniform(0, 1, (B, cap, 1)) < 1.0 / 3), near, far).astype(F32)
        prop_n = np.full(B, cap, dtype=np.int64)
        gt_n = np.full(B, G, dtype=np.int64)
        for b in range(B):
            if b % 4 == 1:
                gt_n[b] = 0
            elif b % 4 == 2:
                prop_n[b] = 0
            elif b % 4 == 3:
                prop_n[b] = min(5, cap)
        if B > 4:
            gt_n[4] = max(1, G // 2)
        _, _, margin = sample_match(prop, prop_n, gtp, gt_n, append_gt, thr)
        _count("sample_inputs", 1, 0 if margin >= IOU_MARGIN else 1)
        if margin >= IOU_MARGIN:
            break
        s += 1000003
    if keys == "uniform":
        u = rng.uniform(0, 1, (B, N)).astype(F32)
    elif keys == "equal":
        u = np.full((B, N), 0.37, dtype=F32)
    elif keys == "one_bin":
        u = (F32(0.5) + rng.integers(0, 64, (B, N)).astype(F32) * F32(2.0 ** -16)).astype(F32)     # all in bin 128, many equal keys
    elif keys == "outside":
        u = rng.uniform(0, 1, (B, N)).astype(F32)
        u[:, 0::5] = rng.choice(np.array([0.0, 1.0, -0.5, 2.0], dtype=F32), u[:, 0::5].shape)
    else:
        raise ValueError(keys)
    return tuple(to_t(a, device) for a in (prop, prop_n, gtp, gt_n, u))


# ---- ROIAlign backward -------------------------------------------------------------------------------------------------------------
# The exact transpose of inferops_ref.roi_align_ref: the same roi_decisions (level, gh, gw, sample coordinates, validity), the same
# border clamps.  The sample grid and the bilinear weights are separable, so a ROI's gradient is
#     dF[cy, cx, c] = (1 / cnt) sum_by sum_bx Wy[by, cy] Wx[bx, cx] dout[by, bx, c],
# Wy[by, cy] the sum over the bin's gh sample rows of their weight on feature row cy (1 - fr on the lower, fr on the upper cell).  mag is
# the same over |dout|.  fp32 sample coordinates move a weight by about u |coord|: as in the forward reference a sample adds
# C_ROI_COORD (|y| + 1/2) (or |x| + 1/2) to the sensitivity E of each cell it touches, the 2-D sensitivity is Ey Wx + Wy Ex, and mag takes
# it divided by sqrt(d).
# Depth, per form (csrc/ore_roi.hip):
#   tiled (k_roi_align_bwd_tile) and column (k_roi_align_bwd_col): an axis weight sum is g additions on top of 1 - fr (g + 1); * inv (1);
#     the fold over the nbx bins that reach a column, a product and an addition each (2 nbx); the weighted row sum over nby bins
#     (2 nby); then ONE addition per ROI that reaches the cell, in ROI order (tiled) or by atomics (column).  A ROI with a bin wider than
#     ROI_AX = 8 cells takes the per-sample walk (tiled) / roi_bwd_bins (the column kernel's ext[4] fallback): dout / cnt (1), the
#     weights (g + 1, 1 for the product), the product with dout (1), and one addition per (bin, cell) or per sample -- counted as one
#     contribution per sample that touches the cell.
#     d = gmax + 2 + 2 nbx + 2 nby + 3 + contributions, all maxima over the ROIs / cells of the call.
#   fixed point (ore_roi_align_bwd_det): the same d, plus an ABSOLUTE term 2^-41 per contribution to the cell (rint(v 2^40)); valid
#     only while |sum| < 2^23 (asserted by the test on its reference).
#   fp32 atomics: the same d with an unordered chain; the bound does not depend on the order.
ROI_AX = 8
FX_ABS = 2.0 ** -41


def _roi_axis(vs, valid, Ln, P, g, dtype, fault):
    """Axis footprint matrices [P, Ln]: W (weight sums), E (coordinate sensitivity), S (samples touching a cell)."""
    W = np.zeros((P, Ln), dtype=dtype); E = np.zeros((P, Ln)); S = np.zeros((P, Ln), dtype=np.int64)
    for b in range(P):
        for i in range(g):
            v = vs[b * g + i]
            if not valid[b * g + i] or (fault == "yH" and v == Ln):
                continue
            raw = abs(float(v))
            v = max(v, dtype(0))
            top = Ln - 2 if (fault == "clampH2" and Ln > 1) else Ln - 1
            lo = int(v)
            if lo >= top:
                lo = hi = top; v = dtype(lo)
            else:
                hi = lo + 1
            fr = v - dtype(lo)
            W[b, lo] += dtype(1) - fr; W[b, hi] += fr
            for c_ in {lo, hi}:
                E[b, c_] += IR.C_ROI_COORD * (raw + 0.5); S[b, c_] += 1
    return W, E, S


def roi_align_bwd_ref(dout, HWs, scales, min_level, P, boxes, bidx, B, C, fault=None, emulate=False, base=None, quantise=False):
    """ore_roi_align_bwd / _det / _tiled -> dict(ref, mag: lists per level of float64 [B, H, W, C]; contrib: per level [B, H, W] int
    contributions per cell; d: the depth).  base: per-level maps to accumulate into (one more addition).  fault (host tests): "yH", "grid"
    (gh + 1), "level" (one too high), "clampH2", "cnt" (cnt of the next box), "skip" (the last ROI of the fullest cell left out), "image"
    (image b + 1).  emulate: fp32 decisions, weights and sums (ROI by ROI, in order); with quantise every ROI's contribution to a cell goes
    through rint(v 2^40) 2^-40 first, as in the fixed-point form."""
    npT = np.float32 if emulate else np.float64
    bx = _np(boxes).astype(F32)
    do = _np(dout).astype(F32).astype(npT).reshape(bx.shape[0], P, P, C)
    n = bx.shape[0]
    bi = np.zeros(n, dtype=np.int64) if bidx is None else _np(bidx).astype(np.int64)
    ref = [np.zeros((B, h, w, C), dtype=npT) if base is None else _np(base[l]).astype(F32).astype(npT).reshape(B, h, w, C).copy() for l, (h, w) in enumerate(HWs)]
    mag = [np.abs(r).astype(F64) for r in ref]
    magc = [np.zeros((B, h, w, C)) for h, w in HWs]
    contrib = [np.zeros((B, h, w), dtype=np.int64) for h, w in HWs]
    last = [np.full((B, h, w), -1, dtype=np.int64) for h, w in HWs]
    gmax, nbx, nby, nwide = 1, 1, 1, 0
    decs = [IR.roi_decisions(bx[r], scales, min_level, P, HWs, npT) for r in range(n)]
    parts = []
    for r in range(n):
        d = decs[r]
        lv = d["level"]
        if fault == "level" and lv + 1 < len(scales):
            lv += 1
            d = IR.roi_decisions(bx[r], [scales[lv]] * len(scales), min_level, P, [HWs[lv]] * len(scales), npT)
        gh, gw = d["gh"], d["gw"]
        cnt = float(max(gh * gw, 1))
        if fault == "cnt":
            d2 = decs[(r + 1) % n]
            cnt = float(max(d2["gh"] * d2["gw"], 1))
        ys, vy = d["ys"], d["vy"]
        H, W = HWs[lv]
        if fault == "grid":
            b = [np.float64(v) for v in bx[r]]
            sc = np.float64(np.float32(scales[lv]))
            y0, bh = b[1] * sc - 0.5, (b[3] - b[1]) * sc / P
            gh = gh + 1
            ys = np.array([y0 + ph * bh + (iy + 0.5) * bh / gh for ph in range(P) for iy in range(max(gh, 0))])
            vy = ~((ys < -1) | (ys > H))
            cnt = float(max(gh * gw, 1))
        if gh <= 0 or gw <= 0:
            continue
        Wy, Ey, Sy = _roi_axis(ys, vy, H, P, gh, npT, fault)
        Wx, Ex, Sx = _roi_axis(d["xs"], d["vx"], W, P, gw, npT, fault)
        ry, rx = np.nonzero(Sy.sum(0))[0], np.nonzero(Sx.sum(0))[0]
        if not len(ry) or not len(rx):
            continue
        y0, y1, x0, x1 = ry[0], ry[-1] + 1, rx[0], rx[-1] + 1
        Wy, Ey, Sy, Wx, Ex, Sx = Wy[:, y0:y1], Ey[:, y0:y1], Sy[:, y0:y1], Wx[:, x0:x1], Ex[:, x0:x1], Sx[:, x0:x1]
        gmax = max(gmax, gh, gw)
        nbx, nby = max(nbx, int((Wx != 0).sum(0).max())), max(nby, int((Wy != 0).sum(0).max()))
        wide = max(int((Sy[b] > 0).sum()) for b in range(P)) > ROI_AX or max(int((Sx[b] > 0).sum()) for b in range(P)) > ROI_AX
        nwide += int(wide)
        img = int(bi[r])
        if fault == "image":
            img = (img + 1) % B
        inv = npT(1.0) / npT(cnt)
        fold = lambda A, Bm, v: np.einsum("ph,pwc->hwc", A, np.einsum("qw,pqc->pwc", Bm, v))      # noqa: E731
        g_ = fold(Wy, Wx * inv, do[r])
        gm = fold(np.abs(Wy).astype(F64), np.abs(Wx).astype(F64) / cnt, np.abs(do[r]).astype(F64))
        gc = (fold(Ey, np.abs(Wx).astype(F64), np.abs(do[r]).astype(F64)) + fold(np.abs(Wy).astype(F64), Ex, np.abs(do[r]).astype(F64))) / cnt
        touch = (Sy.sum(0)[:, None] > 0) & (Sx.sum(0)[None, :] > 0) & ((np.abs(Wy).sum(0)[:, None] * np.abs(Wx).sum(0)[None, :]) != 0)
        k = np.where(touch, (Sy.sum(0)[:, None] * Sx.sum(0)[None, :]) if wide else 1, 0)
        parts.append((lv, img, y0, y1, x0, x1, g_, gm, gc, k, touch, r))
        contrib[lv][img, y0:y1, x0:x1] += k
        last[lv][img, y0:y1, x0:x1] = np.where(touch, r, last[lv][img, y0:y1, x0:x1])
    skip = None
    if fault == "skip":
        lv = int(np.argmax([c.max() for c in contrib]))
        pos = np.unravel_index(int(contrib[lv].argmax()), contrib[lv].shape)
        skip = (lv, pos, int(last[lv][pos]))
    for lv, img, y0, y1, x0, x1, g_, gm, gc, k, touch, r in parts:
        if skip and skip[0] == lv and skip[2] == r and skip[1][0] == img:
            g_ = g_.copy()
            g_[skip[1][1] - y0, skip[1][2] - x0] = 0
        if quantise:
            g_ = (np.rint(g_.astype(F64) * 2.0 ** 40) * 2.0 ** -40).astype(g_.dtype)
        ref[lv][img, y0:y1, x0:x1] += g_
        mag[lv][img, y0:y1, x0:x1] += gm
        magc[lv][img, y0:y1, x0:x1] += gc
    cmax = max(int(c.max()) for c in contrib)
    d = gmax + 2 + 2 * nbx + 2 * nby + 3 + cmax + (1 if base is not None else 0)
    mag = [m + mc / math.sqrt(d) for m, mc in zip(mag, magc)]
    return dict(ref=[r.astype(F64) if not emulate else r for r in ref], mag=mag, contrib=contrib, d=d, wide=nwide,
                levels=sorted({p_[0] for p_ in parts}))


def roi_bwd_hold(got, ref, mag, d, contrib=None):
    """(hard, rms) of one level's map [B, H, W, C].  contrib: the fixed-point form's absolute term, k 2^-41 for a cell with k contributions
    (each rint(v 2^40) is off by at most 2^-41).  It is a bound on that part of the error, not a rounding of relative size u, so each
    check takes it in the units of its own right-hand side: |err| <= 2 d u mag + k 2^-41 is the element check with
    mag + k 2^-41 / (2 d u); and since (a + b) / (A + B) <= max(a / A, b / B), the rms check holds with mag + k 2^-41 / (u sqrt(d))."""
    ref, mag = torch.as_tensor(ref), torch.as_tensor(mag)
    g = got.detach().cpu().reshape(ref.shape)
    if contrib is None:
        return check2(g, ref, mag, d)
    q = torch.as_tensor(contrib, dtype=torch.float64).unsqueeze(-1) * FX_ABS
    return check2(g, ref, mag + q / (2.0 * d * U), d)[0], check2(g, ref, mag + q / (U * math.sqrt(d)), d)[1]


# elongated boxes whose bins are wider than ROI_AX = 8 cells at pooled > 1 too (310 px wide on the finest level: 10 to 19 cells per bin at
# pooled 4, 6 to 12 at pooled 7): the per-sample walk of the tiled form and the column form's fallback with ph, pw > 0
ROI_WIDE_BOXES = [(10.0, 100.0, 310.0, 120.0), (10.0, 100.0, 310.0, 108.0)]
# a 32 px image at strides 8 / 16 / 32: maps 4 x 4, 2 x 2 and 1 x 1.  On the 1 x 1 level every valid sample clamps to cell 0 (L - 1 == 0)
ROI_TINY = dict(strides=(8, 16, 32), min_level=3, HWs=[(4, 4), (2, 2), (1, 1)])
ROI_TINY_BOXES = [
    (-208.0, -208.0, 240.0, 240.0),     # sqrt(area) = 448: exactly the threshold of the 1 x 1 level
    (-230.0, -200.0, 260.0, 270.0),     # 1 x 1 level, most samples beyond the validity limit
    (-8.0, -16.0, 500.0, 440.0),        # 1 x 1 level, starts near the cell
    (-112.0, -112.0, 144.0, 144.0),     # 2 x 2 level
    (-60.0, -50.0, 70.0, 90.0),
    (3.0, 5.0, 27.0, 30.0),             # 4 x 4 level
    (-40.0, 4.0, 200.0, 20.0),
    (0.0, 0.0, 32.0, 32.0),
]


def roi_pyramid(name):
    """(scales, min_level, HWs, strides) of inferops_ref's pyramids or of "tiny" (ROI_TINY)."""
    if name == "tiny":
        return [1.0 / s for s in ROI_TINY["strides"]], ROI_TINY["min_level"], list(ROI_TINY["HWs"]), ROI_TINY["strides"]
    scales, min_level, HWs = IR.roi_pyramid(name)
    return scales, min_level, HWs, IR.ROI_PYRAMIDS[name]["strides"]


def roi_bwd_boxes(pyramid, n, seed):
    """n boxes: inferops_ref.roi_boxes (margins kept at every pooled size of ROI_POOLED), ROI_WIDE_BOXES and ROI_EXACT_BOXES in a cycle;
    from n >= 100 on, 40 copies of one small box share their cells.  "tiny": ROI_TINY_BOXES in a cycle."""
    if pyramid == "tiny":
        pool = np.array(ROI_TINY_BOXES, dtype=F32)
        return pool[np.arange(n) % len(pool)].copy()
    fixed = np.array(ROI_WIDE_BOXES + list(IR.ROI_EXACT_BOXES), dtype=F32)
    k = min(max(n - len(fixed), 0), 24)
    rb = IR.roi_boxes(k, seed, pyramid)[0] if k else np.zeros((0, 4), dtype=F32)
    pool = np.concatenate([rb, fixed], 0)
    boxes = pool[np.arange(n) % len(pool)].copy()
    if n >= 100:
        boxes[30:70] = np.array([40.0, 48.0, 72.0, 80.0], dtype=F32)          # 32 x 32, 1/8 px: 40 ROIs on the same cells ...
    return boxes


def roi_decisions_agree(box, scales, min_level, P, HWs):
    """(fp32 decisions == float64 decisions, roi_margins): the level, both grids and the validity of every sample of `box`."""
    b = np.asarray(box, dtype=F32)
    d, e = IR.roi_decisions(b, scales, min_level, P, HWs), IR.roi_decisions(b, scales, min_level, P, HWs, np.float32)
    same = (d["level"] == e["level"] and d["gh"] == e["gh"] and d["gw"] == e["gw"] and np.array_equal(d["vy"], e["vy"])
            and np.array_equal(d["vx"], e["vx"]))
    return same, IR.roi_margins(b, scales, min_level, P, HWs)


def roi_bwd_case(pyramid, P, C, B, n, seed, device="cpu"):
    """(boxes [n,4] f32, bidx [n] i32 with the images interleaved, dout [n, P*P*C] f32, scales, min_level, HWs, strides).  dout carries
    per-channel scales 1e-3..1e3 and per-box scales."""
    scales, min_level, HWs, strides = roi_pyramid(pyramid)
    boxes = roi_bwd_boxes(pyramid, n, seed)
    bidx = (np.arange(n) % B).astype(np.int32)
    if n >= 100:
        bidx[30:70] = 0                                                        # ... of one image
    dout = TR.scaled_inputs((n, P * P, C), seed + 1, per_image=n > 1).reshape(n, P * P * C)
    dout = dout * torch.as_tensor(10.0 ** ((bidx % 3) - 1.0), dtype=torch.float32).view(n, 1)
    return to_t(boxes, device), to_t(bidx, device), dout.to(device), scales, min_level, HWs, strides


ROI_BWD_CASES = [  # (pyramid, pooled, C, B, n)
    ("p3-5", 7, 32, 1, 300), ("p2-5", 8, 20, 3, 300), ("p3-5", 1, 4, 1, 64), ("p2-5", 4, 48, 3, 63), ("p3-5", 14, 132, 1, 1),
    ("p2-5", 16, 32, 3, 20), ("p3-5", 8, 132, 3, 40), ("p2-5", 14, 4, 1, 64),
    ("p2-5", 7, 4, 1, 40), ("tiny", 1, 4, 1, 8), ("tiny", 7, 20, 3, 16), ("tiny", 8, 32, 1, 8),
]
# (B, cap, G, append_gt, P, keys) of the sampling tests, shared by the host and the GPU file
SAMPLE_CASES = [(1, 40, 1, 1, 64, "uniform"), (16, 400, 3, 1, 64, "outside"), (16, 400, 3, 1, 128, "equal"), (2, 4000, 256, 1, 64, "one_bin"),
                (1, 12544, 256, 1, 64, "uniform"), (2, 12800, 1, 0, 0, "equal"), (1, 12800, 1, 0, 64, "outside")]


# ---- coverage ------------------------------------------------------------------------------------------------------------------------
# kernel of csrc/ore_train.hip -> the entry point that launches it and the test of tests/test_hip_trainloss.py that holds it
KERNELS = {
    "k_cn_targets": ("ore_centernet_targets_fwd", "test_centernet_targets"),
    "k_cn_pos_inds": ("ore_centernet_targets_fwd", "test_centernet_targets"),
    "k_cn_loss_partial": ("ore_centernet_losses_fwd", "test_centernet_loss_sums_and_grad"),
    "k_cn_loss_final": ("ore_centernet_losses_fwd", "test_centernet_loss_sums_and_grad"),
    "k_cn_loss_grad": ("ore_centernet_losses_bwd", "test_centernet_loss_sums_and_grad"),
    "k_cn_loss_grad_pos": ("ore_centernet_losses_bwd", "test_centernet_loss_sums_and_grad"),
    "k_roi_losses": ("ore_roi_losses_fwd", "test_roi_losses"),
    "k_sample_rois": ("ore_sample_rois_fwd", "test_sample_rois"),
    "k_sgd_step": ("ore_sgd_step_fwd", "test_sgd_step"),
}
NOT_REACHED = {
    "k_roi_align_bwd launch": "the per-bin kernel's own launch is reachable only through ORE_ROI_BWD_BINS, which the library reads once per "
                              "process; its body roi_bwd_bins runs as the column kernel's fallback (a bin wider than 8 cells: pooled 1)",
    "k_cn_targets MAXN clamp": "gt_count above max_n, or max_n above 128 (the entry point refuses it)",
    "k_cn_loss_partial nb": "more than 65 536 * 2 rows: a third grid-stride trip adds nothing the second does not have",
    "denormal logits": "|logit| > 87 is covered only where the clamp takes over (+-100); no denormal sigmoid reaches a logarithm",
    "k_sample_rois NaN keys": "a NaN key has no defined rank; torch.rand never makes one",
}
