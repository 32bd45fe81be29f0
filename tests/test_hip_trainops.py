"""Every non-conv kernel a training step launches (csrc/ore_bwd.hip, and the forward partners in csrc/ore_misc.hip) against float64.

tests/trainops_ref.py restates each op in float64 together with the same expression over absolute values (mag) and derives the chain
depth d of every kernel; each output here is held to |got - ref| <= 2 d u mag per element and to rms((got - ref) / mag) <=
C_S u sqrt(d) per 16-row x 16-channel block (tests/test_trainops_host.py shows that fp32 emulations in the kernels' order pass both
and that the faults these kernels can have fail them).  Operands carry per-channel scales from 1e-3 to 1e3 and, where an op has
per-image parameters, per-image scales; GroupNorm inputs carry group mean offsets of up to 30 standard deviations; the eSE inputs keep
every pre-activation 1e-3 away from the hard-sigmoid knees.  No element is left out of any comparison.  Every launch runs twice and
the two results are compared bit for bit.

  shape matrix   every TRAIN_OPS class at batch 1 and 16 (test_matrix), through the same runner the production replay uses;
  edge classes   H = 1, W = 1, single pixels, odd sizes, B > 1 with rows per image off the 64 / 256 chunk sizes, C in {4, 20, 112, 128,
                 224, 512}, GroupNorm cpg 1..16 with both statistics kernels, both adaptive-pool kernels, ld > C with coff > 0 (NaN
                 outside the slice) for every entry point that takes them;
  slabs          ore_prod_colsum_fwd at rows {2047, 2048, 6400, 25600} x B {1, 16}, a workspace that caps S, one of exactly B * C;
  autograd nodes each orehip.autograd node of the table end to end, every returned gradient;
  replay         one eager training step at batch 1 and 16 with a spy on the orehip functions of the table: the recorded classes equal
                 TRAIN_OPS, and every recorded signature is re-run on fresh scaled operands.

ORE_TRAINOPS_LOG=<file>: append the worst hard-bound and rms ratios per op to that file."""
import math
import os

import pytest
import torch

import trainops_ref as TR

pytestmark = pytest.mark.gpu

NAN = float("nan")
DEV = "cuda"
_RATIOS = {}        # op -> [worst hard, worst rms, checks]


@pytest.fixture(scope="module")
def oh():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import orehip
    orehip.lib()
    return orehip


@pytest.fixture(scope="module", autouse=True)
def ratio_report(oh):
    yield
    lines = [f"{op:28s} max hard {h:.3e}  max rms {r:.3e}  ({n} checks)" for op, (h, r, n) in sorted(_RATIOS.items())]
    print("\n" + "\n".join(lines))
    log = os.environ.get("ORE_TRAINOPS_LOG")
    if log and lines:
        with open(log, "a") as f:
            f.write("\n".join(lines) + "\n")


def _hold(op, got, ref, mag, d, what):
    """Both checks of trainops_ref on one output; the ratios go to the report before the assertion."""
    assert tuple(got.shape) == tuple(ref.shape), (op, what, got.shape, ref.shape)
    h, r = TR.check2(got, ref, mag, d)
    h0, r0, n0 = _RATIOS.get(op, (0.0, 0.0, 0))
    _RATIOS[op] = (max(h0, h), max(r0, r), n0 + 1)
    assert h <= 1 and r <= 1, (op, what, {"hard": h, "rms": r, "d": d})


def _twice(fn):
    """Run a launch twice; every output must be bit-identical (the kernels claim determinism).  Returns the first result."""
    a, b = fn(), fn()
    ta, tb = (a, b) if isinstance(a, (tuple, list)) else ((a,), (b,))
    for x, y in zip(ta, tb):
        assert torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)), "two identical launches differ"     # bits: NaN borders too
    return a


def _sliced(v, ld, coff):
    """v [..., C] inside a NaN-filled [..., ld] buffer at channel offset coff."""
    buf = torch.full((*v.shape[:-1], ld), NAN, device=v.device)
    buf[..., coff:coff + v.shape[-1]] = v
    return buf


def _hw(rows):
    h = math.isqrt(rows)
    return (h, h) if h * h == rows else (1, rows)


# ---- runners: one TRAIN_OPS class (or an edge class of the same form) through its entry points -----------------------------------
def run_group_norm(oh, cls, seed=0, ld=None, coff=0):
    """ore_groupnorm_affine_fwd (unit affine), ore_groupnorm_apply_fwd, ore_groupnorm_bwd; x a slice [coff, coff + C) of ld floats."""
    B, rpi, C, G, relu = cls
    ld = ld or C
    L, P, S = oh.lib(), oh._ptr, oh._stream()
    xv = TR.gn_inputs(B, rpi, C, G, seed, DEV)
    x = _sliced(xv, ld, coff)
    gamma, beta = TR.scaled_inputs((C,), seed + 1, DEV, -1, 1), TR.scaled_inputs((C,), seed + 2, DEV, -1, 1)
    dy = TR.scaled_inputs((B, rpi, C), seed + 3, DEV, per_image=True)
    one, zero = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)

    def stats():
        r, a = torch.full((B, C), NAN, device=DEV), torch.full((B, C), NAN, device=DEV)
        ws = torch.empty(B * ((rpi + 63) // 64) * G * 2, device=DEV)
        oh._chk(L.ore_groupnorm_affine_fwd(P(x), ld, coff, B, rpi, C, G, 1e-5, P(one), P(zero), P(r), P(a), P(ws), S), "ore_groupnorm_affine_fwd")
        return r, a
    r, a = _twice(stats)
    (rr, rm), (ar, am) = TR.gn_stats(xv, G, 1e-5)
    tag = f"groupnorm/{TR.gn_stats_kernel(C, G)}"
    d = TR.d_gn_stats(rpi, C, G)
    _hold(tag, r, rr, rm, d, ("rstd", cls, ld, coff))
    _hold(tag, a, ar, am, d, ("shift", cls, ld, coff))

    def apply():
        y = torch.full((B, rpi, C), NAN, device=DEV)
        oh._chk(L.ore_groupnorm_apply_fwd(P(x), ld, coff, B, rpi, C, P(r), P(a), P(gamma), P(beta), int(relu), P(y), S), "ore_groupnorm_apply_fwd")
        return y
    y = _twice(apply)
    _hold("groupnorm/apply", y, *TR.gn_apply(xv, r, a, gamma, beta, relu), TR.D_GN_APPLY, (cls, ld, coff))

    def bwd():
        dx, sums = torch.full((B, rpi, C), NAN, device=DEV), torch.full((B, 2 * C), NAN, device=DEV)
        ws = torch.empty(B * rpi * 2 * C + B * ((rpi + 255) // 256) * 2 * C, device=DEV)
        oh._chk(L.ore_groupnorm_bwd(P(dy), P(y), P(x), ld, coff, B, rpi, C, G, P(r), P(a), P(gamma), int(relu), P(dx), P(sums), P(ws),
                                    ws.numel(), S), "ore_groupnorm_bwd")
        return dx, sums
    dx, sums = _twice(bwd)
    ref = TR.gn_bwd(dy, y, xv, r, a, gamma, G, relu)              # the ReLU mask from the product's own y
    dd = TR.d_gn_bwd(rpi, C // G)
    _hold("groupnorm/bwd dx", dx, *ref["dx"], dd["dx"], (cls, ld, coff))
    _hold("groupnorm/bwd dbeta", sums[:, :C], *ref["dbeta"], dd["dbeta"], (cls, ld, coff))
    _hold("groupnorm/bwd dgamma", sums[:, C:], *ref["dgamma"], dd["dgamma"], (cls, ld, coff))


def _prod_colsum_raw(oh, p, q, scale, ws_floats=None):
    """ore_prod_colsum_fwd with a workspace of ws_floats (None: as orehip.prod_colsum sizes it).  The buffer behind the workspace is
    longer and NaN-filled: what lies beyond ws_floats must stay untouched."""
    if ws_floats is None:
        return oh.prod_colsum(p, q, scale)
    B, C = p.shape[0], p.shape[-1]
    rows = p.numel() // (B * C)
    out = torch.full((B, C), NAN, device=DEV)
    ws = torch.full((ws_floats + 4096,), NAN, device=DEV)
    oh._chk(oh.lib().ore_prod_colsum_fwd(oh._ptr(p), oh._ptr(q) if q is not None else None, B, rows, C, scale, oh._ptr(out), oh._ptr(ws),
                                         ws_floats, oh._stream()), "ore_prod_colsum_fwd")
    assert bool(ws[ws_floats:].isnan().all()), "wrote beyond its workspace"
    return out


def run_prod_colsum(oh, B, rows, C, has_q, seed=0, ws_floats=None, op="prod_colsum"):
    p = TR.scaled_inputs((B, rows, C), seed, DEV, per_image=True)
    q = TR.scaled_inputs((B, rows, C), seed + 1, DEV) if has_q else None
    scale = 1.0 if has_q else 1.0 / rows
    got = _twice(lambda: _prod_colsum_raw(oh, p, q, scale, ws_floats))
    S, per = TR.prod_colsum_plan(B, rows, C, 10 ** 12 if ws_floats is None else ws_floats)      # (the wrapper's workspace never caps S)
    _hold(f"{op}/S{'>1' if S > 1 else '=1'}{'/q' if has_q else ''}", got, *TR.prod_colsum(p, q, scale), TR.d_prod_colsum(rows, S, per, has_q),
          (B, rows, C, has_q, S, per))
    return S, per


def run_scale_add(oh, B, rows, C, has_add, seed=0):
    x = TR.scaled_inputs((B, rows, C), seed, DEV, per_image=True)
    s = TR.scaled_inputs((B, C), seed + 1, DEV, -1, 1, per_image=True)
    v = TR.scaled_inputs((B, C), seed + 2, DEV, per_image=True) if has_add else None
    got = _twice(lambda: oh.scale_add_channels(x, s, v))
    _hold("scale_add_channels", got, *TR.scale_add(x, s, v), TR.D_SCALE_ADD, (B, rows, C, has_add))


def run_ese_node(oh, B, H, W, C, seed=0):
    from orehip import autograd as A
    x, w, b = TR.ese_inputs(B, H, W, C, seed, DEV)
    knee = TR.ese_knee_distance(x, w, b)
    assert knee >= TR.ESE_KNEE_MARGIN, knee
    dy = TR.scaled_inputs((B, H, W, C), seed + 1, DEV, per_image=True)
    x, w, b = x.requires_grad_(True), w.requires_grad_(True), b.requires_grad_(True)

    def node():
        y = A.ese(x, w, b)
        return (y.detach(),) + torch.autograd.grad(y, [x, w, b], dy)
    y, dx, dw, db = _twice(node)
    ref = TR.ese_node(x.detach(), w.detach(), b.detach(), dy)
    rows = H * W
    d = TR.d_ese(rows, C, B, TR.prod_colsum_plan(B, rows, C, 10 ** 12), TR.prod_colsum_plan(B, rows, C, 10 ** 12))
    _hold("A.ese y", y, *ref["y"], d["y"], (B, H, W, C))
    _hold("A.ese dx", dx, *ref["dx"], d["dx"], (B, H, W, C))
    _hold("A.ese dW", dw.reshape(C, C), *ref["dW"], d["dW"], (B, H, W, C))
    _hold("A.ese db", db.reshape(1, C), ref["db"][0].reshape(1, C), ref["db"][1].reshape(1, C), d["db"], (B, H, W, C))


def run_ese(oh, cls, seed=0):
    B, rows, C = cls
    for has_q in (False, True):
        run_prod_colsum(oh, B, rows, C, has_q, seed, op="ese/prod_colsum")
        run_scale_add(oh, B, rows, C, has_q, seed)
    run_ese_node(oh, B, *_hw(rows), C, seed)


def _corr_kernels(B, C, per_image, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    ks = (B,) if per_image else ()
    sk = 10.0 ** (torch.rand(*ks, C, generator=g, device=DEV) * 2 - 1)            # per-image, per-channel support kernel scales
    k11 = torch.randn(*ks, C, generator=g, device=DEV) * sk
    k13 = torch.randn(*ks, C, 3, generator=g, device=DEV) * sk.unsqueeze(-1)
    k31 = torch.randn(*ks, C, 3, generator=g, device=DEV) * sk.unsqueeze(-1)
    return k11.contiguous(), k13.contiguous(), k31.contiguous()


def run_correlation(oh, cls, seed=0, ld=None, coff=0):
    """ore_correlation_train_fwd / _bwd; q a slice [coff, coff + C) of ld floats."""
    B, H, W, C, per_image = cls
    ld = ld or C
    L, P, S = oh.lib(), oh._ptr, oh._stream()
    qv = TR.scaled_inputs((B, H, W, C), seed, DEV, per_image=True)
    q = _sliced(qv, ld, coff)
    k11, k13, k31 = _corr_kernels(B, C, per_image, seed + 1)
    dcat = TR.scaled_inputs((B, H, W, 2 * C), seed + 2, DEV, per_image=True)
    rows, Sg = B * H * W, (B if per_image else 1)

    def fwd():
        cat, t, u = (torch.full((B, H, W, n), NAN, device=DEV) for n in (2 * C, C, C))
        oh._chk(L.ore_correlation_train_fwd(P(q), ld, coff, B, H, W, C, P(k11), P(k13), P(k31), int(per_image), P(cat), P(t), P(u), S),
                "ore_correlation_train_fwd")
        return cat, t, u
    cat, t, u = _twice(fwd)
    ref = TR.corr_fwd(qv, k11, k13, k31)
    what = (cls, ld, coff)
    _hold("correlation/fwd cat", cat, *ref["cat"], TR.D_CORR_FWD, what)
    assert torch.equal(cat[..., C:], qv), "the query half of cat is a copy"
    _hold("correlation/fwd t", t, *ref["t"], TR.D_CORR_FWD, what)
    _hold("correlation/fwd u", u, *ref["u"], TR.D_CORR_FWD, what)

    def bwd():
        dq, dk = torch.full((B, H, W, C), NAN, device=DEV), torch.full((Sg, 7, C), NAN, device=DEV)
        ws = torch.empty(rows * C * 8 + Sg * ((rows // Sg + 255) // 256) * 7 * C, device=DEV)
        oh._chk(L.ore_correlation_train_bwd(P(q), ld, coff, B, H, W, C, P(k11), P(k13), P(k31), int(per_image), P(dcat), P(t), P(u), P(dq),
                                            P(dk), P(ws), ws.numel(), S), "ore_correlation_train_bwd")
        return dq, dk
    dq, dk = _twice(bwd)
    rb = TR.corr_bwd(qv, k11, k13, k31, dcat, t, u)                # the masks [t > 0], [u > 0] from the product's own t, u
    d = TR.d_corr_dk(rows // Sg)
    _hold("correlation/bwd dq", dq, *rb["dq"], TR.D_CORR_DQ, what)
    _hold("correlation/bwd dk11", dk[:, 0], *rb["dk11"], d, what)
    for j in range(3):
        _hold("correlation/bwd dk13", dk[:, 1 + j], rb["dk13"][0][..., j], rb["dk13"][1][..., j], d, what + (j,))
        _hold("correlation/bwd dk31", dk[:, 4 + j], rb["dk31"][0][..., j], rb["dk31"][1][..., j], d, what + (j,))


def _maxpool_input(B, H, W, C, seed, quantised):
    x = TR.scaled_inputs((B, H, W, C), seed, DEV)
    if quantised:                                             # few distinct values per channel: most windows hold ties
        s = x.abs().amax((0, 1, 2)).clamp(min=1e-30) / 3
        x = (x / s).round() * s
    return x


def run_maxpool(oh, cls, seed=0, ld=None, coff=0):
    """ore_maxpool3x3s2_fwd (exact; in / out as slices of wider NaN-filled buffers) and ore_maxpool3x3s2_bwd."""
    B, H, W, C = cls
    ld = ld or C
    Ho, Wo = TR.maxpool_out_hw(H, W)
    assert (Ho, Wo) == oh.maxpool3x3s2_out_hw(H, W)
    for quantised in (True, False):
        xv = _maxpool_input(B, H, W, C, seed, quantised)
        x = _sliced(xv, ld, coff)

        def fwd():
            out = torch.full((B, Ho, Wo, ld), NAN, device=DEV)
            oh._chk(oh.lib().ore_maxpool3x3s2_fwd(oh._ptr(x), ld, coff, B, H, W, C, None, oh._ptr(out), ld, coff, oh._stream()), "ore_maxpool3x3s2_fwd")
            return out
        out = _twice(fwd)
        assert torch.equal(out[..., coff:coff + C], TR.maxpool_fwd(xv)), (cls, quantised)
        assert bool(out[..., :coff].isnan().all()) and bool(out[..., coff + C:].isnan().all()), "wrote outside its slice"
        ones = torch.ones(B, Ho, Wo, C, device=DEV)
        cnt = _twice(lambda: oh.maxpool3x3s2_bwd(xv, ones))                          # windows owned per pixel: the ownership pattern
        assert torch.equal(cnt.double(), TR.maxpool_bwd(xv, ones)[0]), ("ownership", cls, quantised)
        assert float(cnt.sum()) == B * Ho * Wo * C
        dy = TR.scaled_inputs((B, Ho, Wo, C), seed + 1, DEV, per_image=True)
        dx = _twice(lambda: oh.maxpool3x3s2_bwd(xv, dy))
        _hold("maxpool/bwd", dx, *TR.maxpool_bwd(xv, dy), TR.D_MAXPOOL_BWD, (cls, quantised))


def run_sumpool(oh, cls, seed=0, ld=None, coff=0):
    B, H, W, C = cls
    ld = ld or C
    xv = TR.scaled_inputs((B, H, W, C), seed, DEV, per_image=True)
    x = _sliced(xv, ld, coff)

    def go():
        out = torch.full((B, (H + 1) // 2, (W + 1) // 2, C), NAN, device=DEV)
        # the entry point takes ld only: a slice starts at the pointer of its first channel
        oh._chk(oh.lib().ore_sumpool2x2_fwd(oh._ptr(x) + 4 * coff, ld, B, H, W, C, oh._ptr(out), oh._stream()), "ore_sumpool2x2_fwd")
        return out
    _hold("sumpool2x2", _twice(go), *TR.sumpool2(xv), TR.D_SUMPOOL, (cls, ld, coff))


def run_apool(oh, cls, seed=0):
    B, H, W, C, OH, OW = cls
    x = TR.scaled_inputs((B, H, W, C), seed, DEV, per_image=True)
    y = _twice(lambda: oh.adaptive_avgpool_nhwc(x, OH, OW))
    _hold(f"adaptive_avgpool/{TR.apool_kernel(H, W, C, OH, OW)}", y, *TR.apool_fwd(x, OH, OW), TR.d_apool(H, W, C, OH, OW), cls)
    dy = TR.scaled_inputs((B, OH, OW, C), seed + 1, DEV, per_image=True)
    dx = _twice(lambda: oh.adaptive_avgpool_nhwc(dy, OH, OW, grad_of=(H, W)))
    _hold("adaptive_avgpool/bwd", dx, *TR.apool_bwd(dy, H, W), TR.d_apool_bwd(H, W, OH, OW), cls)


def run_group_mean(oh, cls, seed=0):
    G, N, M = cls
    x = TR.scaled_inputs((G * N, M // 128, 128), seed, DEV, per_image=True) if M % 128 == 0 else TR.scaled_inputs((G * N, M), seed, DEV)
    y = _twice(lambda: oh.group_mean(x, G))
    _hold("group_mean/fwd", y, *TR.group_mean(x, G), TR.d_group_mean(N), cls)
    dy = TR.scaled_inputs(tuple(y.shape), seed + 1, DEV, per_image=True)
    dx = _twice(lambda: oh.group_mean(dy, G, backward=True, members=N))
    if N & (N - 1) == 0:
        assert torch.equal(dx, (dy / N).repeat_interleave(N, 0)), cls          # a power of two: exact
    else:
        _hold("group_mean/bwd", dx, *TR.group_mean_bwd(dy, G, N), 2, cls)


def run_sm_permute(oh, cls, seed=0, variants=None):
    """Both axes, both directions, and the accumulating form (the second gradient of SmDualPermuteFn): exact."""
    B, H, W, G, S = cls
    x = TR.scaled_inputs((B, H, W, G * S), seed, DEV, per_image=True)
    for axis, inverse, accumulate in variants or [(a, i, c) for a in "hw" for i in (False, True) for c in (False, True)]:
        want = TR.sm_permute(x, B, H, W, G, S, axis, inverse)
        if not accumulate:
            got = _twice(lambda: oh.sm_permute(x, B, H, W, G, S, axis, inverse))
            assert torch.equal(got.reshape(-1), want.reshape(-1)), (cls, axis, inverse)
            continue
        base = TR.scaled_inputs(tuple(want.shape), seed + 1, DEV)

        def acc():
            out = base.clone()
            oh.sm_permute(x, B, H, W, G, S, axis, inverse, out=out, accumulate=True)
            return out
        assert torch.equal(_twice(acc).reshape(-1), (base + want).reshape(-1)), (cls, axis, inverse, "accumulate")     # one correctly rounded fp32 addition


def run_mean_pair(oh, cls, seed=0):
    from orehip import autograd as A
    B, rows, C = cls
    h = TR.scaled_inputs((B, *_hw(rows), C), seed, DEV, per_image=True).requires_grad_(True)
    w = TR.scaled_inputs((B, *_hw(rows), C), seed + 1, DEV, per_image=True).requires_grad_(True)
    dm = TR.scaled_inputs((B, C), seed + 2, DEV)

    def node():
        m = A.mean_pair(h, w)
        gh, gw = torch.autograd.grad(m, [h, w], dm)
        return m.detach(), gh.contiguous(), gw.contiguous()
    m, gh, gw = _twice(node)
    S, per = TR.prod_colsum_plan(B, rows, C, 10 ** 12)
    _hold("A.mean_pair", m, *TR.mean_pair(h.detach(), w.detach()), TR.d_prod_colsum(rows, S, per, False) + 1, cls)
    want = (dm / rows).view(B, 1, 1, C).expand_as(gh)                  # one correctly rounded division, the same for every pixel
    assert torch.equal(gh, want) and torch.equal(gw, want), cls


def run_combine2(oh, cls, seed=0):
    from orehip import autograd as A
    B, rows, C = cls
    shape = (B, *_hw(rows), C)
    w, h = (TR.scaled_inputs(shape, seed + i, DEV, per_image=True) for i in (0, 1))
    a0, a1, v = (TR.scaled_inputs((B, C), seed + i, DEV, -1, 1, per_image=True) for i in (2, 3, 4))
    dy = TR.scaled_inputs(shape, seed + 5, DEV, per_image=True)
    _hold("combine2/fwd", _twice(lambda: oh.combine2(w, h, a0, a1)), *TR.combine2(w, h, a0, a1), TR.D_COMBINE2, cls)
    for add in (None, v):
        dw, dh = _twice(lambda: oh.combine2_bwd(dy, a0, a1, add))
        (rw, mw), (rh, mh) = TR.combine2_bwd(dy, a0, a1, add)
        _hold("combine2/bwd", dw, rw, mw, TR.D_COMBINE2_BWD, (cls, add is not None))
        _hold("combine2/bwd", dh, rh, mh, TR.D_COMBINE2_BWD, (cls, add is not None))
    # the node end to end: the gradients of a0 / a1 are per-image column sums of dy * w, dy * h
    ins = [t.clone().requires_grad_(True) for t in (w, h, a0, a1)]

    def node():
        y = A.combine2(*ins)
        return (y.detach(),) + torch.autograd.grad(y, ins, dy)
    y, gw, gh, g0, g1 = _twice(node)
    S, per = TR.prod_colsum_plan(B, rows, C, 10 ** 12)
    d = TR.d_prod_colsum(rows, S, per, True)
    _hold("A.combine2 da", g0, *TR.prod_colsum(dy, w, 1.0), d, cls)
    _hold("A.combine2 da", g1, *TR.prod_colsum(dy, h, 1.0), d, cls)
    (rw, mw), (rh, mh) = TR.combine2_bwd(dy, a0, a1)
    _hold("A.combine2 dw", gw, rw, mw, TR.D_COMBINE2_BWD, cls)
    _hold("A.combine2 dw", gh, rh, mh, TR.D_COMBINE2_BWD, cls)


RUNNERS = {"group_norm_relu": run_group_norm, "ese": run_ese, "maxpool": run_maxpool, "sumpool2x2": run_sumpool, "sm_permute": run_sm_permute,
           "mean_pair": run_mean_pair, "combine2": run_combine2, "group_mean": run_group_mean, "adaptive_avg_pool": run_apool,
           "correlation_cat": run_correlation}


# ---- shape matrix ----------------------------------------------------------------------------------------------------------------
def _matrix():
    out = []
    for op, (_, classes) in sorted(TR.TRAIN_OPS.items()):
        for cls in classes:
            out += [(op, "bs1", cls), (op, "bs16", TR.batch16(op, cls))]
    return out


@pytest.mark.parametrize("op,lab,cls", _matrix())
def test_matrix(oh, op, lab, cls):
    RUNNERS[op](oh, cls, seed=sum(cls) % 1000)
    torch.cuda.empty_cache()


# ---- edge classes ----------------------------------------------------------------------------------------------------------------
# (B, rows per image, C, groups): cpg 1, 2, 4 (both k_gn_chunk_stats4 builds), 8, 16; one pixel; below one chunk; off the chunk sizes
GN_EDGES = [(3, 100, 64, 64), (2, 357, 128, 64), (3, 77, 64, 16), (2, 700, 128, 32), (2, 190, 128, 16), (2, 45, 256, 16), (5, 1, 128, 32),
            (2, 63, 128, 32), (3, 65, 32, 8), (2, 257, 16, 16), (4, 1, 4, 1)]


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("sliced", [False, True])
@pytest.mark.parametrize("B,rpi,C,G", GN_EDGES)
def test_groupnorm_edges(oh, B, rpi, C, G, relu, sliced):
    run_group_norm(oh, (B, rpi, C, G, relu), seed=rpi + G, ld=C + 40 if sliced else None, coff=12 if sliced else 0)


def test_groupnorm_statistics_kernels_both_reached():
    ks = {TR.gn_stats_kernel(C, G) for _, _, C, G in GN_EDGES}
    assert ks == {"k_gn_chunk_stats4", "k_gn_chunk_stats"}, ks
    assert {C // G for _, _, C, G in GN_EDGES} >= {1, 2, 4, 8, 16}


C_EDGES = [4, 20, 112, 128, 224, 512]
MAP_EDGES = [(2, 1, 37), (2, 29, 1), (5, 1, 1), (3, 13, 11), (4, 15, 17), (2, 6, 4), (3, 4, 7), (2, 2, 2)]      # (B, H, W)


@pytest.mark.parametrize("sliced", [False, True])
@pytest.mark.parametrize("i", range(len(MAP_EDGES)))
def test_map_op_edges(oh, i, sliced):
    """Correlation, max-pool and 2x2 sum-pool over one image row / column, single pixels, odd sizes whose ceil-mode last window is one
    row or column with B > 1, each with a channel count of C_EDGES; dense and as slices of wider NaN-filled rows."""
    B, H, W = MAP_EDGES[i]
    C = C_EDGES[i % len(C_EDGES)]
    ld, coff = (C + 24, 8) if sliced else (None, 0)
    for per_image in (True, False):
        run_correlation(oh, (B, H, W, C, per_image), seed=i, ld=ld, coff=coff)
    run_maxpool(oh, (B, H, W, C), seed=i, ld=ld, coff=coff)
    run_sumpool(oh, (B, H, W, C), seed=i, ld=ld, coff=coff)


@pytest.mark.parametrize("C", C_EDGES)
def test_channel_edges(oh, C):
    """Every channel-tiled kernel at channel counts that leave its 64-channel column blocks / 256 / (C / 4) slices partly empty."""
    run_correlation(oh, (2, 9, 7, C, True), seed=C)
    run_maxpool(oh, (2, 9, 7, C), seed=C)
    for B, rows in ((3, 357), (2, 63), (2, 700)):
        for has_q in (False, True):
            run_prod_colsum(oh, B, rows, C, has_q, seed=C + rows)
            run_scale_add(oh, B, rows, C, has_q, seed=C + rows)
        run_combine2(oh, (B, rows, C), seed=C)
    run_apool(oh, (2, 32, 32, C, 1, 3), seed=C)                   # k_apool_fwd_big
    run_apool(oh, (2, 7, 11, C, 3, 4), seed=C)                    # k_apool_fwd
    run_group_mean(oh, (3, 5, 7 * C), seed=C)
    run_group_mean(oh, (2, 8, 3 * C), seed=C)                     # N a power of two: the backward is exact


# (B, H, W, C, OH, OW): up- and down-sampling with non-divisible sizes, both sides of the bin >= 64 switch
APOOL_EDGES = [(3, 30, 30, 16, 32, 32), (2, 15, 15, 8, 16, 16), (2, 7, 11, 4, 3, 5), (1, 5, 5, 4, 9, 12), (2, 18, 18, 20, 3, 3),
               (2, 20, 20, 20, 3, 3), (2, 1, 1, 128, 3, 3), (2, 1, 40, 128, 1, 1), (3, 33, 1, 128, 2, 1), (2, 31, 29, 224, 1, 1)]


@pytest.mark.parametrize("cls", APOOL_EDGES)
def test_apool_edges(oh, cls):
    run_apool(oh, cls, seed=sum(cls))


def test_apool_both_kernels_reached():
    ks = [TR.apool_kernel(H, W, C, OH, OW) for _, H, W, C, OH, OW in APOOL_EDGES]
    assert set(ks) == {"k_apool_fwd_big", "k_apool_fwd"}
    assert TR.apool_kernel(20, 20, 20, 3, 3) == "k_apool_fwd_big" and TR.apool_kernel(18, 18, 20, 3, 3) == "k_apool_fwd"      # bin 64 / 49


@pytest.mark.parametrize("segments", [1, 16])
@pytest.mark.parametrize("rps", [6400, 1600, 400, 1024, 256, 64, 357, 63, 1])
def test_colsum_segments(oh, segments, rps):
    """The segmented column sums at the production rows per image, below one chunk and off the chunk size; each segment's sums are
    bitwise those of ore_colsum_fwd on that segment alone."""
    C = C_EDGES[(rps + segments) % len(C_EDGES)]
    x = TR.scaled_inputs((segments * rps, C), rps + segments, DEV)
    got = _twice(lambda: oh.colsum_segments(x, segments))
    _hold("colsum_segments", got, *TR.colsum(x, segments), TR.d_colsum(rps), (segments, rps, C))
    for s in (0, segments - 1):
        assert torch.equal(got[s], oh.colsum(x[s * rps:(s + 1) * rps].contiguous())), (segments, rps, s)


@pytest.mark.parametrize("rows,ld,coff,Cc", [(700, 224, 32, 112), (6400, 128, 0, 128), (63, 40, 20, 20), (2049, 516, 4, 512), (1, 8, 4, 4)])
def test_colsum_slices_and_beta(oh, rows, ld, coff, Cc):
    x = _sliced(TR.scaled_inputs((rows, Cc), rows, DEV), ld, coff)
    xv = x[:, coff:coff + Cc]
    _hold("colsum", _twice(lambda: oh.colsum(x, coff=coff, Cc=Cc)).reshape(1, Cc), *TR.colsum(xv), TR.d_colsum(rows), (rows, ld, coff, Cc))
    old = TR.scaled_inputs((1, Cc), rows + 1, DEV)

    def acc():
        out = old[0].clone()
        oh.colsum(x, coff=coff, Cc=Cc, out=out, beta=0.75)
        return out
    _hold("colsum/beta", _twice(acc).reshape(1, Cc), *TR.colsum(xv, 1, 0.75, old), TR.d_colsum(rows, True), (rows, ld, coff, Cc))


# ---- ore_prod_colsum_fwd: the slab forms ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("has_q", [False, True])
@pytest.mark.parametrize("B", [1, 16])
@pytest.mark.parametrize("rows", [2047, 2048, 6400, 25600])
def test_prod_colsum_slabs(oh, rows, B, has_q):
    S, per = run_prod_colsum(oh, B, rows, 112, has_q, seed=rows + B)
    assert (S > 1) == (rows >= 2048), (rows, B, S, per)
    torch.cuda.empty_cache()


@pytest.mark.parametrize("has_q", [False, True])
def test_prod_colsum_capped_workspace(oh, has_q):
    """A workspace that holds fewer [B][C] partial sums than the natural slab count caps S; one of exactly B * C floats leaves S = 1.
    What lies behind the workspace stays untouched, and the result meets the bounds with d from the S of the restated formula."""
    assert TR.prod_colsum_plan(1, 25600, 112, 10 ** 12)[0] == 50
    S, per = run_prod_colsum(oh, 1, 25600, 112, has_q, seed=1, ws_floats=7 * 112 + 50)
    assert (S, per) == (7, 3712)
    S, per = run_prod_colsum(oh, 16, 6400, 112, has_q, seed=2, ws_floats=16 * 112)
    assert (S, per) == (1, 6400)
    S, per = run_prod_colsum(oh, 2, 6400, 224, has_q, seed=3, ws_floats=3 * 2 * 224 + 1)
    assert (S, per) == (3, 2176)


# ---- autograd nodes end to end ---------------------------------------------------------------------------------------------------
def test_node_group_norm_relu(oh):
    """A.group_norm_relu at the p4 tower map: the statistics are the node's own, so the reference is float64 GroupNorm from x and the
    depth is the sum over the node's kernels."""
    from orehip import autograd as A
    B, rpi, C, G = 2, 1600, 128, 32
    x = TR.gn_inputs(B, rpi, C, G, 11, DEV).reshape(B, 40, 40, C).requires_grad_(True)
    gamma = TR.scaled_inputs((C,), 12, DEV, -1, 1).requires_grad_(True)
    beta = TR.scaled_inputs((C,), 13, DEV, -1, 1).requires_grad_(True)
    dy = TR.scaled_inputs((B, 40, 40, C), 14, DEV, per_image=True)

    def node():
        y = A.group_norm_relu(x, gamma, beta, G, 1e-5, True)
        return (y.detach(),) + torch.autograd.grad(y, [x, gamma, beta], dy)
    y, dx, dgamma, dbeta = _twice(node)
    xr = x.detach().reshape(B, rpi, C)
    (r, _), (a, am) = TR.gn_stats(xr, G, 1e-5)
    ds = TR.d_gn_stats(rpi, C, G)
    # mag of the node: the float64 statistics enter as |r| and the absolute-value form of a (mean |x| * r)
    yr, _ = TR.gn_apply(xr, r, a, gamma.detach(), beta.detach(), True)
    _, ym = TR.gn_apply(xr, r, am, gamma.detach(), beta.detach(), True)
    _hold("A.group_norm_relu y", y.reshape(B, rpi, C), yr, ym, ds + TR.D_GN_APPLY, "y")
    ref = TR.gn_bwd(dy.reshape(B, rpi, C), y.reshape(B, rpi, C), xr, r, a, gamma.detach(), G, True)
    mags = TR.gn_bwd(dy.reshape(B, rpi, C), y.reshape(B, rpi, C), xr, r, am, gamma.detach(), G, True)
    dd = TR.d_gn_bwd(rpi, C // G)
    _hold("A.group_norm_relu dx", dx.reshape(B, rpi, C), ref["dx"][0], mags["dx"][1], ds + dd["dx"], "dx")
    _hold("A.group_norm_relu dgamma", dgamma.reshape(1, C), ref["dgamma"][0].sum(0, True), mags["dgamma"][1].sum(0, True), ds + dd["dgamma"] + B, "dgamma")
    _hold("A.group_norm_relu dbeta", dbeta.reshape(1, C), ref["dbeta"][0].sum(0, True), mags["dbeta"][1].sum(0, True), dd["dbeta"] + B, "dbeta")


def test_node_pools_and_means(oh):
    """A.maxpool, A.adaptive_avg_pool, A.group_mean, A.sm_dual_permute at one production shape each."""
    from orehip import autograd as A
    x = _maxpool_input(24, 16, 16, 384, 21, True).requires_grad_(True)
    dy = TR.scaled_inputs((24, 8, 8, 384), 22, DEV, per_image=True)
    y = A.maxpool(x)
    dx, = torch.autograd.grad(y, [x], dy)
    assert torch.equal(y.detach(), TR.maxpool_fwd(x.detach()))
    _hold("A.maxpool dx", dx, *TR.maxpool_bwd(x.detach(), dy), TR.D_MAXPOOL_BWD, "maxpool")
    for OH, OW in ((1, 1), (3, 1), (1, 3)):
        p = TR.scaled_inputs((16, 32, 32, 128), 23, DEV, per_image=True).requires_grad_(True)
        dk = TR.scaled_inputs((16, OH, OW, 128), 24, DEV, per_image=True)
        k = A.adaptive_avg_pool(p, OH, OW)
        dp, = torch.autograd.grad(k, [p], dk)
        _hold("A.adaptive_avg_pool y", k.detach(), *TR.apool_fwd(p.detach(), OH, OW), TR.d_apool(32, 32, 128, OH, OW), (OH, OW))
        _hold("A.adaptive_avg_pool dx", dp, *TR.apool_bwd(dk, 32, 32), TR.d_apool_bwd(32, 32, OH, OW), (OH, OW))
    s = TR.scaled_inputs((48, 16, 16, 128), 25, DEV, per_image=True).requires_grad_(True)
    dm = TR.scaled_inputs((2, 16, 16, 128), 26, DEV, per_image=True)
    m = A.group_mean(s, 2)
    ds, = torch.autograd.grad(m, [s], dm)
    _hold("A.group_mean y", m.detach(), *TR.group_mean(s.detach(), 2), TR.d_group_mean(24), "group_mean")
    _hold("A.group_mean dx", ds, *TR.group_mean_bwd(dm, 2, 24), 2, "group_mean")
    dims = (24, 16, 16, 16, 8)
    v = TR.scaled_inputs((24, 16, 16, 128), 27, DEV, per_image=True).requires_grad_(True)
    xh, xw = A.sm_dual_permute(v, dims)
    assert torch.equal(xh.detach().reshape(-1), TR.sm_permute(v.detach(), *dims, "h", False).reshape(-1))
    assert torch.equal(xw.detach().reshape(-1), TR.sm_permute(v.detach(), *dims, "w", False).reshape(-1))
    gh, gw = TR.scaled_inputs(tuple(xh.shape), 28, DEV), TR.scaled_inputs(tuple(xw.shape), 29, DEV)
    dv, = torch.autograd.grad([xh, xw], [v], [gh, gw])
    want = TR.sm_permute(gh, *dims, "h", True).reshape(v.shape) + TR.sm_permute(gw, *dims, "w", True).reshape(v.shape)
    assert torch.equal(dv, want)


def test_node_correlation_cat(oh):
    from orehip import autograd as A
    B, H, W, C = 2, 40, 40, 128
    q = TR.scaled_inputs((B, H, W, C), 31, DEV, per_image=True).requires_grad_(True)
    ks = [k.requires_grad_(True) for k in _corr_kernels(B, C, True, 32)]
    dcat = TR.scaled_inputs((B, H, W, 2 * C), 33, DEV, per_image=True)

    def node():
        cat = A.correlation_cat(q, *ks)
        return (cat.detach(),) + torch.autograd.grad(cat, [q] + ks, dcat)
    cat, dq, d11, d13, d31 = _twice(node)
    kd = [k.detach() for k in ks]
    f = TR.corr_fwd(q.detach(), *kd)
    _hold("A.correlation_cat y", cat, *f["cat"], TR.D_CORR_FWD, "cat")
    _, t, u = oh.correlation_train_fwd(q.detach(), *kd)            # the node's saved t, u (bit-identical launches): the masks
    rb = TR.corr_bwd(q.detach(), *kd, dcat, t, u)
    d = TR.d_corr_dk(H * W)
    _hold("A.correlation_cat dq", dq, *rb["dq"], TR.D_CORR_DQ, "dq")
    _hold("A.correlation_cat dk", d11, *rb["dk11"], d, "dk11")
    for j in range(3):
        _hold("A.correlation_cat dk", d13[..., j], rb["dk13"][0][..., j], rb["dk13"][1][..., j], d, ("dk13", j))
        _hold("A.correlation_cat dk", d31[..., j], rb["dk31"][0][..., j], rb["dk31"][1][..., j], d, ("dk31", j))


# ---- production replay -----------------------------------------------------------------------------------------------------------
def _train_step(oh, batch, spies):
    """One eager training step of configs/fsod/finetune_vovnet.yaml over `batch` 640 x 640 query images with 24 support crops each
    (the model construction of tests/test_hip_dgrad.py::_spy_step), with `spies` {name: wrapper factory} installed on orehip."""
    from conftest import PKG
    from detectron2.modeling import build_model
    from detectron2.structures import Boxes, Instances
    from fewx.config import get_cfg
    from fewx.modeling.fsod.train_forward import train_forward
    from fewx.solver.build import get_bucket
    from oracle import ref_model as R
    from oracle import ref_train as T
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(PKG, "configs", "fsod", "finetune_vovnet.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", "cuda", "INPUT.FS.SUPPORT_SHOT", 24])
    cfg.freeze()
    torch.manual_seed(0)
    m = build_model(cfg)
    m.load_state_dict(R.synth_roi_state(R.synth_state_dict(0), 0), strict=False)
    m.train()
    get_bucket(m, cfg)
    data = []
    for b in range(batch):
        img, gt, sup, sbox = T.synth_train_inputs(40 + b, (640, 640), n_gt=15 + b % 6, shots=24, support_hw=240)
        inst = Instances((640, 640))
        inst.gt_boxes, inst.gt_classes = Boxes(gt), torch.zeros(len(gt), dtype=torch.int64)
        data.append({"image": img, "instances": inst, "support_images": sup, "support_bboxes": sbox.numpy()})
    real = {name: getattr(oh, name) for name in spies}
    for name, make in spies.items():
        setattr(oh, name, make(real[name]))
    try:
        losses = train_forward(m, data)
        sum(losses.values()).backward()
        torch.cuda.synchronize()
    finally:
        for name, fn in real.items():
            setattr(oh, name, fn)
    del m


def _spies(rec, relu_calls):
    """Wrapper factories that record the call class of every covered orehip function under its TRAIN_OPS op."""
    def rows_of(t):
        return t.numel() // (t.shape[0] * t.shape[-1])

    def note(op, fn_name, cls):
        rec.setdefault(op, {}).setdefault(tuple(cls), set()).add(fn_name)

    def spy(name, classify):
        def make(real):
            def f(*a, **kw):
                classify(*a, **kw)
                return real(*a, **kw)
            return f
        return name, make

    def prod(p, q=None, scale=1.0):
        C = p.shape[-1]
        op = "ese" if C in (384, 512) else ("combine2" if q is not None else "mean_pair")
        note(op, "prod_colsum", (p.shape[0], rows_of(p), C))

    def maxpool_fwd(x, in_mul=None, out=None, out_coff=0):
        if in_mul is None and out is None and x.dtype == torch.float32:
            note("_maxpool_fwd", "maxpool3x3s2", tuple(x.shape))   # (the frozen seam pools too, without a backward: matched up after the step)

    def relu(dy, y, scale=None, *, dy_coff=0, y_coff=0, Cc=None, out=None, out_coff=0):
        relu_calls.add((y.numel() // y.shape[-1], dy.shape[-1], dy_coff, y.shape[-1], y_coff, Cc if Cc is not None else y.shape[-1] - y_coff,
                        scale is not None))

    return dict([
        spy("groupnorm_affine", lambda x, groups, *a, **k: note("group_norm_relu", "groupnorm_affine", (x.shape[0], rows_of(x), x.shape[-1], groups, True))),
        spy("groupnorm_apply", lambda x, r, a, g, b, relu: note("group_norm_relu", "groupnorm_apply", (x.shape[0], rows_of(x), x.shape[-1], 32, bool(relu)))),
        spy("groupnorm_bwd", lambda dy, y, x, groups, r, a, g, relu: note("group_norm_relu", "groupnorm_bwd", (x.shape[0], rows_of(x), x.shape[-1], groups, bool(relu)))),
        spy("prod_colsum", prod),
        spy("scale_add_channels", lambda x, s, v=None: note("ese", "scale_add_channels", (x.shape[0], rows_of(x), x.shape[-1]))),
        spy("maxpool3x3s2", maxpool_fwd),
        spy("maxpool3x3s2_bwd", lambda x, dy: note("maxpool", "maxpool3x3s2_bwd", tuple(x.shape))),
        spy("sumpool2x2", lambda x: note("sumpool2x2", "sumpool2x2", tuple(x.shape))),
        spy("sm_permute", lambda x, B, H, W, G, S, axis, inverse, out=None, accumulate=False: note("sm_permute", (axis, inverse, accumulate), (B, H, W, G, S))),
        spy("combine2", lambda w, h, a0, a1: note("combine2", "combine2", (w.shape[0], rows_of(w), w.shape[-1]))),
        spy("combine2_bwd", lambda dy, a0, a1, add_bc=None: note("combine2", "combine2_bwd", (dy.shape[0], rows_of(dy), dy.shape[-1]))),
        spy("group_mean", lambda x, groups, backward=False, members=0: note(
            "group_mean", "group_mean", (groups, members if backward else x.shape[0] // groups, x.numel() // (groups if backward else x.shape[0])))),
        spy("adaptive_avgpool_nhwc", lambda x, OH, OW, grad_of=None: note(
            "adaptive_avg_pool", "adaptive_avgpool_nhwc", (x.shape[0], *(grad_of or x.shape[1:3]), x.shape[-1], OH, OW))),
        spy("correlation_train_fwd", lambda q, k11, k13, k31: note("correlation_cat", "correlation_train_fwd", (*q.shape, int(k11.dim() == 2)))),
        spy("correlation_train_bwd", lambda q, k11, *a: note("correlation_cat", "correlation_train_bwd", (*q.shape, int(k11.dim() == 2)))),
        spy("relu_affine_bwd", relu),
    ])


@pytest.mark.parametrize("batch", [1, 16])
def test_production_replay(oh, batch):
    rec, relu_calls = {}, set()
    _train_step(oh, batch, _spies(rec, relu_calls))
    torch.cuda.empty_cache()
    fwd_pools = rec.pop("_maxpool_fwd", {})
    for cls in rec.get("maxpool", {}):
        assert cls in fwd_pools, ("a max-pool backward without its forward", cls)
        rec["maxpool"][cls].add("maxpool3x3s2")
    want = {op: {(c if batch == 1 else TR.batch16(op, c)) for c in classes} for op, (_, classes) in TR.TRAIN_OPS.items() if classes}
    got = {op: set(classes) for op, classes in rec.items()}
    print(f"\nbs{batch} recorded call classes:")
    for op in sorted(got):
        print(f"  {op}: {sorted(got[op])}")
    print(f"  relu_affine_bwd: {len(relu_calls)} distinct signatures")
    extra = {op: sorted(got.get(op, set()) - want.get(op, set())) for op in got if got.get(op, set()) - want.get(op, set())}
    lack = {op: sorted(want[op] - got.get(op, set())) for op in want if want[op] - got.get(op, set())}
    print(f"  recorded but not in TRAIN_OPS: {extra}\n  in TRAIN_OPS but not recorded: {lack}")
    assert not extra, extra
    assert not lack, lack
    for op, (fns, _) in TR.TRAIN_OPS.items():                     # every function of the table was reached through its op
        if op in rec and op != "sm_permute":
            seen = set().union(*rec[op].values())
            assert set(fns) <= seen, (op, sorted(set(fns) - seen))
    # every recorded signature again, on fresh scaled operands of the same shape
    for i, op in enumerate(sorted(got)):
        for cls in sorted(got[op]):
            if op == "sm_permute":
                run_sm_permute(oh, cls, seed=900 + i, variants=sorted(rec[op][cls]))
            else:
                RUNNERS[op](oh, cls, seed=900 + i)
            torch.cuda.empty_cache()
    assert relu_calls, "no relu_affine_bwd call recorded"
    g = torch.Generator(device=DEV).manual_seed(5)
    for rows, dld, dc, yld, yc, Cc, has_scale in sorted(relu_calls):
        dy, y = torch.full((rows, dld), NAN, device=DEV), torch.full((rows, yld), NAN, device=DEV)
        dv = TR.scaled_inputs((rows, Cc), rows % 1000 + Cc, DEV)
        yv = torch.randn(rows, Cc, generator=g, device=DEV)
        yv[yv.abs() < 0.3] = 0.0
        dy[:, dc:dc + Cc], y[:, yc:yc + Cc] = dv, yv
        scale = torch.rand(Cc, generator=g, device=DEV) + 0.5 if has_scale else None
        res = oh.relu_affine_bwd(dy, y, scale, dy_coff=dc, y_coff=yc, Cc=Cc)
        assert torch.equal(res, torch.where(yv > 0, dv * scale if has_scale else dv, torch.zeros_like(yv))), (rows, dld, dc, yld, yc, Cc)
