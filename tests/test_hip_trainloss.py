"""The nine kernels of csrc/ore_train.hip against float64 (tests/trainloss_ref.py; tests/test_trainloss_host.py shows on the CPU that the
references are the operations they name, that fp32 emulations pass and that the faults these kernels can have fail).

Every floating output is held to |got - ref| <= 2 d u mag per element and to the 16 x 16 block rms bound; integer outputs, copies and
selections are compared exactly; no element is left out.  Every launch runs twice and is compared bit for bit.  Outputs start NaN-filled
where the entry point writes every element; head / dhead also run as 5 columns of a 16-column NaN-filled buffer whose other columns
must not change.  The three launch forms of ROIAlign backward (tiled gather, fixed-point atomics, fp32 atomics) are held to the transpose
of the forward reference, each with its own depth.  The shapes are the smallest that reach each branch (trainloss_ref.NOT_REACHED lists
what is left out on purpose).

ORE_TRAINLOSS_LOG=<file>: append the worst hard-bound and rms ratios per op to that file."""
import os

import numpy as np
import pytest
import torch

import trainloss_ref as TL

pytestmark = pytest.mark.gpu

NAN = float("nan")
DEV = "cuda"
_RATIOS = {}


@pytest.fixture(scope="module")
def oh():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import orehip
    orehip.lib()
    return orehip


@pytest.fixture(scope="module", autouse=True)
def ratio_report(oh):
    yield
    lines = [f"{op:34s} max hard {h:.3e}  max rms {r:.3e}  ({n} checks)" for op, (h, r, n) in sorted(_RATIOS.items())]
    print("\n" + "\n".join(lines))
    print("re-drawn inputs (drawn, re-drawn):", {k: tuple(v) for k, v in TL.REDRAWS.items()})
    log = os.environ.get("ORE_TRAINLOSS_LOG")
    if log and lines:
        with open(log, "a") as f:
            f.write("\n".join(lines) + "\n")


def _hold(op, got, x, what):
    h, r = TL.hold(got, x)
    h0, r0, n0 = _RATIOS.get(op, (0.0, 0.0, 0))
    _RATIOS[op] = (max(h0, h), max(r0, r), n0 + 1)
    print(f"{op} {what}: hard {h:.3e} rms {r:.3e} d {x.d}")
    assert h <= 1 and r <= 1, (op, what, {"hard": h, "rms": r, "d": x.d})


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _twice(fn):
    a, b = fn(), fn()
    ta, tb = (a, b) if isinstance(a, (tuple, list)) else ((a,), (b,))
    for x, y in zip(ta, tb):
        assert torch.equal(_bits(x), _bits(y)), "two identical launches differ"
    return a


def _same_bits(got, want):
    """got (device fp32) equals the float32 numpy array `want` bit for bit (NaN payloads aside: NaN matches NaN)."""
    g = got.detach().cpu().numpy()
    w = np.asarray(want, dtype=np.float32).reshape(g.shape)
    nan = np.isnan(w)
    return np.array_equal(np.isnan(g), nan) and np.array_equal(g[~nan].view(np.int32), w[~nan].view(np.int32))


# ---- fused clip + SGD ----------------------------------------------------------------------------------------------------------------
def _sgd_inputs(chunks, seed, clip):
    g = torch.Generator().manual_seed(seed)
    n = chunks * 256
    p = (torch.randn(n, generator=g) * 10.0 ** (torch.rand(n, generator=g) * 3 - 2)).float()
    gr = (torch.randn(n, generator=g) * 10.0 ** (torch.rand(n, generator=g) * 4 - 2)).float()
    if clip > 0:
        gr[:8] = torch.tensor([clip, -clip, 1e6, -1e6, -0.0, 0.0, float("inf"), float("-inf")])
    buf = (torch.randn(n, generator=g) * 0.1).float()
    lr = (torch.rand(chunks, generator=g) * 0.1 + 1e-3).float()               # changes at every chunk
    wd = torch.where(torch.arange(chunks) % 3 == 0, torch.zeros(chunks), torch.rand(chunks, generator=g) * 1e-2).float()
    return p, gr, buf, lr, wd


@pytest.mark.parametrize("chunks,clip,momentum,gs,dev_scale", [(1, 1.0, 0.9, 1.0, False), (3, 0.0, 0.9, 0.5, True), (3, 1.0, 0.0, 0.5, False),
                                                               (1000, 1.0, 0.9, 1.0, True), (1000, 0.0, 0.9, 0.5, False)])
def test_sgd_step(oh, chunks, clip, momentum, gs, dev_scale):
    """Three consecutive steps, each bit-equal to the float32 emulation in the kernel's operation order and within the float64 bound;
    gradients exactly at +-clip, far beyond it, +-0 and +-Inf (which clip to +-clip)."""
    p, gr, buf, lr, wd = _sgd_inputs(chunks, chunks + int(clip), clip)
    scale = 0.37
    sd = torch.tensor([scale], device=DEV) if dev_scale else None

    def run(p0, b0):
        pd, bd = p0.to(DEV).clone(), b0.to(DEV).clone()
        oh.sgd_step(pd, gr.to(DEV), bd, lr.to(DEV), wd.to(DEV), lr_scale=(123.0 if dev_scale else scale), momentum=momentum, clip_value=clip,
                    grad_scale=gs, lr_scale_dev=sd)
        return pd, bd
    for step in range(3):
        pd, bd = _twice(lambda: run(p, buf))
        pe, be = TL.sgd_step_ref(p, gr, buf, lr, wd, scale, momentum, clip, gs, emulate=True)
        assert _same_bits(pd, pe.v) and _same_bits(bd, be.v), (step, "differs from the fp32 emulation")
        px, bx = TL.sgd_step_ref(p, gr, buf, lr, wd, scale, momentum, clip, gs)
        assert np.isfinite(px.v).all() and np.isfinite(bx.v).all()
        _hold("sgd_step p", pd, px, (chunks, clip, step))
        _hold("sgd_step buf", bd, bx, (chunks, clip, step))
        p, buf = pd.cpu(), bd.cpu()


def test_sgd_step_nan_gradient_stays_nan(oh):
    """torch.nn.utils.clip_grad_value_ + torch.optim.SGD keep a NaN gradient (torch.clamp): NaN in the momentum buffer and the parameter.
    Its neighbours are untouched by it."""
    p, gr, buf, lr, wd = _sgd_inputs(3, 5, 1.0)
    gr[300], gr[700] = NAN, NAN
    pd, bd = p.to(DEV).clone(), buf.to(DEV).clone()
    oh.sgd_step(pd, gr.to(DEV), bd, lr.to(DEV), wd.to(DEV), lr_scale=1.0, momentum=0.9, clip_value=1.0, grad_scale=1.0)
    q = torch.nn.Parameter(p.clone())
    q.grad = gr.clone()
    torch.nn.utils.clip_grad_value_([q], 1.0)
    assert bool(torch.isnan(q.grad[300]))                                       # what the replaced step does
    assert bool(torch.isnan(pd[300])) and bool(torch.isnan(bd[300])) and bool(torch.isnan(pd[700])) and bool(torch.isnan(bd[700]))
    pe, be = TL.sgd_step_ref(p, gr, buf, lr, wd, 1.0, 0.9, 1.0, 1.0, emulate=True)
    assert _same_bits(pd, pe.v) and _same_bits(bd, be.v)
    assert int(torch.isnan(pd).sum()) == 2


# ---- the second stage's losses -----------------------------------------------------------------------------------------------------
RW = (10.0, 10.0, 5.0, 5.0)


@pytest.mark.parametrize("B,R,mode", [(1, 7, None), (5, 96, "edges"), (16, 128, None), (256, 3, "edges")])
def test_roi_losses(oh, B, R, mode):
    a = TL.roi_loss_inputs(B, R, B + R, device=DEV, mode=mode)
    ref = TL.roi_losses_ref(*a, B, R, RW)
    assert ref["df_margin"] >= 2.0
    out, ds, dd = _twice(lambda: oh.roi_losses(*a, B, R, RW))
    _hold("roi_losses loss_cls", out[0], ref["loss_cls"], (B, R))
    _hold("roi_losses loss_box", out[1], ref["loss_box"], (B, R))
    _hold("roi_losses dscores", ds, ref["dscores"], (B, R))
    assert _same_bits(dd, ref["ddeltas"]), "ddeltas is +-w or 0, exactly"


# ---- CenterNet losses ------------------------------------------------------------------------------------------------------------------
def _cn_run(oh, head, tgt, hm, pi, pc, coef, dhead_ld, **kw):
    rows, ld = head.shape
    sums = _twice(lambda: oh.centernet_loss_sums(head, tgt, hm, pi, pc, **kw))

    def bwd():
        dh = torch.full((rows, dhead_ld), NAN, device=DEV)
        dh[:, :5] = 7.0                                                         # k_cn_loss_grad overwrites all five before the positives' pass adds
        oh._chk(oh.lib().ore_centernet_losses_bwd(oh._ptr(head), ld, oh._ptr(tgt), oh._ptr(hm), rows, oh._ptr(pi), oh._ptr(pc), int(pi.numel()),
                                                  kw.get("gamma", 2.0), kw.get("beta", 4.0), kw.get("sigmoid_clamp", 1e-4),
                                                  kw.get("ignore_high_fp", 0.85), oh._ptr(coef), oh._ptr(dh), dhead_ld, oh._stream()),
                "ore_centernet_losses_bwd")
        return dh
    dh = _twice(bwd)
    if dhead_ld > 5:
        assert bool(dh[:, 5:].isnan().all()), "columns beyond the five gradients changed"
    return sums, dh[:, :5]


@pytest.mark.parametrize("ign", [0.0, 0.85])
@pytest.mark.parametrize("rows,ld", [(5, 5), (256, 16), (257, 5), (65536, 16), (65537, 16), (65537, 5)])
def test_centernet_loss_sums_and_grad(oh, rows, ld, ign):
    """Rows around one block and around the second grid-stride trip of k_cn_loss_partial (65 537); the edge rows of
    trainloss_ref.cn_loss_inputs; head as 5 columns of 16 with NaN in the others."""
    head, tgt, hm, pi, pc = TL.cn_loss_inputs(rows, rows, ld=ld, ignore_high_fp=ign, device=DEV)
    assert float(TL.cn_margins(head, 1e-4, ign).min()) >= TL.S_MARGIN
    coef = torch.tensor([0.7, 0.3, 1.9], device=DEV)
    sums, dh = _cn_run(oh, head, tgt, hm, pi, pc, coef, ld, ignore_high_fp=ign)
    ref = TL.centernet_losses_ref(head, tgt, hm, pi, pc, ignore_high_fp=ign)
    assert float(sums[1]) == ref["count"]
    for k, i in (("giou", 0), ("pos", 2), ("neg", 3)):
        _hold("centernet_loss_sums " + k, sums[i], ref[k], (rows, ld, ign))
    g = TL.centernet_loss_grad_ref(head, tgt, hm, pi, pc, coef, ignore_high_fp=ign)
    _hold("centernet_loss_grad", dh, g, (rows, ld, ign))
    if rows > 12:
        assert bool((dh[4:10, 4] == 0).all()), "logits +-12, +-20, +-100 are outside the clamp: no gradient"


@pytest.mark.parametrize("npos", [0, 1])
def test_centernet_loss_limits_and_no_positives(oh, npos):
    """clamp = 0.5 and logit 0: the sigmoid is 0.5 = both clamp limits = ignore_high_fp exactly.  The closed clamp passes the gradient,
    pred == ignore_high_fp is ignored.  pos_count = 0 leaves the positive sum an exact 0."""
    head, tgt, hm, pi, pc = TL.cn_loss_inputs(64, 9, clamp=0.5, ignore_high_fp=0.5, device=DEV, n_pos=npos)
    head[:8, 4] = 0.0
    coef = torch.tensor([1.0, 1.0, 1.0], device=DEV)
    for ign in (0.5, 0.0):
        kw = dict(sigmoid_clamp=0.5, ignore_high_fp=ign)
        sums, dh = _cn_run(oh, head, tgt, hm, pi, pc, coef, 5, **kw)
        ref = TL.centernet_losses_ref(head, tgt, hm, pi, pc, clamp=0.5, ignore_high_fp=ign)
        for k, i in (("giou", 0), ("pos", 2), ("neg", 3)):
            _hold("centernet_loss_sums/limits " + k, sums[i], ref[k], (npos, ign))
        if npos == 0:
            assert float(sums[2]) == 0.0
        if ign == 0.5:
            assert float(sums[3]) == 0.0
        g = TL.centernet_loss_grad_ref(head, tgt, hm, pi, pc, coef, clamp=0.5, ignore_high_fp=ign)
        _hold("centernet_loss_grad/limits", dh, g, (npos, ign))
        if ign == 0.0:
            assert bool((dh[:8, 4] != 0).all()) and bool((dh[8:, 4] == 0).all())


# ---- CenterNet targets -----------------------------------------------------------------------------------------------------------------
def _shapes(hw, strides=(8, 16, 32)):
    return [(-(-hw[0] // s), -(-hw[1] // s)) for s in strides]


@pytest.mark.parametrize("hw,B,counts", [((64, 96), 1, (1,)), ((64, 96), 3, (7, 0, 20)), ((136, 264), 1, (128,)), ((136, 264), 3, (128, 0, 128)),
                                         ((136, 264), 1, (0,))])
def test_centernet_targets(oh, hw, B, counts):
    """Levels smaller than a block (64 x 96) and a 561-row level 0 (136 x 264); 0, 1 and 128 objects; an empty image between two full
    ones; B * max_n * L = 1152 compaction entries (a second pass of k_cn_pos_inds); the list entry and the padded entry."""
    shapes = _shapes(hw)
    gt, cnt, _ = TL.cn_target_boxes(B, counts, hw, sum(counts) + B, shapes)
    ref = TL.centernet_targets_ref(gt, cnt, shapes, soi=TL.CN_SOI)
    mg = ref["margins"]
    assert mg["soi"] >= TL.CN_MARGIN and mg["owner"] >= TL.CN_MARGIN and mg["hm_cut"] >= TL.HM_MARGIN, mg
    gtd, cntd = torch.as_tensor(gt).to(DEV), torch.as_tensor(cnt).to(DEV)

    def padded():
        o = oh.centernet_targets(None, shapes, soi=TL.CN_SOI, padded=(gtd, cntd))
        return o["reg_targets"], o["hm_targets"], o["pos_inds"], o["pos_count"]

    def listed():
        o = oh.centernet_targets([torch.as_tensor(gt[b, :counts[b]]) for b in range(B)], shapes, soi=TL.CN_SOI)
        return o["reg_targets"], o["hm_targets"], o["pos_inds"], o["pos_count"]
    for form, fn in (("padded", padded), ("list", listed)):
        reg, hm, pi, pc = _twice(fn)
        n = int(pc.item())
        assert n == ref["pos_count"] and np.array_equal(pi[:n].cpu().numpy(), ref["pos_inds"]), form
        assert _same_bits(reg, ref["reg_targets"]), form
        assert np.array_equal(hm.cpu().numpy() == 0, ref["hm"].v == 0), (form, "the 1e-4 cut")
        _hold("centernet_targets hm", hm, ref["hm"], (hw, B, counts, form))


# ---- ROI sampling ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,cap,G,app,P,keys", TL.SAMPLE_CASES)
def test_sample_rois(oh, B, cap, G, app, P, keys):
    """Up to the kernel's 12 800 candidates (more than 48 KB of dynamic LDS); images without ground truth, without proposals, with fewer
    candidates than R and fewer foreground than P; equal keys, keys within one histogram bin, keys 0.0, 1.0, -0.5 and 2.0.  Every output
    equals the reference exactly, padding rows included."""
    a = TL.sample_inputs(B, cap, G, app, B + cap, thr=0.6, keys=keys, device=DEV)
    boxes, labels, gt, valid, margin = TL.sample_rois_ref(*a, 128, P, 0.6, bool(app))
    assert margin >= TL.IOU_MARGIN

    def run():
        ob, ol, og, ov = (torch.full((B, 128, 4), NAN, device=DEV), torch.full((B, 128), -7, device=DEV, dtype=torch.int64),
                          torch.full((B, 128, 4), NAN, device=DEV), torch.full((B, 128), True, device=DEV, dtype=torch.bool))
        N = cap + (G if app else 0)
        oh._chk(oh.lib().ore_sample_rois_fwd(oh._ptr(a[0]), oh._ptr(a[1]), oh._ptr(a[2]), oh._ptr(a[3]), oh._ptr(a[4]), B, cap, G, int(app), 128, P,
                                             0.6, oh._ptr(ob), oh._ptr(ol), oh._ptr(og), oh._ptr(ov), oh._stream()), "ore_sample_rois_fwd")
        assert a[4].shape == (B, N)
        return ob, ol, og, ov
    ob, ol, og, ov = _twice(run)
    assert np.array_equal(ov.cpu().numpy(), valid) and np.array_equal(ol.cpu().numpy(), labels)
    assert _same_bits(ob, boxes) and _same_bits(og, gt)


# ---- ROIAlign backward -------------------------------------------------------------------------------------------------------------
ROI_FORMS = ("tiled", "fixed", "atomics")


def _roi_bwd(oh, form, dout, feats_like, boxes, bidx, strides, min_level, P, dfeats=None):
    det, mode = oh.ROI_BWD_DETERMINISTIC, oh.ROI_BWD_MODE
    oh.ROI_BWD_DETERMINISTIC, oh.ROI_BWD_MODE = form != "atomics", ("tiled" if form == "tiled" else "fixed")
    try:
        return oh.roi_align_bwd(dout, feats_like, boxes, strides=strides, min_level=min_level, pooled=P, dfeats=dfeats, box_image=bidx)
    finally:
        oh.ROI_BWD_DETERMINISTIC, oh.ROI_BWD_MODE = det, mode


def _roi_check(form, got, ref, what):
    for l, gl in enumerate(got):
        if form == "fixed":
            assert float(np.abs(ref["ref"][l]).max()) < 2.0 ** 23, "the fixed-point form saturates"
        h, r = TL.roi_bwd_hold(gl, ref["ref"][l], ref["mag"][l], ref["d"], ref["contrib"][l] if form == "fixed" else None)
        op = f"roi_align_bwd/{form}"
        h0, r0, n0 = _RATIOS.get(op, (0.0, 0.0, 0))
        _RATIOS[op] = (max(h0, h), max(r0, r), n0 + 1)
        print(f"{op} {what} level {l}: hard {h:.3e} rms {r:.3e} d {ref['d']}")
        assert h <= 1 and r <= 1, (op, what, l, {"hard": h, "rms": r, "d": ref["d"]})


@pytest.mark.parametrize("pyramid,P,C,B,n", TL.ROI_BWD_CASES)
def test_roi_align_bwd(oh, pyramid, P, C, B, n):
    """Every case through all three launch forms of orehip.roi_align_bwd; the deterministic forms run twice, bit for bit.  The tiled form
    gets maps it must write completely (the wrapper hands it uninitialised ones)."""
    boxes, bidx, dout, scales, min_level, HWs, strides = TL.roi_bwd_case(pyramid, P, C, B, n, seed=P + C, device=DEV)
    ref = TL.roi_align_bwd_ref(dout, HWs, scales, min_level, P, boxes, bidx, B, C)
    if n >= 100:
        assert max(int(c.max()) for c in ref["contrib"]) >= 40 and ref["d"] >= 40
    like = [torch.full((B, h, w, C), NAN, device=DEV) for h, w in HWs]
    if P == 4 or (P == 7 and pyramid == "p2-5"):
        assert ref["wide"] >= 1, "no box with bins wider than 8 cells: the per-sample walk / roi_bwd_bins would not run with ph, pw > 0"
    if pyramid == "tiny":
        assert ref["levels"] == [0, 1, 2], "the 1 x 1 level is not reached"
    for r in range(n):
        same, margin = TL.roi_decisions_agree(boxes[r].cpu().numpy(), scales, min_level, P, HWs)
        assert same, (r, boxes[r].tolist(), margin)
    for form in ROI_FORMS:
        if form == "fixed" and n <= B:
            continue        # orehip.roi_align_bwd sends at most one ROI per image to the fp32-atomics launch: that is the "atomics" run
        run = lambda: tuple(_roi_bwd(oh, form, dout, like, boxes, bidx, strides, min_level, P))      # noqa: E731
        out = run() if form == "atomics" else _twice(run)
        _roi_check(form, list(out), ref, (pyramid, P, C, B, n))


@pytest.mark.parametrize("form", ROI_FORMS)
def test_roi_align_bwd_channel_slice(oh, form):
    """dfeat as channels [8, 8 + C) of a wider NaN-filled buffer (ld = C + 16, coff = 8), through the C entry points themselves: the
    other channels must not change."""
    import ctypes as CT
    pyramid, P, C, B, n = "p2-5", 7, 20, 3, 64
    boxes, bidx, dout, scales, min_level, HWs, strides = TL.roi_bwd_case(pyramid, P, C, B, n, seed=11, device=DEV)
    L = len(HWs)
    ref = TL.roi_align_bwd_ref(dout, HWs, scales, min_level, P, boxes, bidx, B, C)

    def run():
        wide = [torch.full((B, h, w, C + 16), NAN, device=DEV) for h, w in HWs]
        for x in wide:
            x[..., 8:8 + C] = 0.0
        i32 = lambda v: (CT.c_int32 * L)(*v)      # noqa: E731
        ptrs = (CT.c_void_p * L)(*[oh._ptr(x) for x in wide])
        args = (ptrs, i32([C + 16] * L), i32([8] * L), i32([h for h, _ in HWs]), i32([w for _, w in HWs]), (CT.c_float * L)(*scales), L, min_level,
                C, P, oh._ptr(boxes), oh._ptr(bidx), n, oh._ptr(dout))
        lib, S = oh.lib(), oh._stream()
        if form == "tiled":
            oh._chk(lib.ore_roi_align_bwd_tiled(*args, B, 1, S), "ore_roi_align_bwd_tiled")
        elif form == "fixed":
            scratch = [torch.zeros(B * h * w * C, dtype=torch.int64, device=DEV) for h, w in HWs]
            accs = (CT.c_void_p * L)(*[oh._ptr(s) for s in scratch])
            oh._chk(lib.ore_roi_align_bwd_det(*args, accs, B, S), "ore_roi_align_bwd_det")
        else:
            oh._chk(lib.ore_roi_align_bwd(*args, S), "ore_roi_align_bwd")
        torch.cuda.synchronize()
        return tuple(wide)
    wide = run() if form == "atomics" else _twice(run)
    for x in wide:
        assert bool(x[..., :8].isnan().all()) and bool(x[..., 8 + C:].isnan().all()), "wrote outside its channel slice"
    _roi_check(form, [x[..., 8:8 + C].contiguous() for x in wide], ref, "channel slice")


def test_roi_align_bwd_fresh_maps_and_accumulate(oh):
    """The tiled form without given maps writes every cell of NaN-free fresh maps; with given maps it accumulates onto their values."""
    pyramid, P, C, B, n = "p3-5", 7, 20, 3, 64
    boxes, bidx, dout, scales, min_level, HWs, strides = TL.roi_bwd_case(pyramid, P, C, B, n, seed=3, device=DEV)
    like = [torch.full((B, h, w, C), NAN, device=DEV) for h, w in HWs]
    out = _twice(lambda: tuple(_roi_bwd(oh, "tiled", dout, like, boxes, bidx, strides, min_level, P)))
    ref = TL.roi_align_bwd_ref(dout, HWs, scales, min_level, P, boxes, bidx, B, C)
    _roi_check("tiled", list(out), ref, "fresh maps")
    base = [TL.to_t(np.random.default_rng(l).standard_normal((B, h, w, C)).astype(np.float32), DEV) for l, (h, w) in enumerate(HWs)]
    refa = TL.roi_align_bwd_ref(dout, HWs, scales, min_level, P, boxes, bidx, B, C, base=base)
    for form in ROI_FORMS:
        maps = [b.clone() for b in base]
        _roi_bwd(oh, form, dout, maps, boxes, bidx, strides, min_level, P, dfeats=maps)
        _roi_check(form, maps, refa, "accumulate")


def test_roi_align_bwd_fixed_point_small_channel(oh):
    """Channels scaled to 1e-6 and 1e-8, where the fixed-point form's absolute term 2^-41 per contribution matters: at 1e-6 it reaches
    half of the relative bound 2 d u mag at the worst cell of these inputs, at 1e-8 it is the binding one (asserted on the reference)."""
    pyramid, P, C, B, n = "p3-5", 7, 4, 1, 64
    boxes, bidx, dout, scales, min_level, HWs, strides = TL.roi_bwd_case(pyramid, P, C, B, n, seed=5, device=DEV)
    dout = dout.reshape(n, P * P, C).clone()
    gen = torch.Generator().manual_seed(7)
    dout[..., 1] = (torch.randn(n, P * P, generator=gen) * 1e-6).to(DEV)
    dout[..., 2] = (torch.randn(n, P * P, generator=gen) * 1e-8).to(DEV)
    dout = dout.reshape(n, P * P * C)
    ref = TL.roi_align_bwd_ref(dout, HWs, scales, min_level, P, boxes, bidx, B, C)
    binding = max(float((c * TL.FX_ABS / np.maximum(2.0 * ref["d"] * TL.U * m[..., 2], 1e-300)).max()) for c, m in zip(ref["contrib"], ref["mag"]))
    assert binding > 1.0, ("on the 1e-8 channel the 2^-41 term must exceed 2 d u mag at some cell", binding)
    for form in ("fixed", "tiled"):
        maps = [torch.zeros(B, h, w, C, device=DEV) for h, w in HWs]
        _roi_bwd(oh, form, dout, maps, boxes, bidx, strides, min_level, P, dfeats=maps)
        _roi_check(form, maps, ref, "1e-6 channel")
