"""CPU: the float64 restatements of tests/trainloss_ref.py are the operations they name, and their bounds have teeth.

tests/trainloss_ref.py restates the nine kernels of csrc/ore_train.hip in float64 with a running-error magnitude.  Here, without a GPU:
  * every generator keeps its margins at every seed and shape tests/test_hip_trainloss.py uses (nothing is dropped; the share of
    re-drawn inputs is printed);
  * each restatement equals the pinned oracle: oracle.ref_model.centernet_targets, centernet_losses and its autograd,
    train_forward.get_deltas + F.cross_entropy and their autograd, train_forward.sample_rois_torch, torch.optim.SGD after
    clip_grad_value_;
  * an fp32 emulation in the kernel's operation and summation order passes both checks (the worst ratios are printed);
  * each fault the checks are there to catch fails at least one of them, on the shapes the GPU file uses;
  * every __global__ of csrc/ore_train.hip is in the coverage table."""
import os
import re
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import trainloss_ref as TL
import trainops_ref as TR
import inferops_ref as IR
from conftest import PKG
from oracle import ref_model as R

F64 = torch.float64
HEAD = {}


def _ratios(got, x):
    return TL.hold(torch.as_tensor(np.asarray(got, dtype=np.float64)), x)


def _ok(got, x):
    h, r = _ratios(got, x)
    return h <= 1 and r <= 1


def _head(op, got, x):
    h, r = _ratios(got, x)
    a = HEAD.setdefault(op, [0.0, 0.0])
    a[0], a[1] = max(a[0], h), max(a[1], r)
    assert h <= 1 and r <= 1, (op, h, r)


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nfp32 emulations, worst hard / rms ratio per op:")
    for op, (h, r) in sorted(HEAD.items()):
        print(f"  {op:28s} {h:.3f} {r:.3f}")
    print("re-drawn inputs (drawn, re-drawn):", {k: tuple(v) for k, v in TL.REDRAWS.items()})


# ---- SGD -----------------------------------------------------------------------------------------------------------------------------
def _sgd_case(chunks, seed, clip):
    g = torch.Generator().manual_seed(seed)
    n = chunks * 256
    p = TR.scaled_inputs((chunks, 256), seed, lo=-2, hi=1).reshape(n).clone()
    gr = (torch.randn(n, generator=g) * 10.0 ** (torch.rand(n, generator=g) * 4 - 2)).float()
    if clip > 0:
        gr[0], gr[1], gr[2], gr[3], gr[4] = clip, -clip, 1e6, -1e6, -0.0
    buf = torch.randn(n, generator=g) * 0.1
    lr = (torch.rand(chunks, generator=g) * 0.1 + 1e-3).float()
    wd = torch.where(torch.arange(chunks) % 3 == 0, torch.zeros(chunks), torch.rand(chunks, generator=g) * 1e-2).float()
    return p, gr, buf, lr, wd


@pytest.mark.parametrize("chunks,clip,momentum,gs", [(1, 1.0, 0.9, 1.0), (3, 0.0, 0.9, 0.5), (3, 1.0, 0.0, 0.5), (1000, 1.0, 0.9, 1.0)])
def test_sgd_reference_is_torch_sgd(chunks, clip, momentum, gs):
    p, gr, buf, lr, wd = _sgd_case(chunks, chunks, clip)
    ps = [torch.nn.Parameter(p[c * 256:(c + 1) * 256].double().clone()) for c in range(chunks)]
    opt = torch.optim.SGD([{"params": [q], "lr": float(lr[c]) * 0.5, "weight_decay": float(wd[c])} for c, q in enumerate(ps)],
                          lr=0.1, momentum=float(np.float32(momentum)))     # the kernel's momentum is an fp32 argument
    for c, q in enumerate(ps):
        q.grad = gr[c * 256:(c + 1) * 256].double() * gs
        if momentum:
            opt.state[q]["momentum_buffer"] = buf[c * 256:(c + 1) * 256].double().clone()
    if clip > 0:
        torch.nn.utils.clip_grad_value_(ps, clip)
    opt.step()
    px, bx = TL.sgd_step_ref(p, gr, buf, lr, wd, 0.5, momentum, clip, gs)
    want = torch.cat([q.detach() for q in ps]).numpy()
    assert np.abs(px.v - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    assert (px.m >= np.abs(px.v)).all() and (bx.m >= np.abs(bx.v)).all()
    pe, be = TL.sgd_step_ref(p, gr, buf, lr, wd, 0.5, momentum, clip, gs, emulate=True)
    assert pe.v.dtype == np.float32
    _head("sgd_step p", pe.v, px)
    _head("sgd_step buf", be.v, bx)


def test_sgd_emulation_equals_oracle_sgd_bitwise():
    """The float32 emulation is the fp32 statement of the oracle (oracle.ref_model.sgd_step_flat, torch fp32 ops one by one)."""
    p, gr, buf, lr, wd = _sgd_case(5, 7, 1.0)
    pe, be = TL.sgd_step_ref(p, gr, buf, lr, wd, 0.5, 0.9, 1.0, 0.5, emulate=True)
    po, bo = p.clone(), buf.clone()
    R.sgd_step_flat(po, gr, bo, lr, wd, 0.5, 0.9, 1.0, 0.5)
    assert np.array_equal(pe.v.view(np.int32), po.numpy().view(np.int32)) and np.array_equal(be.v.view(np.int32), bo.numpy().view(np.int32))


def test_sgd_nan_and_inf_follow_torch_clamp():
    p, gr, buf, lr, wd = _sgd_case(1, 3, 1.0)
    gr[10], gr[11], gr[12] = float("nan"), float("inf"), float("-inf")
    pe, be = TL.sgd_step_ref(p, gr, buf, lr, wd, 1.0, 0.9, 1.0, 1.0, emulate=True)
    q = torch.nn.Parameter(p.clone())
    q.grad = gr.clone()
    torch.nn.utils.clip_grad_value_([q], 1.0)
    assert torch.isnan(q.grad[10]) and q.grad[11] == 1.0 and q.grad[12] == -1.0
    assert np.isnan(pe.v[10]) and np.isnan(be.v[10])
    for i, c in ((11, 1.0), (12, -1.0)):
        b = np.float32(0.9) * buf[i].numpy() + (np.float32(c) + wd[0].numpy() * p[i].numpy())
        assert be.v[i] == b and np.isfinite(pe.v[i])
    assert np.isfinite(np.delete(pe.v, 10)).all()


@pytest.mark.parametrize("fault", ["wd_first", "lr_next"])
def test_sgd_faults_fail(fault):
    p, gr, buf, lr, wd = _sgd_case(3, 5, 1.0)
    wd[:] = torch.tensor([1e-2, 0.0, 5e-3])
    px, bx = TL.sgd_step_ref(p, gr, buf, lr, wd, 1.0, 0.9, 1.0, 1.0)
    pf, bf = TL.sgd_step_ref(p, gr, buf, lr, wd, 1.0, 0.9, 1.0, 1.0, emulate=True, fault=fault)
    assert not _ok(pf.v, px)


# ---- ROI losses ------------------------------------------------------------------------------------------------------------------------
ROI_LOSS_CASES = [(1, 7, None), (5, 96, "edges"), (16, 128, None), (256, 3, "edges")]
RW = (10.0, 10.0, 5.0, 5.0)


@pytest.mark.parametrize("B,R_,mode", ROI_LOSS_CASES)
def test_roi_losses_reference_is_cross_entropy_and_l1(B, R_, mode):
    from fewx.modeling.fsod import train_forward as TF
    scores, deltas, boxes, gt, labels, valid = TL.roi_loss_inputs(B, R_, B + R_, mode=mode)
    ref = TL.roi_losses_ref(scores, deltas, boxes, gt, labels, valid, B, R_, RW)
    assert ref["df_margin"] >= 2.0
    s, d = scores.double().requires_grad_(True), deltas.double().requires_grad_(True)
    nb = valid.view(B, R_).sum(1).clamp(min=1).double()
    w = (valid.view(B, R_).double() / (nb * B).view(B, 1)).reshape(-1)
    ce = F.cross_entropy(s, labels, reduction="none")
    fg = valid & (labels == 0)
    tgt = TF.get_deltas(boxes.double(), gt.double(), RW)
    l1 = ((d - tgt).abs().sum(1))
    lc, lb = (w * ce).sum(), (w * torch.where(fg, l1, torch.zeros_like(l1))).sum()
    (lc + lb).backward()
    close = lambda a, b: abs(a - b) <= 1e-12 * max(1.0, abs(b))      # noqa: E731
    assert close(float(ref["loss_cls"].v), float(lc.detach())) and close(float(ref["loss_box"].v), float(lb.detach()))
    assert np.abs(ref["dscores"].v - s.grad.numpy()).max() <= 1e-14
    assert np.abs(ref["ddeltas"].astype(np.float64) - d.grad.numpy()).max() <= 1e-7 * np.abs(d.grad.numpy()).max() + 1e-30
    if mode is None:                                         # the rows with boxes == gt and deltas == 0: target and gradient exactly 0
        assert (ref["ddeltas"][:min(3, R_)] == 0).all() and bool(fg[:min(3, R_)].all())
    emu = TL.roi_losses_ref(scores, deltas, boxes, gt, labels, valid, B, R_, RW, emulate=True)
    assert np.array_equal(emu["ddeltas"], ref["ddeltas"])
    _head("roi_losses dscores", emu["dscores"].v, ref["dscores"])
    for k in ("loss_cls", "loss_box"):
        _head("roi_losses " + k, _roi_sum_order(emu, k), ref[k])


def _roi_sum_order(emu, k):
    """k_roi_losses' sum in fp32: thread t adds its terms t, t + 256, ... in order, then 8 tree steps over the 256 partial sums."""
    x = emu[k + "_terms"]
    pad = np.zeros(-(-len(x) // 256) * 256, dtype=np.float32)
    pad[:len(x)] = x
    acc = np.zeros(256, dtype=np.float32)
    for row in pad.reshape(-1, 256):
        acc = acc + row
    d = 128
    while d:
        acc[:d] = acc[:d] + acc[d:2 * d]
        d //= 2
    return acc[0]


@pytest.mark.parametrize("fault", ["no_B", "count_invalid"])
def test_roi_losses_faults_fail(fault):
    B, R_, mode = 5, 96, "edges"
    a = TL.roi_loss_inputs(B, R_, B + R_, mode=mode)
    ref = TL.roi_losses_ref(*a, B, R_, RW)
    bad = TL.roi_losses_ref(*a, B, R_, RW, emulate=True, fault=fault)
    assert not _ok(bad["loss_cls"].v, ref["loss_cls"]) and not _ok(bad["dscores"].v, ref["dscores"])
    assert not np.array_equal(bad["ddeltas"], ref["ddeltas"])


# ---- CenterNet losses ------------------------------------------------------------------------------------------------------------------
CN_ROWS = (5, 256, 257, 65536, 65537)


@pytest.mark.parametrize("ign", [0.0, 0.85])
@pytest.mark.parametrize("rows", CN_ROWS)
def test_centernet_losses_reference_is_oracle(rows, ign):
    head, tgt, hm, pi, pc = TL.cn_loss_inputs(rows, rows, ld=16, ignore_high_fp=ign)
    assert float(TL.cn_margins(head, 1e-4, ign).min()) >= TL.S_MARGIN
    n = int(pc[0])
    ref = TL.centernet_losses_ref(head, tgt, hm, pi, pc, ignore_high_fp=ign)
    hd = head[:, :5].double().requires_grad_(True)
    o = R.centernet_losses(hd[:, :4], hd[:, 4], pi[:n], tgt.double(), hm.double(), clamp=float(np.float32(1e-4)),
                           ignore_high_fp=(float(np.float32(ign)) if ign > 0 else 2.0))
    sums = o["sums"]
    for k, i in (("giou", 0), ("pos", 2), ("neg", 3)):
        # the oracle's upper limit is the float64 1 - 1e-4, the kernel's fl32(1 - fl32(1e-4)): 3e-8 apart, seen by the clamped rows
        tol = 1e-9 if k == "giou" else 1e-5          # and it takes the sigmoid in fp32
        assert abs(float(ref[k].v) - float(sums[i])) <= tol * max(1.0, abs(float(sums[i]))), (k, float(ref[k].v), float(sums[i]))
        assert float(ref[k].m) >= abs(float(ref[k].v))
    assert ref["count"] == int(sums[1])
    coef = torch.tensor([0.7, 0.3, 1.9])
    (coef[0].double() * sums[0] - coef[1].double() * sums[2] - coef[2].double() * sums[3]).backward()
    g = TL.centernet_loss_grad_ref(head, tgt, hm, pi, pc, coef, ignore_high_fp=ign)
    want = hd.grad.numpy()
    scale = np.maximum(np.abs(want), 1e-30)
    # the oracle clamps 1 - 1e-4 in float64, the kernel at fl32(1 - fl32(1e-4)): rows between the two limits differ by design
    s64 = 1 / (1 + np.exp(-head[:, 4].double().numpy()))
    between = (s64 > float(np.float32(1) - np.float32(1e-4))) & (s64 < 1 - float(np.float32(1e-4)))
    assert not between.any()
    assert (np.abs(g.v - want)[:, :4] <= 1e-10 * g.m[:, :4] + 1e-300).all(), float(np.abs(g.v - want)[:, :4].max())
    # the oracle takes the sigmoid of the logit in fp32 (hm_logit.float()): one fp32 rounding of s, which the magnitude of column 4 covers
    assert (np.abs(g.v - want)[:, 4] <= 20 * TL.U * g.m[:, 4] + 1e-300).all(), float((np.abs(g.v - want)[:, 4] / np.maximum(g.m[:, 4], 1e-300)).max())
    assert (g.m >= np.abs(g.v) * (1 - 1e-12)).all()
    emu = TL.centernet_losses_ref(head, tgt, hm, pi, pc, ignore_high_fp=ign, emulate=True)
    assert emu["count"] == ref["count"]
    for k in ("giou", "pos", "neg"):
        _head("centernet_loss_sums " + k, emu[k].v, ref[k])
    ge = TL.centernet_loss_grad_ref(head, tgt, hm, pi, pc, coef, ignore_high_fp=ign, emulate=True)
    _head("centernet_loss_grad", ge.v, g)


def test_centernet_losses_edge_rows_are_present():
    head, tgt, hm, pi, pc = TL.cn_loss_inputs(257, 257, ld=16)
    h, t = head.numpy(), tgt.numpy()
    assert h[0, 0] == 0 and (h[1, :4] == t[1]).sum() == 1 and (h[2, :4] == t[2]).sum() == 2 and (h[3, :4] == t[3]).all()
    assert list(h[4:10, 4]) == [12, -12, 20, -20, 100, -100] and hm[10] == 0 and hm[11] == 1
    assert np.isnan(h[:, 5:]).all() and len(set(pi.tolist())) < len(pi)
    g = TL.centernet_loss_grad_ref(head, tgt, hm, pi, pc, torch.ones(3))
    assert (g.v[4:10, 4] == 0).all() and (g.m[4:10, 4] == 0).all()            # outside the clamp: no gradient, exactly
    assert g.v[11, 4] != 0 and int(pi[3]) == 11                              # hm == 1: no negative term, the positive one remains


def test_centernet_losses_on_the_clamp_and_ignore_limits():
    """clamp = 0.5 and logit 0: s = 0.5 = both clamp limits = ignore_high_fp, exactly, in fp32 and float64."""
    head, tgt, hm, pi, pc = TL.cn_loss_inputs(64, 9, clamp=0.5, ignore_high_fp=0.5)
    head[:8, 4] = 0.0
    pi[:2] = 1
    coef = torch.tensor([1.0, 1.0, 1.0])
    ref = TL.centernet_losses_ref(head, tgt, hm, pi, pc, clamp=0.5, ignore_high_fp=0.5)
    off = TL.centernet_losses_ref(head, tgt, hm, pi, pc, clamp=0.5, ignore_high_fp=0.0)
    assert float(ref["neg"].v) == 0.0 and float(off["neg"].v) < 0                # pred == ignore_high_fp is ignored
    bad = TL.centernet_losses_ref(head, tgt, hm, pi, pc, clamp=0.5, ignore_high_fp=0.5, emulate=True, fault="ignore_le")
    assert not _ok(bad["neg"].v, ref["neg"])
    g = TL.centernet_loss_grad_ref(head, tgt, hm, pi, pc, coef, clamp=0.5, ignore_high_fp=0.0)
    assert (g.v[:8, 4] != 0).all() and (g.v[8:, 4] == 0).all()                  # the closed interval passes the gradient AT the limit
    gb = TL.centernet_loss_grad_ref(head, tgt, hm, pi, pc, coef, clamp=0.5, ignore_high_fp=0.0, emulate=True, fault="clamp_open")
    assert not _ok(gb.v, g)


@pytest.mark.parametrize("fault", ["trip2", "wave"])
def test_centernet_loss_sum_faults_fail(fault):
    rows = 65537
    a = TL.cn_loss_inputs(rows, rows, ld=16)
    ref = TL.centernet_losses_ref(*a)
    bad = TL.centernet_losses_ref(*a, emulate=True, fault=fault)
    assert not _ok(bad["neg"].v, ref["neg"]) and not _ok(bad["giou"].v, ref["giou"])


@pytest.mark.parametrize("fault", ["tie10", "ignore_le", "dup_once", "clamp_open"])
def test_centernet_loss_grad_faults_fail(fault):
    rows = 257
    kw = dict(clamp=0.5, ignore_high_fp=0.5) if fault in ("ignore_le", "clamp_open") else {}
    head, tgt, hm, pi, pc = TL.cn_loss_inputs(rows, rows, ld=16, **kw)
    if kw:
        head[:8, 4] = 0.0
        kw["ignore_high_fp"] = 0.5 if fault == "ignore_le" else 0.0
    coef = torch.tensor([0.7, 0.3, 1.9])
    g = TL.centernet_loss_grad_ref(head, tgt, hm, pi, pc, coef, **kw)
    gb = TL.centernet_loss_grad_ref(head, tgt, hm, pi, pc, coef, emulate=True, fault=fault, **kw)
    assert not _ok(gb.v, g)


# ---- CenterNet targets -----------------------------------------------------------------------------------------------------------------
CN_TARGET_CASES = [((64, 96), 1, (1,)), ((64, 96), 3, (7, 0, 20)), ((136, 264), 1, (128,)), ((136, 264), 3, (128, 0, 128)), ((136, 264), 1, (0,))]


def _shapes(hw, strides=(8, 16, 32)):
    return [(-(-hw[0] // s), -(-hw[1] // s)) for s in strides]


@pytest.mark.parametrize("hw,B,counts", CN_TARGET_CASES)
def test_centernet_targets_reference_is_oracle(hw, B, counts):
    shapes = _shapes(hw)
    gt, cnt, _ = TL.cn_target_boxes(B, counts, hw, sum(counts) + B, shapes)
    ref = TL.centernet_targets_ref(gt, cnt, shapes, soi=TL.CN_SOI)
    mg = ref["margins"]
    assert mg["soi"] >= TL.CN_MARGIN and mg["owner"] >= TL.CN_MARGIN and mg["hm_cut"] >= TL.HM_MARGIN, mg
    pos, reg, hm = R.centernet_targets([torch.as_tensor(gt[b, :counts[b]]) for b in range(B)], shapes, soi=TL.CN_SOI)
    assert np.array_equal(ref["pos_inds"], pos.numpy()) and ref["pos_count"] == len(pos)
    assert np.array_equal(ref["reg_targets"], reg.numpy())
    assert np.abs(ref["hm"].v - hm.numpy()).max() <= 1e-5
    assert ((ref["hm"].v == 0) == (hm.numpy() == 0)).all()
    _head("centernet_targets hm (oracle fp32)", hm.numpy(), ref["hm"])


def test_centernet_targets_exact_cases_sit_on_the_limits():
    hw, shapes = (136, 264), _shapes((136, 264))
    gt, cnt, _ = TL.cn_target_boxes(1, (8,), hw, 1, shapes)
    b = gt[0]
    crit = np.sqrt((b[:, 2] - b[:, 0]) ** 2 + (b[:, 3] - b[:, 1]) ** 2) / 2
    assert crit[0] == 40 and crit[2] == 80 and (b[0] == b[1]).all()
    ref = TL.centernet_targets_ref(gt, cnt, shapes, soi=TL.CN_SOI)
    rows0 = shapes[0][0] * shapes[0][1]
    # box 0 (crit 40) is a positive of level 0 AND level 1; box 2 (crit 80) of level 1 AND level 2
    assert (ref["pos_inds"] < rows0).sum() >= 3 and ref["pos_count"] == 8 + 4
    for fault in ("owner_le", "in_box_ge", "half7"):
        bad = TL.centernet_targets_ref(gt, cnt, shapes, soi=TL.CN_SOI, fault=fault)
        assert not np.array_equal(bad["reg_targets"], ref["reg_targets"]), fault


# ---- ROI sampling ----------------------------------------------------------------------------------------------------------------------
SAMPLE_CASES = TL.SAMPLE_CASES


@pytest.mark.parametrize("B,cap,G,app,P,keys", SAMPLE_CASES)
def test_sample_rois_reference_is_the_histogram_selection_and_torch(B, cap, G, app, P, keys, monkeypatch):
    from fewx.modeling.fsod import train_forward as TF
    a = TL.sample_inputs(B, cap, G, app, B + cap, thr=0.6, keys=keys)
    prop, prop_n, gtp, gt_n, u = a
    boxes, labels, gt, valid, margin = TL.sample_rois_ref(*a, 128, P, 0.6, bool(app))
    assert margin >= TL.IOU_MARGIN
    lab, mi, _ = TL.sample_match(prop, prop_n, gtp, gt_n, bool(app), 0.6)
    for b in range(B):
        pick = TL.sample_rois_histogram(lab[b], u[b].numpy(), 128, P)
        cand = torch.cat([prop[b], gtp[b]], 0).numpy() if app else prop[b].numpy()
        assert np.array_equal(valid[b], pick >= 0)
        assert np.array_equal(boxes[b][valid[b]], cand[pick[pick >= 0]])
    if keys == "uniform" and cap <= 4000:              # torch.topk orders equal keys (and its own 2.0 sentinel) arbitrarily
        rh = types.SimpleNamespace(batch_size_per_image=128, positive_fraction=P / 128, iou_threshold=0.6, proposal_append_gt=bool(app))
        monkeypatch.setattr(torch, "rand", lambda *s, **k: u.clone())
        tb, tl, tg, tv = TF.sample_rois_torch(rh, prop, prop_n, gtp, gt_n)
        monkeypatch.undo()
        assert np.array_equal(tv.numpy(), valid) and np.array_equal(tl.numpy(), labels)
        assert np.array_equal(tb.numpy(), boxes) and np.array_equal(tg.numpy()[valid], gt[valid])


def test_sample_rois_faults_fail():
    a = TL.sample_inputs(2, 4000, 256, 1, 4002, thr=0.6, keys="one_bin")
    ref = TL.sample_rois_ref(*a, 128, 64, 0.6, True)
    bad = TL.sample_rois_ref(*a, 128, 64, 0.6, True, tie_high=True)
    assert not np.array_equal(ref[0], bad[0])
    a = TL.sample_inputs(16, 400, 3, 1, 416, thr=0.6, keys="outside")
    prop, prop_n, gtp, gt_n, u = a
    lab, _, _ = TL.sample_match(prop, prop_n, gtp, gt_n, True, 0.6)
    differs = any(not np.array_equal(TL.sample_rois_histogram(lab[b], u[b].numpy(), 128, 64),
                                     TL.sample_rois_histogram(lab[b], u[b].numpy(), 128, 64, wrap=True)) for b in range(16))
    assert differs


# ---- ROIAlign backward -------------------------------------------------------------------------------------------------------------
def _roi_levels_check(got, ref):
    worst = [0.0, 0.0]
    for l in range(len(got)):
        h, r = TL.roi_bwd_hold(torch.as_tensor(np.asarray(got[l], dtype=np.float64)), ref["ref"][l], ref["mag"][l], ref["d"])
        worst = [max(worst[0], h), max(worst[1], r)]
    return worst


@pytest.mark.parametrize("P,C,B,n", [(7, 8, 1, 40), (1, 4, 1, 30), (8, 4, 3, 45), (14, 4, 1, 20), (4, 4, 3, 40)])
def test_roi_align_bwd_reference_is_the_oracle_autograd(P, C, B, n):
    """Autograd of oracle.ref_model.roi_pool_levels itself, image by image: it pools in fp32 (its output buffer is fp32), so its gradient
    is held to the bound of the kernels (level routing and image index included); the same expression over assign_levels + roi_align
    runs in float64 and is held to 1e-10 of the magnitude."""
    boxes, bidx, dout, scales, min_level, HWs, strides = TL.roi_bwd_case("p3-5", P, C, B, n, seed=P)
    ref = TL.roi_align_bwd_ref(dout, HWs, scales, min_level, P, boxes, bidx, B, C)
    feats = [torch.zeros(B, C, h, w, requires_grad=True) for h, w in HWs]
    f64s = [torch.zeros(B, C, h, w, dtype=F64, requires_grad=True) for h, w in HWs]
    loss = 0
    for b in range(B):
        idx = torch.nonzero(bidx == b).squeeze(1)
        o = R.roi_pool_levels([f[b:b + 1] for f in feats], boxes[idx], P, strides=strides)          # [k, C, P, P]
        loss = loss + (o.permute(0, 2, 3, 1).reshape(len(idx), -1) * dout[idx]).sum()
        lv = R.assign_levels(boxes[idx])
        for l, f in enumerate(f64s):
            j = idx[lv == l]
            if len(j):
                o64 = R.roi_align(f[b], boxes[j].double(), scales[l], P)
                loss = loss + (o64.permute(0, 2, 3, 1).reshape(len(j), -1) * dout[j].double()).sum()
    loss.backward()
    h, r = _roi_levels_check([f.grad.permute(0, 2, 3, 1).numpy() for f in feats], ref)
    assert h <= 1 and r <= 1, (h, r)
    for l, f in enumerate(f64s):
        want = f.grad.permute(0, 2, 3, 1).numpy()
        assert (np.abs(ref["ref"][l] - want) <= 1e-10 * ref["mag"][l] + 1e-300).all(), l
        assert (ref["mag"][l] >= np.abs(ref["ref"][l]) * (1 - 1e-12)).all()


@pytest.mark.parametrize("pyramid,P,C,B,n", TL.ROI_BWD_CASES)
def test_roi_bwd_boxes_keep_their_decisions(pyramid, P, C, B, n):
    """Every box of every GPU case: fp32 and float64 agree on the level, both grids and every sample's validity; a box that is not one
    of the hand-written exact ones also keeps ROI_MARGIN.  The cases reach what they are there for."""
    boxes, bidx, dout, scales, min_level, HWs, _ = TL.roi_bwd_case(pyramid, P, C, B, n, seed=P + C)
    exact = {tuple(b) for b in IR.ROI_EXACT_BOXES} | {tuple(b) for b in TL.ROI_TINY_BOXES} | {(40.0, 48.0, 72.0, 80.0)} | set(TL.ROI_WIDE_BOXES)
    worst = 1.0
    for r in range(n):
        same, margin = TL.roi_decisions_agree(boxes[r].numpy(), scales, min_level, P, HWs)
        assert same, (r, boxes[r].tolist())
        if tuple(boxes[r].tolist()) not in exact:
            worst = min(worst, margin)
    assert worst >= IR.ROI_MARGIN, worst
    ref = TL.roi_align_bwd_ref(dout, HWs, scales, min_level, P, boxes, bidx, B, C)
    if pyramid == "tiny":
        assert ref["levels"] == [0, 1, 2]
    elif P == 4 or (P == 7 and pyramid == "p2-5"):
        assert ref["wide"] >= 1


@pytest.mark.parametrize("pyramid,P,C,B,n", TL.ROI_BWD_CASES)
def test_roi_align_bwd_fp32_emulation_passes(pyramid, P, C, B, n):
    boxes, bidx, dout, scales, min_level, HWs, _ = TL.roi_bwd_case(pyramid, P, C, B, n, seed=P + C)
    ref = TL.roi_align_bwd_ref(dout, HWs, scales, min_level, P, boxes, bidx, B, C)
    emu = TL.roi_align_bwd_ref(dout, HWs, scales, min_level, P, boxes, bidx, B, C, emulate=True)
    assert emu["ref"][0].dtype == np.float32
    h, r = _roi_levels_check(emu["ref"], ref)
    a = HEAD.setdefault("roi_align_bwd", [0.0, 0.0])
    a[0], a[1] = max(a[0], h), max(a[1], r)
    assert h <= 1 and r <= 1, (h, r)


def test_roi_align_bwd_fixed_point_term():
    """A channel at 1e-8: an emulation that quantises every contribution to 2^-40 passes with the 2^-41 term and fails without it."""
    pyramid, P, C, B, n = "p3-5", 7, 4, 1, 64
    boxes, bidx, dout, scales, min_level, HWs, _ = TL.roi_bwd_case(pyramid, P, C, B, n, seed=5)
    dout = dout.reshape(n, P * P, C).clone()
    dout[..., 2] = torch.randn(n, P * P, generator=torch.Generator().manual_seed(7)) * 1e-8
    dout = dout.reshape(n, P * P * C)
    ref = TL.roi_align_bwd_ref(dout, HWs, scales, min_level, P, boxes, bidx, B, C)
    emu = TL.roi_align_bwd_ref(dout, HWs, scales, min_level, P, boxes, bidx, B, C, emulate=True, quantise=True)
    with_term, without = [0.0, 0.0], [0.0, 0.0]
    for l in range(len(HWs)):
        got = torch.as_tensor(emu["ref"][l].astype(np.float64))
        for acc, c in ((with_term, ref["contrib"][l]), (without, None)):
            h, r = TL.roi_bwd_hold(got, ref["ref"][l], ref["mag"][l], ref["d"], c)
            acc[0], acc[1] = max(acc[0], h), max(acc[1], r)
    HEAD["roi_align_bwd fixed point"] = with_term
    assert max(with_term) <= 1, with_term
    assert max(without) > 1, without


@pytest.mark.parametrize("fault", ["yH", "grid", "level", "clampH2", "cnt", "skip", "image"])
def test_roi_align_bwd_faults_fail(fault):
    pyramid, P, C, B, n = ("p2-5", 8, 20, 3, 300) if fault == "image" else (("p3-5", 1, 4, 1, 64) if fault == "yH" else ("p3-5", 7, 32, 1, 300))
    boxes, bidx, dout, scales, min_level, HWs, _ = TL.roi_bwd_case(pyramid, P, C, B, n, seed=P + C)
    ref = TL.roi_align_bwd_ref(dout, HWs, scales, min_level, P, boxes, bidx, B, C)
    bad = TL.roi_align_bwd_ref(dout, HWs, scales, min_level, P, boxes, bidx, B, C, fault=fault)
    h, r = _roi_levels_check(bad["ref"], ref)
    assert h > 1 or r > 1, (fault, h, r)


# ---- coverage ------------------------------------------------------------------------------------------------------------------------
def test_every_train_kernel_is_in_the_table():
    with open(os.path.join(PKG, "csrc", "ore_train.hip")) as f:
        names = set(re.findall(r"__global__.*?void\s+(\w+)\s*\(", f.read()))
    assert names == set(TL.KERNELS), names ^ set(TL.KERNELS)
    with open(os.path.join(os.path.dirname(__file__), "test_hip_trainloss.py")) as f:
        src = f.read()
    for k, (entry, test) in TL.KERNELS.items():
        assert ("def " + test + "(") in src, (k, test)
    for fn in ("roi_losses", "centernet_loss_sums", "centernet_loss_grad"):
        assert "test_hip_trainloss" in TR.NOT_COVERED[fn]
    assert "test_hip_trainloss" in TR.NOT_COVERED["roi_align_bwd"]
    for k in ("k_roi_align_bwd", "k_roi_align_bwd_col", "k_roi_align_bwd_tile"):
        assert "test_hip_trainloss" in IR.NOT_COVERED[k], k
    assert "k_roi_align_bwd launch" in TL.NOT_REACHED


def test_charges_are_twice_the_measured_ulps():
    import math
    for fn, K in (("expf", TL.K_EXP), ("logf", TL.K_LOG), ("powf", TL.K_POW)):
        assert TL.ULP_MEASURED[fn] > 0 and K == math.ceil(2 * TL.ULP_MEASURED[fn]), fn
    assert TL.ULP_MEASURED["sqrtf"] <= 0.5 and TL.ULP_MEASURED["div"] <= 0.5
