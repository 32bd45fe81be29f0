"""Training wrappers: CenterNet targets and losses, sampling, ROI losses, SGD and norms, device packing, gradients, train ops."""

from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import torch

import orehip          # _S2_MAX_BYTES lives on the package, where tests rebind it
from ._capi import OreError, _chk, _f32, _ptr, _stream, lib
from .image import to_device


def centernet_targets(gt_boxes: Sequence[torch.Tensor], shapes: Sequence[Tuple[int, int]], strides=(8, 16, 32),
                      soi=((0, 64), (48, 192), (128, 1000000)), hm_min_overlap: float = 0.8, min_radius: float = 4.0,
                      device=None, padded: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                      more_pos: Optional[Tuple[torch.Tensor, float, int]] = None) -> Dict[str, torch.Tensor]:
    """CenterNet._get_ground_truth (ref:fewx/modeling/fsod/fsod_rpn.py:803-901) on device.  gt_boxes: per image [N_i,4]; or
    `padded` = (boxes [B,G,4] fp32, counts [B] int32) already on the device (fixed shapes: a captured training step).
    `more_pos` = (head rows [rows, ld >= 4] fp32 in the targets' row order, MORE_POS_THRESH, MORE_POS_TOPK): pos_inds / pos_count are
    the reference's _add_more_pos list (:1213-1343; ore_centernet_more_pos_fwd, capacity B * max_n * L * 9) instead of one centre per
    (object, level that cares); the same stream, no host sync."""
    dev = torch.device(device or "cuda")
    L = len(strides)
    if padded is not None:
        gt, cnt = padded
        assert gt.is_cuda and gt.dtype == torch.float32 and gt.is_contiguous() and cnt.dtype == torch.int32 and cnt.numel() == gt.shape[0]
        B, max_n = int(gt.shape[0]), int(gt.shape[1])
    else:
        B = len(gt_boxes)
        ns = [int(b.shape[0]) for b in gt_boxes]
        max_n = max(1, max(ns))
        # no blocking copy in either direction: device boxes are padded on the device, host boxes go up through pinned memory
        if any(b.is_cuda for b in gt_boxes):
            gt = torch.zeros(B, max_n, 4, dtype=torch.float32, device=dev)
            for i, b in enumerate(gt_boxes):
                if ns[i]:
                    gt[i, :ns[i]] = to_device(b.detach().float(), dev)
        else:
            gt = torch.zeros(B, max_n, 4, dtype=torch.float32)
            for i, b in enumerate(gt_boxes):
                gt[i, :ns[i]] = b.detach().float()
            gt = to_device(gt, dev)
        cnt = to_device(torch.tensor(ns, dtype=torch.int32), dev)
    rows = sum(B * h * w for h, w in shapes)
    if more_pos is not None:
        head, mp_thresh, mp_topk = more_pos
        head = head.detach()
        if not (head.is_cuda and head.dtype == torch.float32 and head.dim() == 2 and head.shape[0] == rows and head.shape[1] >= 4
                and head.stride(1) == 1 and head.stride(0) >= head.shape[1]):
            raise OreError(f"centernet_targets: more_pos takes the [{rows}, >= 4] fp32 head rows on the device, got "
                           f"{tuple(head.shape)} {head.dtype} {head.device}")
    o = {"reg_targets": torch.empty(rows, 4, device=dev), "hm_targets": torch.empty(rows, device=dev),
         "pos_inds": torch.zeros(B * max_n * L * (9 if more_pos is not None else 1), dtype=torch.int64, device=dev),
         "pos_count": torch.zeros(1, dtype=torch.int32, device=dev)}
    Hs = (C.c_int32 * L)(*[h for h, _ in shapes]); Ws = (C.c_int32 * L)(*[w for _, w in shapes]); St = (C.c_int32 * L)(*strides)
    so = (C.c_float * (2 * L))(*[float(v) for r in soi for v in r])
    if more_pos is None:
        _chk(lib().ore_centernet_targets_fwd(L, Hs, Ws, St, B, _ptr(gt), _ptr(cnt), max_n, so, hm_min_overlap, min_radius,
                                             _ptr(o["reg_targets"]), _ptr(o["hm_targets"]), _ptr(o["pos_inds"]), _ptr(o["pos_count"]),
                                             _stream()), "ore_centernet_targets_fwd")
    else:
        _chk(lib().ore_centernet_targets_fwd(L, Hs, Ws, St, B, _ptr(gt), _ptr(cnt), max_n, so, hm_min_overlap, min_radius,
                                             _ptr(o["reg_targets"]), _ptr(o["hm_targets"]), None, None, _stream()), "ore_centernet_targets_fwd")
        _chk(lib().ore_centernet_more_pos_fwd(L, Hs, Ws, St, B, _ptr(gt), _ptr(cnt), max_n, so, _ptr(head), int(head.stride(0)),
                                              float(mp_thresh), int(mp_topk), _ptr(o["pos_inds"]), _ptr(o["pos_count"]), _stream()),
             "ore_centernet_more_pos_fwd")
    o["_keep"] = (gt, cnt) if more_pos is None else (gt, cnt, head)
    return o


def centernet_loss_sums(head: torch.Tensor, reg_targets: torch.Tensor, hm_targets: torch.Tensor, pos_inds: torch.Tensor,
                        pos_count: torch.Tensor, gamma: float = 2.0, beta: float = 4.0, sigmoid_clamp: float = 1e-4,
                        ignore_high_fp: float = 0.85) -> torch.Tensor:
    """[giou sum, #reg rows, pos focal sum, neg focal sum] of CenterNet.losses (ref:fewx/modeling/fsod/fsod_rpn.py:702-779).
    head [rows, ld>=5]: cols 0..3 ltrb prediction, col 4 heatmap logit."""
    rows, ld = head.shape
    out = torch.zeros(4, device=head.device)
    ws = torch.empty(4 * 256, device=head.device)
    _chk(lib().ore_centernet_losses_fwd(_ptr(_f32(head)), ld, _ptr(_f32(reg_targets)), _ptr(_f32(hm_targets)), rows, _ptr(pos_inds),
                                        _ptr(pos_count), gamma, beta, sigmoid_clamp, ignore_high_fp, _ptr(out), _ptr(ws), _stream()),
         "ore_centernet_losses_fwd")
    return out


def centernet_loss_grad(head: torch.Tensor, reg_targets: torch.Tensor, hm_targets: torch.Tensor, pos_inds: torch.Tensor,
                        pos_count: torch.Tensor, coef3: torch.Tensor, gamma: float = 2.0, beta: float = 4.0, sigmoid_clamp: float = 1e-4,
                        ignore_high_fp: float = 0.85) -> torch.Tensor:
    """d(losses)/d(head[:, :5]) for coef3 = [reg_w/reg_norm, pos_w*alpha/num_pos_avg, neg_w*(1-alpha)/num_pos_avg] (device)."""
    rows, ld = head.shape
    dhead = torch.zeros(rows, ld, device=head.device, dtype=torch.float32)
    _chk(lib().ore_centernet_losses_bwd(_ptr(_f32(head)), ld, _ptr(_f32(reg_targets)), _ptr(_f32(hm_targets)), rows, _ptr(pos_inds),
                                        _ptr(pos_count), int(pos_inds.numel()), gamma, beta, sigmoid_clamp, ignore_high_fp,
                                        _ptr(_f32(coef3)), _ptr(dhead), ld, _stream()), "ore_centernet_losses_bwd")
    return dhead


def sample_rois(prop: torch.Tensor, prop_n: torch.Tensor, gtp: torch.Tensor, gt_n: torch.Tensor, keys: torch.Tensor, R: int, P: int,
                iou_thr: float, append_gt: bool = True):
    """label_and_sample_proposals of B images in one launch (ore_sample_rois_fwd).  prop [B,cap,4], prop_n [B] int64, gtp [B,G,4],
    gt_n [B] int64, keys [B, cap (+G)] fp32 -> boxes [B,R,4], labels [B,R] int64, matched gt [B,R,4], valid [B,R] bool."""
    B, cap, _ = prop.shape
    G = gtp.shape[1]
    N = cap + (G if append_gt else 0)
    dev = prop.device
    assert keys.shape == (B, N) and keys.dtype == torch.float32 and keys.is_contiguous()
    assert prop_n.dtype == torch.int64 and gt_n.dtype == torch.int64 and prop.is_contiguous() and gtp.is_contiguous()
    boxes = torch.empty(B, R, 4, device=dev, dtype=torch.float32)
    gt = torch.empty(B, R, 4, device=dev, dtype=torch.float32)
    labels = torch.empty(B, R, device=dev, dtype=torch.int64)
    valid = torch.empty(B, R, device=dev, dtype=torch.bool)
    _chk(lib().ore_sample_rois_fwd(_ptr(_f32(prop)), _ptr(prop_n), _ptr(_f32(gtp)), _ptr(gt_n), _ptr(keys), B, cap, G, int(bool(append_gt)),
                                   R, P, iou_thr, _ptr(boxes), _ptr(labels), _ptr(gt), _ptr(valid), _stream()), "ore_sample_rois_fwd")
    return boxes, labels, gt, valid


def roi_losses(scores: torch.Tensor, deltas: torch.Tensor, boxes: torch.Tensor, gt: torch.Tensor, labels: torch.Tensor, valid: torch.Tensor,
               B: int, R: int, reg_weights) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The second stage's two losses and their gradients in one launch (ore_roi_losses_fwd): scores [B*R,2], deltas / boxes / gt [B*R,4],
    labels [B*R] int64 (0 fg / 1 bg), valid [B*R] bool -> (losses [2] = (cls, box), dscores [B*R,2], ddeltas [B*R,4])."""
    RT = B * R
    dev = scores.device
    assert scores.shape == (RT, 2) and deltas.shape == (RT, 4) and boxes.shape == (RT, 4) and gt.shape == (RT, 4)
    assert labels.dtype == torch.int64 and labels.numel() == RT and valid.dtype == torch.bool and valid.numel() == RT
    out = torch.empty(2, device=dev, dtype=torch.float32)
    ds = torch.empty(RT, 2, device=dev, dtype=torch.float32)
    dd = torch.empty(RT, 4, device=dev, dtype=torch.float32)
    rw = (C.c_float * 4)(*[float(v) for v in reg_weights])
    _chk(lib().ore_roi_losses_fwd(_ptr(_f32(scores)), _ptr(_f32(deltas)), _ptr(_f32(boxes)), _ptr(_f32(gt)), _ptr(labels.contiguous()),
                                  _ptr(valid.contiguous()), B, R, rw, _ptr(out), _ptr(ds), _ptr(dd), _stream()), "ore_roi_losses_fwd")
    return out, ds, dd


def sgd_step(params: torch.Tensor, grads: torch.Tensor, momentum_buf: torch.Tensor, chunk_lr: torch.Tensor, chunk_wd: torch.Tensor,
             lr_scale: float = 1.0, momentum: float = 0.9, clip_value: float = 1.0, grad_scale: float = 1.0,
             lr_scale_dev: Optional[torch.Tensor] = None) -> None:
    """In-place clip + SGD over a flat bucket of 256-float chunks (see ore_sgd_step_fwd)."""
    n = params.numel()
    assert n % 256 == 0 and grads.numel() == n and momentum_buf.numel() == n and chunk_lr.numel() == n // 256 == chunk_wd.numel()
    for t in (params, grads, momentum_buf, chunk_lr, chunk_wd):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
    _chk(lib().ore_sgd_step_fwd(_ptr(params), _ptr(grads), _ptr(momentum_buf), n // 256, _ptr(chunk_lr), _ptr(chunk_wd), _ptr(lr_scale_dev),
                                lr_scale, momentum, clip_value, grad_scale, _stream()), "ore_sgd_step_fwd")


GRAD_NORM_KINDS = {2.0: 2, 1.0: 1, float("inf"): 0}          # NORM_TYPE -> ore_grad_norm_fwd's norm_kind


def grad_norm_geometry() -> Tuple[int, int]:
    """(chunks of 256 floats one partial sum covers, partials one pass of the per-parameter reduction takes) of ore_grad_norm_fwd."""
    g, w = C.c_int32(), C.c_int32()
    _chk(lib().ore_grad_norm_geometry(C.byref(g), C.byref(w)), "ore_grad_norm_geometry")
    return g.value, w.value


def grad_norm_workspace(numels, device) -> Dict[str, torch.Tensor]:
    """Everything ore_grad_norm_fwd needs besides the bucket's own tables, sized once (ore_grad_norm_plan): the device tables part0 /
    part_param, the workspaces partial / acc and the outputs norm / coef / total (NaN until a launch writes them)."""
    P = len(numels)
    ne = (C.c_int64 * P)(*[int(n) for n in numels])
    nc, npart = C.c_int64(), C.c_int64()
    _chk(lib().ore_grad_norm_plan(ne, P, None, None, 0, C.byref(nc), C.byref(npart)), "ore_grad_norm_plan")
    part0, part_param = (C.c_int32 * (P + 1))(), (C.c_int32 * npart.value)()
    _chk(lib().ore_grad_norm_plan(ne, P, part0, part_param, npart.value, C.byref(nc), C.byref(npart)), "ore_grad_norm_plan")
    nan = lambda n: torch.full((n,), float("nan"), dtype=torch.float32, device=device)   # noqa: E731
    return {"n_params": P, "n_chunks": nc.value, "n_parts": npart.value,
            "part0": torch.tensor(list(part0), dtype=torch.int32, device=device),
            "part_param": torch.tensor(list(part_param), dtype=torch.int32, device=device),
            "partial": nan(npart.value), "acc": nan(P), "norm": nan(P), "coef": nan(P), "total": nan(1)}


def grad_norms(grads: torch.Tensor, param_numel: torch.Tensor, param_chunk0: torch.Tensor, ws: Dict[str, torch.Tensor],
               norm_type: float = 2.0, full_model: bool = False, clip_value: float = 1.0,
               grad_scale: float = 1.0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The p-norms of grad_scale * gradient over a flat bucket and the clip coefficients min(clip_value / (norm + 1e-6), 1) (see
    ore_grad_norm_fwd) -> ws's device tensors (norm [P], coef [P], total [1]); total is written in full-model mode only.  param_numel /
    param_chunk0: the bucket's int64 tables; ws: grad_norm_workspace(numels).  No host read, no allocation: capturable."""
    if float(norm_type) not in GRAD_NORM_KINDS:
        raise NotImplementedError(f"NORM_TYPE {norm_type}: only 2, 1 and inf are built")
    P = ws["n_params"]
    assert grads.is_cuda and grads.dtype == torch.float32 and grads.is_contiguous() and grads.numel() == ws["n_chunks"] * 256
    assert param_numel.dtype == torch.int64 and param_chunk0.dtype == torch.int64 and param_numel.numel() == P == param_chunk0.numel()
    _chk(lib().ore_grad_norm_fwd(_ptr(grads), P, _ptr(param_numel), _ptr(param_chunk0), _ptr(ws["part_param"]), _ptr(ws["part0"]),
                                 ws["n_parts"], GRAD_NORM_KINDS[float(norm_type)], int(bool(full_model)), clip_value, grad_scale,
                                 _ptr(ws["partial"]), _ptr(ws["acc"]), _ptr(ws["norm"]), _ptr(ws["coef"]), _ptr(ws["total"]), _stream()),
         "ore_grad_norm_fwd")
    return ws["norm"], ws["coef"], ws["total"]


def sgd_step_norm(params: torch.Tensor, grads: torch.Tensor, momentum_buf: torch.Tensor, chunk_lr: torch.Tensor, chunk_wd: torch.Tensor,
                  chunk_param: torch.Tensor, param_numel: torch.Tensor, param_chunk0: torch.Tensor, coef: Optional[torch.Tensor],
                  lr_scale: float = 1.0, momentum: float = 0.9, clip_value: float = 1.0, grad_scale: float = 1.0,
                  nesterov: bool = False, lr_scale_dev: Optional[torch.Tensor] = None) -> None:
    """In-place SGD over a flat bucket with the gradient multiplied by coef[parameter] (grad_norms), or value-clamped when coef is
    None; Nesterov momentum on request (see ore_sgd_step_clipnorm_fwd)."""
    n = params.numel()
    assert n % 256 == 0 and grads.numel() == n and momentum_buf.numel() == n and chunk_lr.numel() == n // 256 == chunk_wd.numel()
    assert chunk_param.numel() == n // 256 and chunk_param.dtype == torch.int32
    assert param_numel.dtype == torch.int64 and param_chunk0.dtype == torch.int64 and param_numel.numel() == param_chunk0.numel()
    assert coef is None or (coef.dtype == torch.float32 and coef.numel() == param_numel.numel())
    for t in (params, grads, momentum_buf, chunk_lr, chunk_wd):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
    _chk(lib().ore_sgd_step_clipnorm_fwd(_ptr(params), _ptr(grads), _ptr(momentum_buf), n // 256, _ptr(chunk_lr), _ptr(chunk_wd),
                                         _ptr(chunk_param), _ptr(param_numel), _ptr(param_chunk0), _ptr(coef), _ptr(lr_scale_dev),
                                         lr_scale, momentum, clip_value, grad_scale, int(bool(nesterov)), _stream()),
         "ore_sgd_step_clipnorm_fwd")


def pack_conv_weight_dev(w_oihw: torch.Tensor, dgrad: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Device-side repack of OIHW master weights (runs every optimizer step): forward layout [Cout16][tap][Cin], or the
    data-gradient layout [Cin16][flipped tap][Cout16]."""
    w = _f32(w_oihw.detach())
    co, ci, kh, kw = w.shape
    co16, ci16 = (co + 15) // 16 * 16, (ci + 15) // 16 * 16
    n = ci16 * kh * kw * co16 if dgrad else co16 * kh * kw * ci
    if out is None:
        out = torch.empty(n, device=w.device, dtype=torch.float32)
    assert out.numel() == n
    _chk(lib().ore_pack_conv_weight_fwd(_ptr(w), co, ci, kh, kw, int(dgrad), _ptr(out), _stream()), "ore_pack_conv_weight_fwd")
    return out


class PackJob(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("Cout", C.c_int32), ("Cin", C.c_int32), ("kh", C.c_int32), ("kw", C.c_int32),
                ("dgrad", C.c_int32), ("reserved", C.c_int32), ("first", C.c_int64)]


_PACK_TABLES: Dict[tuple, torch.Tensor] = {}


def pack_conv_weights_multi(jobs) -> None:
    """jobs: [(w_oihw contiguous fp32 device tensor, dgrad, out)] -> every `out` holds pack_conv_weight_dev(w, dgrad): ONE launch
    (ore_pack_conv_weights_multi_fwd).  The device-side job table is cached by its contents (pointers and shapes): a training loop hands
    the same list every step, and a captured step replays the launch on the same table."""
    if not jobs:
        return
    assert len(jobs) <= 256
    dev = jobs[0][0].device
    rows, first = [], 0
    for w, dgrad, out in jobs:
        co, ci, kh, kw = w.shape
        co16, ci16 = (co + 15) // 16 * 16, (ci + 15) // 16 * 16
        n = ci16 * kh * kw * co16 if dgrad else co16 * kh * kw * ci
        assert w.is_contiguous() and w.dtype == torch.float32 and out.numel() == n and (dgrad or ci % 16 == 0)
        rows.append((_ptr(w), _ptr(out), co, ci, kh, kw, int(bool(dgrad)), first))
        first += n
    key = (str(dev), tuple(rows))
    tab = _PACK_TABLES.get(key)
    if tab is None:
        arr = (PackJob * len(rows))()
        for i, (src, dst, co, ci, kh, kw, dg, f) in enumerate(rows):
            arr[i] = PackJob(src, dst, co, ci, kh, kw, dg, 0, f)
        host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).clone()
        if len(_PACK_TABLES) > 64:
            _PACK_TABLES.clear()
        tab = _PACK_TABLES[key] = host.to(dev)
    _chk(lib().ore_pack_conv_weights_multi_fwd(_ptr(tab), len(rows), first, _stream()), "ore_pack_conv_weights_multi_fwd")


_WGWS: Dict[str, torch.Tensor] = {}


def _wgrad_ws(device, n: int) -> torch.Tensor:
    k = str(device)
    if k not in _WGWS or _WGWS[k].numel() < n:
        _WGWS[k] = torch.empty(max(n, 16 << 20), device=device, dtype=torch.float32)
    return _WGWS[k]


def conv2d_wgrad(x: torch.Tensor, dz: torch.Tensor, k: int, *, x_coff: int = 0, Cin: Optional[int] = None, dz_coff: int = 0,
                 Cout: Optional[int] = None, out: Optional[torch.Tensor] = None, beta: float = 0.0, want_bias: bool = False,
                 db_out: Optional[torch.Tensor] = None, beta_b: float = 0.0):
    """x [B,H,W,x_ld], dz [B,H,W,dz_ld] NHWC -> dW [Cout,Cin,k,k] (OIHW); stride 1, pad k//2.  want_bias: also the bias gradient
    (column sums of dz) from the same launch -> (dW, db).  out / beta, db_out / beta_b: dW = beta * out + ..., db = beta_b * db_out + ...
    written in place (a parameter's gradient accumulated by the launch itself)."""
    _f32(x); _f32(dz)
    B, H, W, xld = x.shape
    dld = dz.shape[-1]
    assert dz.shape[:3] == (B, H, W)
    Cin = Cin if Cin is not None else xld - x_coff
    Cout = Cout if Cout is not None else dld - dz_coff
    if out is None:
        out = torch.empty(Cout, Cin, k, k, device=x.device, dtype=torch.float32)
        beta = 0.0
    assert out.shape == (Cout, Cin, k, k) and out.is_contiguous()
    n = lib().ore_conv_wgrad_workspace_floats(B * H * W, Cin, Cout, k, k)
    ws = _wgrad_ws(x.device, n)
    if want_bias and db_out is not None:
        assert db_out.shape == (Cout,) and db_out.is_contiguous() and db_out.dtype == torch.float32
        db = db_out
    else:
        db, beta_b = (torch.empty(Cout, device=x.device, dtype=torch.float32) if want_bias else None), 0.0
    _chk(lib().ore_conv2d_wgrad_bias_fwd(_ptr(x), xld, x_coff, _ptr(dz), dld, dz_coff, B, H, W, Cin, Cout, k, k, k // 2, _ptr(out), beta,
                                         _ptr(db), beta_b, _ptr(ws), ws.numel(), _stream()), "ore_conv2d_wgrad_bias_fwd")
    return (out, db) if want_bias else out


def _s2_out_hw(H: int, W: int) -> Tuple[int, int]:
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def _s2_image_groups(B: int, *bytes_per_image: int) -> List[Tuple[int, int]]:
    """Whole-image groups of a stride-2 gradient launch, each tensor below orehip._S2_MAX_BYTES (explained where it is defined)."""
    nb = max(1, min(B, orehip._S2_MAX_BYTES // max(bytes_per_image)))
    return [(b0, min(B, b0 + nb)) for b0 in range(0, B, nb)]


def conv2d_wgrad_s2(x: torch.Tensor, dz: torch.Tensor, *, x_coff: int = 0, Cin: Optional[int] = None, dz_coff: int = 0,
                    Cout: Optional[int] = None, out: Optional[torch.Tensor] = None, beta: float = 0.0,
                    workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [B,H,W,x_ld], dz [B,Ho,Wo,dz_ld] NHWC -> dW [Cout,Cin,3,3] of the 3x3 / stride 2 / pad 1 conv (ore_conv2d_wgrad_s2_fwd, fp32 in
    every precision mode, deterministic).  out / beta: dW = beta * out + ... in place.  The workspace is the weight-gradient one
    (allocated outside any capture by the first eager call, reused); `workspace`: the caller's instead (a smaller one caps the row split)."""
    _f32(x); _f32(dz)
    B, H, W, xld = x.shape
    dld = dz.shape[-1]
    assert tuple(dz.shape[:3]) == (B, *_s2_out_hw(H, W)), (tuple(dz.shape), tuple(x.shape))
    Cin = Cin if Cin is not None else xld - x_coff
    Cout = Cout if Cout is not None else dld - dz_coff
    if out is None:
        out = torch.empty(Cout, Cin, 3, 3, device=x.device, dtype=torch.float32)
        beta = 0.0
    assert out.shape == (Cout, Cin, 3, 3) and out.is_contiguous() and out.dtype == torch.float32
    for i, (b0, b1) in enumerate(_s2_image_groups(B, H * W * xld * 4, dz.shape[1] * dz.shape[2] * dld * 4)):
        rows = (b1 - b0) * dz.shape[1] * dz.shape[2]
        ws = workspace if workspace is not None else _wgrad_ws(x.device, lib().ore_conv_wgrad_s2_workspace_floats(rows, Cin, Cout))
        _chk(lib().ore_conv2d_wgrad_s2_fwd(_ptr(x[b0:b1]), xld, x_coff, _ptr(dz[b0:b1]), dld, dz_coff, b1 - b0, H, W, Cin, Cout, _ptr(out),
                                           beta if i == 0 else 1.0, _ptr(ws), ws.numel(), _stream()), "ore_conv2d_wgrad_s2_fwd")
    return out


def conv2d_dgrad_s2(dz: torch.Tensor, w_oihw: torch.Tensor, H: int, W: int, *, dz_coff: int = 0, out: Optional[torch.Tensor] = None,
                    out_coff: int = 0) -> torch.Tensor:
    """dz [B,Ho,Wo,dz_ld], w [Cout,Cin,3,3] -> dX [B,H,W,Cin] of the 3x3 / stride 2 / pad 1 conv over an H x W input
    (ore_conv2d_dgrad_s2_fwd: parity decomposition, fp32, deterministic).  out / out_coff: write channels [out_coff, out_coff + Cin) of a
    wider buffer.  The packed weights live in the weight-gradient workspace (stream-ordered behind whatever used it last)."""
    _f32(dz); _f32(w_oihw)
    Cout, Cin = w_oihw.shape[:2]
    assert tuple(w_oihw.shape[2:]) == (3, 3)
    B = dz.shape[0]
    assert tuple(dz.shape[1:3]) == _s2_out_hw(H, W) and dz_coff + Cout <= dz.shape[-1], (tuple(dz.shape), H, W)
    if out is None:
        out = torch.empty(B, H, W, Cin, device=dz.device, dtype=torch.float32)
    _f32(out)
    assert tuple(out.shape[:3]) == (B, H, W)
    ws = _wgrad_ws(dz.device, lib().ore_conv_dgrad_s2_workspace_floats(Cin, Cout))
    for b0, b1 in _s2_image_groups(B, dz.shape[1] * dz.shape[2] * dz.shape[-1] * 4, H * W * out.shape[-1] * 4):
        _chk(lib().ore_conv2d_dgrad_s2_fwd(_ptr(dz[b0:b1]), dz.shape[-1], dz_coff, _ptr(w_oihw), b1 - b0, H, W, Cin, Cout, _ptr(out[b0:b1]),
                                           out.shape[-1], out_coff, _ptr(ws), ws.numel(), _stream()), "ore_conv2d_dgrad_s2_fwd")
    return out


def stem1_wgrad(img: torch.Tensor, Hp: int, Wp: int, mean: Sequence[float], std: Sequence[float], dz: torch.Tensor, *, dz_coff: int = 0,
                Cout: Optional[int] = None, out: Optional[torch.Tensor] = None, beta: float = 0.0,
                workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """img [B,3,H,W] uint8 or fp32 (planar, raw), dz [B,Hp/2,Wp/2,dz_ld] -> dW [Cout,3,3,3] of stem_1 (ore_stem1_wgrad_fwd): the
    normalisation and the zero padding to (Hp, Wp) are formed on the fly as in stem1().  out / beta: dW = beta * out + ... in place."""
    assert img.is_contiguous() and img.dtype in (torch.uint8, torch.float32)
    _f32(dz)
    B, _, H, W = img.shape
    assert tuple(dz.shape[:3]) == (B, Hp // 2, Wp // 2), (tuple(dz.shape), Hp, Wp)
    Cout = Cout if Cout is not None else dz.shape[-1] - dz_coff
    if out is None:
        out = torch.empty(Cout, 3, 3, 3, device=img.device, dtype=torch.float32)
        beta = 0.0
    assert out.numel() == Cout * 27 and out.is_contiguous() and out.dtype == torch.float32
    m = (C.c_float * 3)(*mean)
    s = (C.c_float * 3)(*std)
    for i, (b0, b1) in enumerate(_s2_image_groups(B, (Hp // 2) * (Wp // 2) * dz.shape[-1] * 4, 3 * H * W * img.element_size())):
        rows = (b1 - b0) * (Hp // 2) * (Wp // 2)
        ws = workspace if workspace is not None else _wgrad_ws(img.device, lib().ore_stem1_wgrad_workspace_floats(rows, Cout))
        _chk(lib().ore_stem1_wgrad_fwd(_ptr(img[b0:b1]), int(img.dtype == torch.uint8), b1 - b0, H, W, Hp, Wp, m, s, _ptr(dz[b0:b1]), dz.shape[-1],
                                       dz_coff, Cout, _ptr(out), beta if i == 0 else 1.0, _ptr(ws), ws.numel(), _stream()), "ore_stem1_wgrad_fwd")
    return out


def _dw_out(x: torch.Tensor, C: int, stride: int, out: Optional[torch.Tensor]) -> torch.Tensor:
    B, H, W, _ = x.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    if out is None:
        out = torch.empty(B, Ho, Wo, C, device=x.device, dtype=torch.float32)
    _f32(out)
    assert out.shape[:3] == (B, Ho, Wo), (tuple(out.shape), (B, Ho, Wo))
    return out


def dwpw(x: torch.Tensor, w_dw: torch.Tensor, w_pw_packed: torch.Tensor, C: int, stride: int = 1, scale=None, shift=None, *,
         in_coff: int = 0, out: Optional[torch.Tensor] = None, out_coff: int = 0, fused: Optional[bool] = None) -> torch.Tensor:
    """One depthwise-separable unit of the *-dw-* VoVNet bodies in one launch (ore_dwpw_fwd): depthwise 3x3 (stride 1 | 2, pad 1) ->
    pointwise 1x1 -> scale / shift (folded FrozenBN) -> ReLU.  x [B,H,W,ld] NHWC fp32, channels [in_coff, in_coff + C) are read;
    w_dw [C,1,3,3]; w_pw_packed = pack_conv_weight of the [C,C,1,1] weight; channels [out_coff, out_coff + C) of `out` are written
    (x and out may be one buffer when the slices do not overlap).  fp32 in every conv precision mode.
    fused=None: the library's planner (ore_dwpw_planned_fwd) -- the fused launch, except at stride 1 with rows * C >= 2^22 (dwpw_prefers_composition:
    stem_2 at 640x640), where the depthwise conv goes through a scratch tensor to the 1x1 conv launch; fused=True: always k_dwpw."""
    _f32(x); _f32(w_dw); _f32(w_pw_packed)
    assert w_dw.numel() == C * 9 and w_pw_packed.numel() == C * C, (tuple(w_dw.shape), w_pw_packed.numel(), C)
    assert out is None or out.data_ptr() != x.data_ptr() or in_coff + C <= out_coff or out_coff + C <= in_coff, "overlapping slices"
    out = _dw_out(x, C, stride, out)
    B, H, W, ld = x.shape
    rows = out.shape[0] * out.shape[1] * out.shape[2]
    if fused is None and dwpw_prefers_composition(rows, C, stride):
        scratch = torch.empty(rows * C, device=x.device, dtype=torch.float32)
        _chk(lib().ore_dwpw_planned_fwd(_ptr(x), ld, in_coff, B, H, W, C, stride, _ptr(w_dw), _ptr(w_pw_packed), _ptr(scale), _ptr(shift),
                                        _ptr(out), out.shape[-1], out_coff, _ptr(scratch), scratch.numel(), _stream()), "ore_dwpw_planned_fwd")
        return out
    assert fused is not False or not dwpw_prefers_composition(rows, C, stride), "fused=False: the planner's choice is the only unfused form"
    _chk(lib().ore_dwpw_fwd(_ptr(x), ld, in_coff, B, H, W, C, stride, _ptr(w_dw), _ptr(w_pw_packed), _ptr(scale), _ptr(shift), _ptr(out),
                            out.shape[-1], out_coff, _stream()), "ore_dwpw_fwd")
    return out


def dwpw_prefers_composition(rows: int, C: int, stride: int = 1) -> bool:
    """True where orehip.dwpw / the engine run a unit as k_dw3x3 + the 1x1 conv launch instead of k_dwpw (ore_dwpw_prefers_composition)."""
    return bool(lib().ore_dwpw_prefers_composition(int(rows), int(C), int(stride)))


def dw3x3(x: torch.Tensor, w_dw: torch.Tensor, C: int, stride: int = 1, *, in_coff: int = 0, out: Optional[torch.Tensor] = None,
          out_coff: int = 0, dgrad: bool = False, accumulate: bool = False) -> torch.Tensor:
    """The depthwise 3x3 alone (ore_dw3x3_fwd), slices as in dwpw.  dgrad: mirrored taps = the data gradient of a stride-1 unit (x is
    then dT); stride 2 is refused there.  accumulate: out[..., slice] += result."""
    _f32(x); _f32(w_dw)
    assert w_dw.numel() == C * 9
    out = _dw_out(x, C, stride, out)
    B, H, W, ld = x.shape
    _chk(lib().ore_dw3x3_fwd(_ptr(x), ld, in_coff, B, H, W, C, stride, _ptr(w_dw), int(bool(dgrad)), _ptr(out), out.shape[-1], out_coff,
                             int(bool(accumulate)), _stream()), "ore_dw3x3_fwd")
    return out


def dw3x3_wgrad(x: torch.Tensor, dt: torch.Tensor, C: int, *, x_coff: int = 0, dt_coff: int = 0, out: Optional[torch.Tensor] = None,
                beta: float = 0.0) -> torch.Tensor:
    """x [B,H,W,x_ld], dt [B,H,W,dt_ld] -> dW [C,1,3,3] of the stride-1 depthwise conv (ore_dw3x3_wgrad_fwd): deterministic, fixed split
    and combine order.  out / beta: dW = beta * out + ... in place.  The workspace is the weight-gradient one (allocated outside any
    capture by the first eager call, like conv2d_wgrad's)."""
    _f32(x); _f32(dt)
    B, H, W, xld = x.shape
    assert dt.shape[:3] == (B, H, W)
    if out is None:
        out = torch.empty(C, 1, 3, 3, device=x.device, dtype=torch.float32)
        beta = 0.0
    assert out.numel() == C * 9 and out.is_contiguous() and out.dtype == torch.float32
    ws = _wgrad_ws(x.device, lib().ore_dw3x3_wgrad_workspace_floats(B * H * W, C))
    _chk(lib().ore_dw3x3_wgrad_fwd(_ptr(x), xld, x_coff, _ptr(dt), dt.shape[-1], dt_coff, B, H, W, C, _ptr(out), beta, _ptr(ws), ws.numel(),
                                   _stream()), "ore_dw3x3_wgrad_fwd")
    return out


def relu_affine_bwd(dy: torch.Tensor, y: torch.Tensor, scale: Optional[torch.Tensor] = None, *, dy_coff: int = 0, y_coff: int = 0,
                    Cc: Optional[int] = None, out: Optional[torch.Tensor] = None, out_coff: int = 0) -> torch.Tensor:
    """dZ = dY * (Y > 0) * scale over channel slices of NHWC/row-major buffers (last dim = ld)."""
    _f32(dy); _f32(y)
    Cc = Cc if Cc is not None else y.shape[-1] - y_coff
    rows = y.numel() // y.shape[-1]
    if out is None:
        out = torch.empty(*y.shape[:-1], Cc, device=y.device, dtype=torch.float32)
    _chk(lib().ore_relu_affine_bwd(_ptr(dy), dy.shape[-1], dy_coff, _ptr(y), y.shape[-1], y_coff, _ptr(scale), rows, Cc, _ptr(_f32(out)),
                                   out.shape[-1], out_coff, _stream()), "ore_relu_affine_bwd")
    return out


def colsum(x: torch.Tensor, *, coff: int = 0, Cc: Optional[int] = None, out: Optional[torch.Tensor] = None, beta: float = 0.0) -> torch.Tensor:
    """Bias gradient: sums over all leading dims of x[..., coff:coff+Cc]."""
    _f32(x)
    ld = x.shape[-1]
    Cc = Cc if Cc is not None else ld - coff
    rows = x.numel() // ld
    if out is None:
        out = torch.empty(Cc, device=x.device, dtype=torch.float32)
        beta = 0.0
    ws = _wgrad_ws(x.device, ((rows + 63) // 64) * Cc)
    _chk(lib().ore_colsum_fwd(_ptr(x), ld, coff, rows, Cc, beta, _ptr(out), _ptr(ws), ws.numel(), _stream()), "ore_colsum_fwd")
    return out


def colsum_segments(x: torch.Tensor, segments: int) -> torch.Tensor:
    """x [rows, C] made of `segments` equal runs of rows (the images of a batch) -> [segments, C] per-run column sums; each run's sums
    are bitwise those of `colsum` on that run alone (ore_colsum_segments_fwd)."""
    _f32(x)
    rows, Cc = x.shape
    assert rows % segments == 0
    rps = rows // segments
    out = torch.empty(segments, Cc, device=x.device, dtype=torch.float32)
    ws = _wgrad_ws(x.device, segments * ((rps + 255) // 256) * Cc)
    _chk(lib().ore_colsum_segments_fwd(_ptr(x), Cc, 0, segments, rps, Cc, 0.0, _ptr(out), _ptr(ws), ws.numel(), _stream()),
         "ore_colsum_segments_fwd")
    return out


def correlation_train_fwd(q: torch.Tensor, k11: torch.Tensor, k13: torch.Tensor, k31: torch.Tensor):
    """q [B,H,W,C]; k11 [C], k13 / k31 [C,3] shared by the B images, or [B,C] / [B,C,3] = one support kernel set per image
    -> (cat [B,H,W,2C] = [attn | q], t, u)."""
    _f32(q)
    B, H, W, Cc = q.shape
    per_image = int(k11.dim() == 2)
    assert k11.numel() == (B if per_image else 1) * Cc and k13.numel() == k31.numel() == 3 * k11.numel()
    cat = torch.empty(B, H, W, 2 * Cc, device=q.device, dtype=torch.float32)
    t = torch.empty(B, H, W, Cc, device=q.device, dtype=torch.float32)
    u = torch.empty_like(t)
    _chk(lib().ore_correlation_train_fwd(_ptr(q), Cc, 0, B, H, W, Cc, _ptr(_f32(k11)), _ptr(_f32(k13)), _ptr(_f32(k31)), per_image,
                                         _ptr(cat), _ptr(t), _ptr(u), _stream()), "ore_correlation_train_fwd")
    return cat, t, u


def correlation_train_bwd(q, k11, k13, k31, dcat, t, u):
    """-> dq [B,H,W,C], dk11, dk13, dk31 shaped like k11 / k13 / k31."""
    B, H, W, Cc = q.shape
    rows = B * H * W
    per_image = int(k11.dim() == 2)
    S = B if per_image else 1
    dq = torch.empty_like(q)
    dk = torch.empty(S, 7, Cc, device=q.device, dtype=torch.float32)
    ws = _wgrad_ws(q.device, rows * Cc * 8 + S * ((rows // S + 255) // 256) * 7 * Cc)
    _chk(lib().ore_correlation_train_bwd(_ptr(_f32(q)), Cc, 0, B, H, W, Cc, _ptr(_f32(k11)), _ptr(_f32(k13)), _ptr(_f32(k31)), per_image,
                                         _ptr(_f32(dcat)), _ptr(t), _ptr(u), _ptr(dq), _ptr(dk), _ptr(ws), ws.numel(), _stream()),
         "ore_correlation_train_bwd")
    d11, d13, d31 = dk[:, 0], dk[:, 1:4].transpose(1, 2).contiguous(), dk[:, 4:7].transpose(1, 2).contiguous()
    if not per_image:
        d11, d13, d31 = d11[0], d13[0], d31[0]
    return dq, d11.contiguous(), d13, d31


def groupnorm_apply(x: torch.Tensor, rstd_c: torch.Tensor, shift_c: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, relu: bool):
    """x [B,H,W,C], rstd_c / shift_c [B,C] (per image) -> relu?((x*rstd_c + shift_c)*gamma + beta)."""
    _f32(x)
    B, Cc = x.shape[0], x.shape[-1]
    rpi = x.numel() // (Cc * B)
    assert rstd_c.numel() == B * Cc and shift_c.numel() == B * Cc
    y = torch.empty_like(x)
    _chk(lib().ore_groupnorm_apply_fwd(_ptr(x), Cc, 0, B, rpi, Cc, _ptr(_f32(rstd_c)), _ptr(_f32(shift_c)), _ptr(_f32(gamma)),
                                       _ptr(_f32(beta)), int(relu), _ptr(y), _stream()), "ore_groupnorm_apply_fwd")
    return y


def groupnorm_bwd(dy, y, x, groups: int, rstd_c, shift_c, gamma, relu: bool):
    """x [B,H,W,C], rstd_c / shift_c [B,C] -> dx like x, dbeta [B,C], dgamma [B,C] (per image; sum over B for the parameters)."""
    _f32(dy); _f32(y); _f32(x)
    B, Cc = x.shape[0], x.shape[-1]
    rpi = x.numel() // (Cc * B)
    dx = torch.empty_like(x)
    sums = torch.empty(B, 2 * Cc, device=x.device, dtype=torch.float32)
    ws = _wgrad_ws(x.device, B * rpi * 2 * Cc + B * ((rpi + 255) // 256) * 2 * Cc)
    _chk(lib().ore_groupnorm_bwd(_ptr(dy), _ptr(y), _ptr(x), Cc, 0, B, rpi, Cc, groups, _ptr(_f32(rstd_c)), _ptr(_f32(shift_c)),
                                 _ptr(_f32(gamma)), int(relu), _ptr(dx), _ptr(sums), _ptr(ws), ws.numel(), _stream()), "ore_groupnorm_bwd")
    return dx, sums[:, :Cc], sums[:, Cc:]


def prod_colsum(p: torch.Tensor, q: Optional[torch.Tensor] = None, scale: float = 1.0) -> torch.Tensor:
    """p (, q) [B,H,W,C] -> [B,C]: per-image sum over pixels of p (* q), times scale."""
    _f32(p)
    B, Cc = p.shape[0], p.shape[-1]
    rows = p.numel() // (B * Cc)
    out = torch.empty(B, Cc, device=p.device, dtype=torch.float32)
    ws = _wgrad_ws(p.device, p.numel())
    _chk(lib().ore_prod_colsum_fwd(_ptr(p), _ptr(_f32(q)) if q is not None else None, B, rows, Cc, scale, _ptr(out), _ptr(ws), ws.numel(),
                                   _stream()), "ore_prod_colsum_fwd")
    return out


def scale_add_channels(x: torch.Tensor, scale_bc: torch.Tensor, add_bc: Optional[torch.Tensor] = None) -> torch.Tensor:
    _f32(x)
    B, Cc = x.shape[0], x.shape[-1]
    rows = x.numel() // (B * Cc)
    out = torch.empty_like(x)
    _chk(lib().ore_scale_add_channels_fwd(_ptr(x), _ptr(_f32(scale_bc)), _ptr(_f32(add_bc)) if add_bc is not None else None, B, rows, Cc,
                                          _ptr(out), _stream()), "ore_scale_add_channels_fwd")
    return out


def adaptive_avgpool_nhwc(x: torch.Tensor, OH: int, OW: int, grad_of: Optional[Tuple[int, int]] = None) -> torch.Tensor:
    """F.adaptive_avg_pool2d on an NHWC map: x [B,H,W,C] -> [B,OH,OW,C].  grad_of=(H, W): x is the gradient w.r.t. the pooled map
    [B,OH,OW,C] and the result is the gradient w.r.t. the [B,H,W,C] input."""
    _f32(x)
    B, Cc = x.shape[0], x.shape[-1]
    if grad_of is None:
        H, W = x.shape[1:3]
        y = torch.empty(B, OH, OW, Cc, device=x.device, dtype=torch.float32)
        _chk(lib().ore_adaptive_avgpool_nhwc_fwd(_ptr(x), B, H, W, Cc, OH, OW, _ptr(y), _stream()), "ore_adaptive_avgpool_nhwc_fwd")
        return y
    H, W = grad_of
    assert tuple(x.shape[1:3]) == (OH, OW)
    dx = torch.empty(B, H, W, Cc, device=x.device, dtype=torch.float32)
    _chk(lib().ore_adaptive_avgpool_nhwc_bwd(_ptr(x), B, H, W, Cc, OH, OW, _ptr(dx), _stream()), "ore_adaptive_avgpool_nhwc_bwd")
    return dx


def group_mean(x: torch.Tensor, groups: int, backward: bool = False, members: int = 0) -> torch.Tensor:
    """x [groups*N, ...] -> [groups, ...]: mean over the N consecutive members of each group (the prototype over an image's shots);
    backward=True: x [groups, ...] is the gradient of that mean -> [groups*members, ...]."""
    _f32(x)
    if not backward:
        N = x.shape[0] // groups
        assert N * groups == x.shape[0]
        M = x.numel() // x.shape[0]
        y = torch.empty(groups, *x.shape[1:], device=x.device, dtype=torch.float32)
        _chk(lib().ore_group_mean_fwd(_ptr(x), groups, N, M, _ptr(y), _stream()), "ore_group_mean_fwd")
        return y
    M = x.numel() // groups
    dx = torch.empty(groups * members, *x.shape[1:], device=x.device, dtype=torch.float32)
    _chk(lib().ore_group_mean_bwd(_ptr(x), groups, members, M, _ptr(dx), _stream()), "ore_group_mean_bwd")
    return dx


def sm_permute(x: torch.Tensor, B: int, H: int, W: int, G: int, S: int, axis: str, inverse: bool, out: Optional[torch.Tensor] = None,
               accumulate: bool = False) -> torch.Tensor:
    """The SM_Block's mixing layouts as one coalesced pass (ore_granule_transpose_fwd).  axis 'h': [B,H,W,G,S] <-> [B,G,W,H,S]
    (= .permute(0,3,2,1,4)); axis 'w': [B,H,W,G,S] <-> [B,G,H,W,S] (= .permute(0,3,1,2,4) and back).  x contiguous with B*H*W*G*S elements;
    returns a contiguous tensor in the other layout (forward: the mixing layout, inverse: NHWC).  out + accumulate: out += the result."""
    _f32(x)
    assert x.numel() == B * H * W * G * S and axis in ("h", "w")
    Cc, img = G * S, H * W * G * S
    if axis == "h":
        nb2, mix = W, (B, G, W, H, S)
        fwd = (H, G, img, Cc, W * Cc, img, H * S, W * H * S)          # A, Bc, in_b1, in_b2, in_rs, out_b1, out_b2, out_rs
        inv = (G, H, img, H * S, W * H * S, img, Cc, W * Cc)
    else:
        nb2, mix = H, (B, G, H, W, S)
        fwd = (W, G, img, W * Cc, Cc, img, W * S, H * W * S)
        inv = (G, W, img, W * S, H * W * S, img, W * Cc, Cc)
    A_, Bc, ib1, ib2, irs, ob1, ob2, ors = inv if inverse else fwd
    if out is None:
        assert not accumulate
        out = torch.empty((B, H, W, G * S) if inverse else mix, device=x.device, dtype=torch.float32)
    else:
        _f32(out)
        assert out.numel() == x.numel()
    _chk(lib().ore_granule_transpose_fwd(_ptr(x), _ptr(out), B, nb2, A_, Bc, S, ib1, ib2, irs, ob1, ob2, ors, int(accumulate), _stream()),
         "ore_granule_transpose_fwd")
    return out


def combine2(w: torch.Tensor, h: torch.Tensor, a0: torch.Tensor, a1: torch.Tensor) -> torch.Tensor:
    """y = w * a0[b, c] + h * a1[b, c];  w, h [B, ..., C], a0, a1 [B, C]."""
    _f32(w); _f32(h)
    B, Cc = w.shape[0], w.shape[-1]
    y = torch.empty_like(w)
    _chk(lib().ore_combine2_fwd(_ptr(w), _ptr(h), _ptr(_f32(a0)), _ptr(_f32(a1)), B, w.numel() // (B * Cc), Cc, _ptr(y), _stream()),
         "ore_combine2_fwd")
    return y


def combine2_bwd(dy: torch.Tensor, a0: torch.Tensor, a1: torch.Tensor, add_bc: Optional[torch.Tensor] = None):
    """(dw, dh) = (dy * a0 + v, dy * a1 + v) with the optional per-(image, channel) constant v."""
    _f32(dy)
    B, Cc = dy.shape[0], dy.shape[-1]
    dw, dh = torch.empty_like(dy), torch.empty_like(dy)
    _chk(lib().ore_combine2_bwd(_ptr(dy), _ptr(_f32(a0)), _ptr(_f32(a1)), _ptr(_f32(add_bc)) if add_bc is not None else None, B,
                                dy.numel() // (B * Cc), Cc, _ptr(dw), _ptr(dh), _stream()), "ore_combine2_bwd")
    return dw, dh


def maxpool3x3s2_bwd(x: torch.Tensor, dy: torch.Tensor) -> torch.Tensor:
    _f32(x); _f32(dy)
    B, H, W, Cc = x.shape
    dx = torch.empty_like(x)
    _chk(lib().ore_maxpool3x3s2_bwd(_ptr(x), _ptr(dy), B, H, W, Cc, _ptr(dx), _stream()), "ore_maxpool3x3s2_bwd")
    return dx


def sumpool2x2(x: torch.Tensor) -> torch.Tensor:
    _f32(x)
    B, H, W, Cc = x.shape
    out = torch.empty(B, (H + 1) // 2, (W + 1) // 2, Cc, device=x.device, dtype=torch.float32)
    _chk(lib().ore_sumpool2x2_fwd(_ptr(x), Cc, B, H, W, Cc, _ptr(out), _stream()), "ore_sumpool2x2_fwd")
    return out
