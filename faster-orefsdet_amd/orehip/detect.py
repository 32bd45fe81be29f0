"""Proposal decoding, COCO evaluation, proposal recall, NMS, ROIAlign and the second stage."""

from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

import orehip          # ROI_BWD_DETERMINISTIC / ROI_BWD_MODE live on the package, where callers rebind them
from ._capi import DetectDesc, OreError, _chk, _f32, _i32s, _ptr, _stream, lib


def _detect_spec(L: int, pre_topk: int):
    cap = L * pre_topk
    capa = (cap + 3) // 4 * 4                                   # one zero-filled allocation carved into the 8 outputs (16-byte aligned)
    spec = (("pre_boxes", torch.float32, 4 * capa, (cap, 4)), ("pre_scores", torch.float32, capa, (cap,)),
            ("pre_loc", torch.int64, capa, (cap,)), ("pre_level", torch.int32, capa, (cap,)), ("keep_idx", torch.int64, capa, (cap,)),
            ("counts", torch.int32, 4, (4,)), ("out_boxes", torch.float32, 4 * capa, (cap, 4)), ("out_scores", torch.float32, capa, (cap,)))
    return spec, sum(n * (8 if dt == torch.int64 else 4) for _, dt, n, _ in spec)


def _detect_desc(heads: Sequence[torch.Tensor], strides, score_thresh, pre_topk, nms_thresh, post_topk, d: "DetectDesc",
                 raw: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None):
    """Allocate one image's outputs + workspace (or carve them out of the caller's `raw` (zeroed) / `ws`) and fill its descriptor."""
    L = len(heads)
    dev = heads[0].device
    cap = L * pre_topk
    spec, raw_bytes = _detect_spec(L, pre_topk)
    if raw is None:
        raw = torch.zeros(raw_bytes, dtype=torch.uint8, device=dev)
    o, off = {}, 0
    for name, dt, n, shape in spec:
        nb = n * (8 if dt == torch.int64 else 4)
        o[name] = raw[off:off + nb].view(dt)[: shape[0] * (4 if len(shape) == 2 else 1)].view(shape)
        off += nb
    wsb = lib().ore_detect_workspace_bytes(L, pre_topk)
    if ws is None:
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    d.n_levels, d.head_ld = L, heads[0].shape[-1]
    for l, h in enumerate(heads):
        _f32(h)
        assert h.dim() == 3 and h.shape[-1] == d.head_ld
        d.head[l], d.H[l], d.W[l], d.stride[l] = _ptr(h), h.shape[0], h.shape[1], strides[l]
    d.score_thresh, d.pre_topk, d.nms_thresh, d.post_topk = score_thresh, pre_topk, nms_thresh, post_topk
    for k in ("pre_boxes", "pre_scores", "pre_loc", "pre_level", "keep_idx", "counts", "out_boxes", "out_scores"):
        setattr(d, k, _ptr(o[k]))
    d.workspace, d.workspace_bytes = _ptr(ws), wsb
    o["_ws"] = ws
    return o


def detect(heads: Sequence[torch.Tensor], strides: Sequence[int], score_thresh: float, pre_topk: int, nms_thresh: float,
           post_topk: int) -> Dict[str, torch.Tensor]:
    """heads[l]: [H,W,ld>=8] fp32: channels 0..3 reg (after Scale+ReLU), 4 = heatmap logit.  No host sync inside."""
    d = DetectDesc()
    o = _detect_desc(heads, strides, score_thresh, pre_topk, nms_thresh, post_topk, d)
    _chk(lib().ore_detect_fwd(C.byref(d), _stream()), "ore_detect_fwd")
    return o


def detect_batch(heads_per_image: Sequence[Sequence[torch.Tensor]], strides: Sequence[int], score_thresh: float, pre_topk: int,
                 nms_thresh: float, post_topk: int) -> List[Dict[str, torch.Tensor]]:
    """`detect` for B independent images (ore_detect_batch_fwd: the greedy scans of up to 16 images share one launch).  Per image the
    outputs of `detect`, bit for bit.  No host sync inside."""
    B = len(heads_per_image)
    ds = (DetectDesc * B)()
    # the outputs and workspaces of all images from two allocations (ONE zero fill instead of B)
    L = len(heads_per_image[0])
    _, raw_bytes = _detect_spec(L, pre_topk)
    raw_bytes = (raw_bytes + 255) // 256 * 256
    wsb = (int(lib().ore_detect_workspace_bytes(L, pre_topk)) + 255) // 256 * 256
    dev = heads_per_image[0][0].device
    raw = torch.zeros(B, raw_bytes, dtype=torch.uint8, device=dev)
    ws = torch.empty(B, wsb, dtype=torch.uint8, device=dev)
    outs = [_detect_desc(heads_per_image[b], strides, score_thresh, pre_topk, nms_thresh, post_topk, ds[b], raw[b], ws[b]) for b in range(B)]
    _chk(lib().ore_detect_batch_fwd(ds, B, _stream()), "ore_detect_batch_fwd")
    return outs


class CocoEvalDesc(C.Structure):
    _fields_ = [("n_images", C.c_int32), ("n_cats", C.c_int32),
                ("det_boxes", C.c_void_p), ("det_scores", C.c_void_p), ("det_image", C.c_void_p), ("det_cat", C.c_void_p), ("n_dets", C.c_int32),
                ("gt_boxes", C.c_void_p), ("gt_area", C.c_void_p), ("gt_crowd", C.c_void_p), ("gt_id", C.c_void_p), ("gt_off", C.c_void_p),
                ("n_gts", C.c_int32),
                ("iou_thrs_host", C.c_void_p), ("n_iou_thrs", C.c_int32), ("rec_thrs_host", C.c_void_p), ("n_rec_thrs", C.c_int32),
                ("area_rngs_host", C.c_void_p), ("n_areas", C.c_int32), ("max_dets_host", C.c_void_p), ("n_max_dets", C.c_int32),
                ("precision", C.c_void_p), ("recall", C.c_void_p), ("scores", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t)]


class CocoEvalImages(C.Structure):
    _fields_ = [("n_units", C.c_void_p), ("unit_pair", C.c_void_p), ("det_index", C.c_void_p), ("dt_matches", C.c_void_p),
                ("dt_ignore", C.c_void_p), ("gt_npig", C.c_void_p), ("capacity", C.c_int64)]


def coco_eval(det_boxes: torch.Tensor, det_scores: torch.Tensor, det_image: torch.Tensor, det_cat: torch.Tensor, gt: Dict[str, torch.Tensor],
              n_images: int, n_cats: int, iou_thrs, rec_thrs, area_rngs, max_dets, per_image: bool = False,
              workspace: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """pycocotools COCOeval (bbox, useCats) on the device: ore_coco_eval.  Detections in results-json order: det_boxes [N, 4] XYXY fp32,
    det_scores [N] fp32, det_image / det_cat [N] int32 indices into the id-sorted images / categories.  gt: device tensors "boxes"
    [G, 4] XYWH fp64, "area" fp64, "crowd" int32, "id" int64, grouped by (category, image) pair with "off" [K * I + 1] int32.
    iou_thrs / rec_thrs / area_rngs / max_dets are host sequences (the exact doubles of COCOeval's Params).  Returns device
    "precision" [T, R, K, A, M], "recall" [T, K, A, M], "scores" [T, R, K, A, M] fp64, and with per_image=True the per-image stage's
    arrays (n_units, unit_pair, det_index, dt_matches, dt_ignore, gt_npig; include/ore_hip.h).  Enqueued on the current stream, no sync."""
    dev = det_boxes.device
    N, G = int(det_scores.numel()), int(gt["area"].numel())
    iou = np.ascontiguousarray(iou_thrs, dtype=np.float64)
    rec = np.ascontiguousarray(rec_thrs, dtype=np.float64)
    area = np.ascontiguousarray(area_rngs, dtype=np.float64).reshape(-1, 2)
    mdet = np.ascontiguousarray(max_dets, dtype=np.int32)
    T, R, A, M = len(iou), len(rec), len(area), len(mdet)
    wsb = lib().ore_coco_eval_workspace_bytes(n_cats, n_images, N, G, T, A, int(mdet[-1]))
    if wsb == 0:
        raise OreError(f"coco_eval: bad sizes (cats {n_cats}, images {n_images}, dets {N}, gts {G}, T {T}, A {A})")
    if workspace is None or workspace.numel() < wsb:
        workspace = torch.empty(wsb, dtype=torch.uint8, device=dev)
    out = {"precision": torch.empty(T, R, n_cats, A, M, dtype=torch.float64, device=dev),
           "recall": torch.empty(T, n_cats, A, M, dtype=torch.float64, device=dev),
           "scores": torch.empty(T, R, n_cats, A, M, dtype=torch.float64, device=dev)}
    det_boxes, det_scores = det_boxes.float().contiguous(), det_scores.float().contiguous()
    det_image, det_cat = det_image.to(torch.int32).contiguous(), det_cat.to(torch.int32).contiguous()
    d = CocoEvalDesc(n_images=n_images, n_cats=n_cats, det_boxes=_ptr(det_boxes) if N else None, det_scores=_ptr(det_scores) if N else None,
                     det_image=_ptr(det_image) if N else None, det_cat=_ptr(det_cat) if N else None, n_dets=N,
                     gt_boxes=_ptr(gt["boxes"]) if G else None, gt_area=_ptr(gt["area"]) if G else None,
                     gt_crowd=_ptr(gt["crowd"]) if G else None, gt_id=_ptr(gt["id"]) if G else None, gt_off=_ptr(gt["off"]), n_gts=G,
                     iou_thrs_host=iou.ctypes.data, n_iou_thrs=T, rec_thrs_host=rec.ctypes.data, n_rec_thrs=R,
                     area_rngs_host=area.ctypes.data, n_areas=A, max_dets_host=mdet.ctypes.data, n_max_dets=M,
                     precision=_ptr(out["precision"]), recall=_ptr(out["recall"]), scores=_ptr(out["scores"]),
                     workspace=_ptr(workspace), workspace_bytes=wsb)
    img = None
    if per_image:
        cap = max(1, min(n_cats * n_images, N + G))
        D = int(mdet[-1])
        pi = {"n_units": torch.zeros(1, dtype=torch.int32, device=dev), "unit_pair": torch.zeros(cap, dtype=torch.int32, device=dev),
              "det_index": torch.zeros(cap, D, dtype=torch.int32, device=dev),
              "dt_matches": torch.zeros(cap, A, T, D, dtype=torch.int64, device=dev),
              "dt_ignore": torch.zeros(cap, A, T, D, dtype=torch.uint8, device=dev), "gt_npig": torch.zeros(cap, A, dtype=torch.int32, device=dev)}
        img = CocoEvalImages(capacity=cap, **{k: _ptr(v) for k, v in pi.items()})
        out.update(pi)
    _chk(lib().ore_coco_eval(C.byref(d), C.byref(img) if img is not None else None, _stream()), "ore_coco_eval")
    return out


class ProposalRecallDesc(C.Structure):
    _fields_ = [("n_entries", C.c_int32), ("n_images", C.c_int32),
                ("prop_boxes", C.c_void_p), ("prop_logits", C.c_void_p), ("n_props", C.c_int32),
                ("entry_off", C.c_void_p), ("entry_image", C.c_void_p),
                ("gt_boxes", C.c_void_p), ("gt_area", C.c_void_p), ("gt_crowd", C.c_void_p), ("gt_off", C.c_void_p), ("n_gts", C.c_int32),
                ("area_rngs_host", C.c_void_p), ("n_areas", C.c_int32), ("limits_host", C.c_void_p), ("n_limits", C.c_int32),
                ("iou_thrs_host", C.c_void_p), ("n_iou_thrs", C.c_int32),
                ("n_slots", C.c_int32), ("n_iou_cells", C.c_int64),
                ("num_pos", C.c_void_p), ("gt_overlaps", C.c_void_p), ("counts", C.c_void_p), ("status", C.c_void_p),
                ("entry_overlaps", C.c_void_p), ("entry_slot_off", C.c_void_p), ("entry_valid", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t)]


def proposal_recall_sizes(entry_counts, entry_image, gt_off_host, limits) -> Tuple[int, int]:
    """(n_slots, n_iou_cells) of one ore_proposal_recall call, from what the host knows: the proposal count and image index of every
    entry and the per-image GT offsets (include/ore_hip.h)."""
    cnt = np.asarray(entry_counts, dtype=np.int64).reshape(-1)
    img = np.asarray(entry_image, dtype=np.int64).reshape(-1)
    per = np.diff(np.asarray(gt_off_host, dtype=np.int64))
    g = per[img] if len(img) else np.zeros(0, np.int64)
    cells = np.minimum(cnt, int(max(limits))) * g
    return int(g.sum()), int(cells[cells > lib().ore_proposal_recall_lds_cells()].sum())


def proposal_recall(prop_boxes: torch.Tensor, prop_logits: torch.Tensor, entry_counts, entry_image, gt: Dict[str, torch.Tensor], gt_off_host,
                    area_rngs, limits, iou_thrs, per_image: bool = False, workspace: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """The reference's proposal recall (_evaluate_box_proposals) on the device for every (limit, area range) pair: ore_proposal_recall.
    prop_boxes [N, 4] XYXY fp32 and prop_logits [N] fp32: the proposals of all prediction entries concatenated; entry_counts /
    entry_image: host sequences, the proposal count of every entry and the index of its image among the id-sorted images.  gt: the
    per-image view (CocoGT.device_images): device "boxes" [G, 4] XYWH fp64, "area" fp64, "crowd" int32, "off" [I + 1] int32;
    gt_off_host: the same offsets on the host.  area_rngs [A][2], limits [L], iou_thrs [T] fp32 are host sequences; chain c = l * A + a.
    Returns device tensors: "num_pos" [L * A] int64; "gt_overlaps" [L * A, S] fp32, row c ascending, its first num_pos[c] values valid;
    "counts" [L * A, T] int64 (overlaps >= threshold); "status" [1] int32 (0: every entry was evaluated); with per_image=True also
    "entry_overlaps" [L * A, S] (entry e's recorded vector of chain c at [c, entry_slot_off[e] : + entry_valid[e, c]]),
    "entry_slot_off" [E + 1] int32, "entry_valid" [E, L * A] int32.  Enqueued on the current stream, no sync."""
    dev = prop_boxes.device
    cnt = np.ascontiguousarray(entry_counts, dtype=np.int64).reshape(-1)
    img = np.ascontiguousarray(entry_image, dtype=np.int32).reshape(-1)
    off_h = np.ascontiguousarray(gt_off_host, dtype=np.int64).reshape(-1)
    E, I, N, G = len(cnt), len(off_h) - 1, int(prop_logits.numel()), int(gt["area"].numel())
    if len(img) != E or int(cnt.sum()) != N or (E and (int(img.min()) < 0 or int(img.max()) >= I)) or int(gt["off"].numel()) != I + 1:
        raise OreError(f"proposal_recall: {E} entries with {int(cnt.sum())} proposals, {N} rows, {len(img)} image indices, {I} images")
    area = np.ascontiguousarray(area_rngs, dtype=np.float64).reshape(-1, 2)
    lim = np.ascontiguousarray(limits, dtype=np.int32)
    thr = np.ascontiguousarray(iou_thrs, dtype=np.float32)
    A, L, T = len(area), len(lim), len(thr)
    S, cells = proposal_recall_sizes(cnt, img, off_h, lim)
    wsb = lib().ore_proposal_recall_workspace_bytes(E, N, S, cells, A, L)
    if wsb == 0:
        raise OreError(f"proposal_recall: bad sizes (entries {E}, proposals {N}, slots {S}, areas {A}, limits {L})")
    if workspace is None or workspace.numel() < wsb:
        workspace = torch.empty(wsb, dtype=torch.uint8, device=dev)
    entry_off = torch.from_numpy(np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)).to(dev)
    entry_img = torch.from_numpy(img).to(dev)
    prop_boxes, prop_logits = prop_boxes.float().contiguous(), prop_logits.float().contiguous()
    out = {"num_pos": torch.empty(L * A, dtype=torch.int64, device=dev), "gt_overlaps": torch.empty(L * A, S, dtype=torch.float32, device=dev),
           "counts": torch.empty(L * A, T, dtype=torch.int64, device=dev), "status": torch.empty(1, dtype=torch.int32, device=dev)}
    if per_image:
        out.update({"entry_overlaps": torch.empty(L * A, S, dtype=torch.float32, device=dev),
                    "entry_slot_off": torch.empty(E + 1, dtype=torch.int32, device=dev),
                    "entry_valid": torch.empty(max(E, 1), L * A, dtype=torch.int32, device=dev)})
    p = lambda t: _ptr(t) if t.numel() else None
    d = ProposalRecallDesc(n_entries=E, n_images=I, prop_boxes=p(prop_boxes), prop_logits=p(prop_logits), n_props=N,
                           entry_off=_ptr(entry_off), entry_image=p(entry_img),
                           gt_boxes=p(gt["boxes"]), gt_area=p(gt["area"]), gt_crowd=p(gt["crowd"]), gt_off=_ptr(gt["off"]), n_gts=G,
                           area_rngs_host=area.ctypes.data, n_areas=A, limits_host=lim.ctypes.data, n_limits=L,
                           iou_thrs_host=thr.ctypes.data, n_iou_thrs=T, n_slots=S, n_iou_cells=cells,
                           num_pos=_ptr(out["num_pos"]), gt_overlaps=p(out["gt_overlaps"]), counts=_ptr(out["counts"]), status=_ptr(out["status"]),
                           entry_overlaps=p(out["entry_overlaps"]) if per_image else None,
                           entry_slot_off=_ptr(out["entry_slot_off"]) if per_image else None,
                           entry_valid=out["entry_valid"].data_ptr() if per_image else None,
                           workspace=_ptr(workspace), workspace_bytes=wsb)
    _chk(lib().ore_proposal_recall(C.byref(d), _stream()), "ore_proposal_recall")
    if per_image:
        out["entry_valid"] = out["entry_valid"][:E]
    return out


def nms(boxes: torch.Tensor, scores: torch.Tensor, thr: float) -> torch.Tensor:
    """torchvision.ops.nms semantics (stable order); returns int64 keep indices (this call syncs to read the count)."""
    n = scores.numel()
    dev = boxes.device
    keep = torch.zeros(max(n, 1), dtype=torch.int64, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    wsb = lib().ore_nms_workspace_bytes(n)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    b = boxes.float().contiguous() if n else torch.zeros(1, 4, device=dev)
    s = scores.float().contiguous() if n else torch.zeros(1, device=dev)
    _chk(lib().ore_nms_fwd(_ptr(b), _ptr(s), n, thr, _ptr(keep), _ptr(cnt), _ptr(ws), wsb, _stream()), "ore_nms_fwd")
    return keep[: int(cnt.item())]


def _roi_levels(maps: Sequence[torch.Tensor], strides: Sequence[int]):
    """The per-level arrays of the ROIAlign entry points: map pointers, ld, channel offset (0), H, W and 1 / stride."""
    L = len(maps)
    return ((C.c_void_p * L)(*[_ptr(_f32(f)) for f in maps]), _i32s(f.shape[-1] for f in maps), _i32s([0] * L),
            _i32s(f.shape[-3] for f in maps), _i32s(f.shape[-2] for f in maps), (C.c_float * L)(*[1.0 / s for s in strides]))


def roi_align(feats: Sequence[torch.Tensor], boxes: torch.Tensor, strides: Sequence[int], pooled: int = 8,
              n_dev: Optional[torch.Tensor] = None, cap: Optional[int] = None, min_level: int = 3) -> torch.Tensor:
    """feats[l]: [1,H,W,C] NHWC (or a channel-slice view described by (tensor, coff, C)); boxes [n,4] -> [cap, pooled*pooled*C]."""
    L = len(feats)
    n = boxes.shape[0]
    cap = cap or max(n, 1)
    Cc = feats[0].shape[-1]
    out = torch.empty(cap, pooled * pooled * Cc, device=boxes.device, dtype=torch.float32)
    ptrs, ld, coff, Hs, Ws, sc = _roi_levels(feats, strides)
    b = boxes.float().contiguous() if n else torch.zeros(1, 4, device=boxes.device)
    _chk(lib().ore_roi_align_fwd(ptrs, ld, coff, Hs, Ws, sc, L, min_level, Cc, pooled, _ptr(b), _ptr(n_dev), n, cap, _ptr(out), _stream()),
         "ore_roi_align_fwd")
    return out


def roi_align_batched(feats: Sequence[torch.Tensor], boxes: torch.Tensor, box_image: torch.Tensor, strides=(8, 16, 32), pooled: int = 8,
                      min_level: int = 3) -> torch.Tensor:
    """feats[l] [B,H,W,C]; box i pools image box_image[i] (int32) -> [n, pooled*pooled*C]."""
    L = len(feats)
    n = boxes.shape[0]
    Cc = feats[0].shape[-1]
    out = torch.empty(max(n, 1), pooled * pooled * Cc, device=boxes.device, dtype=torch.float32)
    ptrs, ld, coff, Hs, Ws, sc = _roi_levels(feats, strides)
    assert box_image.dtype == torch.int32 and box_image.numel() == n
    _chk(lib().ore_roi_align_batched_fwd(ptrs, ld, coff, Hs, Ws, sc, L, min_level, Cc, pooled, _ptr(_f32(boxes)), _ptr(box_image), n,
                                         _ptr(out), _stream()), "ore_roi_align_batched_fwd")
    return out[:n]


def roi_align_bwd(dout: torch.Tensor, feats_like: Sequence[torch.Tensor], boxes: torch.Tensor, strides=(8, 16, 32), min_level: int = 3,
                  pooled: int = 8, dfeats: Optional[Sequence[torch.Tensor]] = None, box_image: Optional[torch.Tensor] = None) -> List[torch.Tensor]:
    """dout [n, pooled*pooled*C]; returns/accumulates into per-level gradient buffers shaped like feats_like ([H,W,ld] NHWC)."""
    L = len(feats_like)
    n = boxes.shape[0]
    tiled = orehip.ROI_BWD_DETERMINISTIC and orehip.ROI_BWD_MODE == "tiled" and pooled <= 16
    given = dfeats is not None
    if dfeats is None:
        # the tiled form writes every cell of every map itself: nothing to zero
        dfeats = [torch.empty_like(f, dtype=torch.float32) if tiled else torch.zeros_like(f) for f in feats_like]
    Cc = dfeats[0].shape[-1]
    assert dout.numel() == n * pooled * pooled * Cc
    if n == 0:
        if tiled and not given:
            for f in dfeats:
                f.zero_()
        return list(dfeats)
    ptrs, ld, coff, Hs, Ws, sc = _roi_levels(dfeats, strides)
    n_img = 1 if dfeats[0].dim() == 3 else dfeats[0].shape[0]
    assert box_image is not None or n_img == 1
    if tiled:
        # one block per (image, level, 16 x 16-cell tile, 32 channels) gathers the ROIs that reach its cells in index order: no atomics, no
        # scratch, bit-reproducible (ore_roi_align_bwd_tiled)
        _chk(lib().ore_roi_align_bwd_tiled(ptrs, ld, coff, Hs, Ws, sc, L, min_level, Cc, pooled, _ptr(_f32(boxes.float().contiguous())),
                                           _ptr(box_image), n, _ptr(_f32(dout)), n_img, int(given), _stream()), "ore_roi_align_bwd_tiled")
        return list(dfeats)
    # Two ROIs of one image may touch the same cell: their sum must not depend on the order the blocks run in -> fixed-point accumulation
    # (ore_roi_align_bwd_det, one zeroed int64 scratch for all levels).  With at most one ROI per image (the support crops: one box each)
    # every cell receives ONE add from the column kernel, fp32 atomics are order-free there and the scratch (8 bytes per map element) is
    # saved.
    if orehip.ROI_BWD_DETERMINISTIC and (n > n_img or box_image is None and n > 1):
        sizes = [n_img * f.shape[-3] * f.shape[-2] * Cc for f in dfeats]
        scratch = torch.zeros(sum(sizes), dtype=torch.int64, device=dout.device)
        offs = [sum(sizes[:i]) for i in range(L)]
        accs = (C.c_void_p * L)(*[_ptr(scratch) + 8 * o for o in offs])
        _chk(lib().ore_roi_align_bwd_det(ptrs, ld, coff, Hs, Ws, sc, L, min_level, Cc, pooled, _ptr(_f32(boxes.float().contiguous())),
                                         _ptr(box_image), n, _ptr(_f32(dout)), accs, n_img, _stream()), "ore_roi_align_bwd_det")
        return list(dfeats)
    _chk(lib().ore_roi_align_bwd(ptrs, ld, coff, Hs, Ws, sc, L, min_level, Cc, pooled, _ptr(_f32(boxes.float().contiguous())),
                                 _ptr(box_image), n, _ptr(_f32(dout)), _stream()), "ore_roi_align_bwd")
    return list(dfeats)


def roi_predict(h: torch.Tensor, cls_w, cls_b, box_w, box_b, boxes: torch.Tensor, reg_weights, image_hw, score_thresh: float,
                nms_thresh: float, topk: int, n_dev: Optional[torch.Tensor] = None, parts: int = 0, bias: Optional[torch.Tensor] = None,
                post: Optional[torch.Tensor] = None, pin: Optional[torch.Tensor] = None, score_sum: Optional[torch.Tensor] = None,
                dead: Optional[torch.Tensor] = None, n_stages: int = 1) -> Dict[str, torch.Tensor]:
    """h [cap, C] fc1 rows, or with parts >= 1 the K-split partial sums [parts, cap, C] (bias [C] or None) that the engine's second
    stage hands over (ore_roi_predict_parts_fwd).  post: device {sx, sy, out_w, out_h} -> detector_postprocess in the same launch,
    returned as "fin_boxes" / "fin_scores" / "fin_count".  pin: device int32 tensor of >= 4 words: word 0 receives the final count,
    words 2..3 hold the 64-bit device address of a record tensor (boxes | scores | int64 classes, see the header) or 0.
    n_stages > 1: the last stage of a cascade (ore_roi_predict_cascade_fwd) with score_sum [cap] fp32 / dead [cap] uint8 of
    roi_cascade_refine; the candidate score is (score_sum + s) * float32(1 / n_stages)."""
    cap, Cc = h.shape[-2:]
    if n_stages > 1 and (score_sum is None or dead is None or score_sum.numel() < cap or dead.numel() < cap or dead.dtype != torch.uint8):
        raise OreError(f"roi_predict: {n_stages} cascade stages need score_sum [cap] fp32 and dead [cap] uint8 of the stages before the last")
    if h.dim() != (3 if parts >= 1 else 2) or (parts >= 1 and h.shape[0] != parts):
        raise OreError(f"roi_predict: h {tuple(h.shape)} with parts={parts}")
    if pin is not None and (pin.dtype != torch.int32 or pin.numel() < 4):
        raise OreError("roi_predict: pin must hold at least 4 int32 words")
    n = boxes.shape[0]
    dev = h.device
    o = {"boxes": torch.zeros(cap, 4, device=dev), "scores": torch.zeros(cap, device=dev),
         "src": torch.zeros(cap, dtype=torch.int64, device=dev), "count": torch.zeros(1, dtype=torch.int32, device=dev)}
    if post is not None:
        o.update({"fin_boxes": torch.zeros(cap, 4, device=dev), "fin_scores": torch.zeros(cap, device=dev),
                  "fin_count": torch.zeros(1, dtype=torch.int32, device=dev)})
    wsb = lib().ore_roi_predict_workspace_bytes(cap)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    rw = (C.c_float * 4)(*reg_weights)
    b = boxes.float().contiguous() if n else torch.zeros(1, 4, device=dev)
    args = (_ptr(_f32(h)), Cc, _ptr(_f32(cls_w)), _ptr(_f32(cls_b)), _ptr(_f32(box_w)), _ptr(_f32(box_b)), _ptr(b),
            _ptr(n_dev), n, cap, rw, image_hw[0], image_hw[1], score_thresh, nms_thresh, topk, _ptr(o["boxes"]),
            _ptr(o["scores"]), _ptr(o["src"]), _ptr(o["count"]), _ptr(_f32(post)) if post is not None else None,
            _ptr(o.get("fin_boxes")), _ptr(o.get("fin_scores")), _ptr(o.get("fin_count")), _ptr(pin),
            _ptr(ws), wsb, _stream(), parts, _ptr(_f32(bias)) if bias is not None else None)
    if n_stages == 1 and score_sum is None and dead is None:
        _chk(lib().ore_roi_predict_parts_fwd(*args), "ore_roi_predict_parts_fwd")
    else:
        _chk(lib().ore_roi_predict_cascade_fwd(*args, _ptr(_f32(score_sum)) if score_sum is not None else None, _ptr(dead), int(n_stages)),
             "ore_roi_predict_cascade_fwd")
    o["_ws"] = ws
    return o


def roi_cascade_refine(h: torch.Tensor, cls_w, cls_b, box_w, box_b, boxes: torch.Tensor, reg_weights, image_hw,
                       n_dev: Optional[torch.Tensor] = None, parts: int = 0, bias: Optional[torch.Tensor] = None,
                       score_sum: Optional[torch.Tensor] = None, dead: Optional[torch.Tensor] = None):
    """One intermediate cascade stage (ore_roi_cascade_refine_fwd): h as roi_predict takes it, boxes [n,4] the stage's proposals.
    score_sum / dead None: the first stage (both are created and written); given: added into / kept sticky.
    Returns (next boxes [n,4], score_sum [cap], dead [cap] uint8)."""
    cap, Cc = h.shape[-2:]
    if h.dim() != (3 if parts >= 1 else 2) or (parts >= 1 and h.shape[0] != parts):
        raise OreError(f"roi_cascade_refine: h {tuple(h.shape)} with parts={parts}")
    if (score_sum is None) != (dead is None):
        raise OreError("roi_cascade_refine: score_sum and dead come together")
    n = boxes.shape[0]
    dev = h.device
    acc = 0 if score_sum is None else 1
    if score_sum is None:
        score_sum = torch.zeros(cap, device=dev)
        dead = torch.zeros(cap, dtype=torch.uint8, device=dev)
    if score_sum.numel() < cap or dead.numel() < cap or dead.dtype != torch.uint8:
        raise OreError("roi_cascade_refine: score_sum [cap] fp32 and dead [cap] uint8")
    nxt = torch.zeros(cap, 4, device=dev)
    rw = (C.c_float * 4)(*reg_weights)
    b = boxes.float().contiguous() if n else torch.zeros(1, 4, device=dev)
    _chk(lib().ore_roi_cascade_refine_fwd(_ptr(_f32(h)), Cc, parts, _ptr(_f32(bias)) if bias is not None else None, _ptr(_f32(cls_w)),
                                          _ptr(_f32(cls_b)), _ptr(_f32(box_w)), _ptr(_f32(box_b)), _ptr(b), _ptr(n_dev), n, cap, rw,
                                          image_hw[0], image_hw[1], _ptr(nxt), _ptr(_f32(score_sum)), _ptr(dead), acc, _stream()),
         "ore_roi_cascade_refine_fwd")
    return nxt[:n] if n_dev is None else nxt, score_sum, dead


def cascade_relabel(boxes: torch.Tensor, deltas: torch.Tensor, valid: torch.Tensor, img_hw: torch.Tensor, gtp: torch.Tensor,
                    gt_n: torch.Tensor, reg_weights, iou_thr: float):
    """The training seam between two cascade stages for B images x R rows in one launch (ore_cascade_relabel_fwd): boxes / deltas [B,R,4]
    of the producing stage, valid [B,R] bool, img_hw [B,2] fp32 (h, w) on the device, gtp [B,G,4] + gt_n [B] int64, reg_weights of the
    producing stage, iou_thr of the consuming one -> (boxes' [B,R,4], labels [B,R] int64 (0 fg / 1 bg), matched gt [B,R,4], valid' [B,R])."""
    B, R, _ = boxes.shape
    G = gtp.shape[1]
    dev = boxes.device
    assert deltas.shape == (B, R, 4) and valid.shape == (B, R) and valid.dtype == torch.bool and img_hw.shape == (B, 2)
    assert gt_n.dtype == torch.int64 and gt_n.numel() == B and gtp.dim() == 3 and gtp.shape[0] == B
    ob = torch.empty(B, R, 4, device=dev, dtype=torch.float32)
    og = torch.empty(B, R, 4, device=dev, dtype=torch.float32)
    ol = torch.empty(B, R, device=dev, dtype=torch.int64)
    ov = torch.empty(B, R, device=dev, dtype=torch.bool)
    rw = (C.c_float * 4)(*[float(v) for v in reg_weights])
    _chk(lib().ore_cascade_relabel_fwd(_ptr(_f32(boxes)), _ptr(_f32(deltas)), _ptr(valid.contiguous()), _ptr(_f32(img_hw)),
                                       _ptr(_f32(gtp)) if G else None, _ptr(gt_n), B, R, G, rw, float(iou_thr), _ptr(ob), _ptr(ov), _ptr(ol),
                                       _ptr(og), _stream()), "ore_cascade_relabel_fwd")
    return ob, ol, og, ov
