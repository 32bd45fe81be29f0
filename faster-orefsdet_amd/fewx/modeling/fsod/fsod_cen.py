"""CenterNet2Detector meta-architecture (ref:fewx/modeling/fsod/fsod_cen.py:38-555) on the MI355X HIP path.

Eval hot path = ONE call into libore_hip.so's engine, replayed as a hipGraph:
stem_1 with fused BGR normalisation -> VoVNet OSA stages -> FPN -> query<->support depthwise correlation ->
conv3 -> CenterNet head -> sigmoid/top-k/decode/NMS.  The support prototypes are loaded ONCE (the reference re-reads
support_feature.pkl on every forward) and the engine is rebuilt only when parameters change."""
import logging
import operator
import os

import numpy as np
import pickle

import torch
import torch.nn.functional as F
from torch import nn

from detectron2.layers import _require_gpu
from detectron2.modeling import META_ARCH_REGISTRY, build_backbone, build_proposal_generator
from detectron2.modeling.postprocessing import detector_postprocess
from detectron2.structures import ImageList

from .fsod_roi_heads import build_roi_heads
from .fsod_rpn import make_proposals

_TENSOR_VERSION = operator.attrgetter("_version")
_MAX_CLASSES = 16                                     # ORE_MAX_CLASSES (include/ore_hip.h)


def resolve_support_classes(support_dict, selection):
    """The support classes an N-way forward answers for, in slot order (CenterNet2Detector.support_classes):
    None -> None (the reference's path: the last class only); "all" -> every class of support_dict in insertion order
    (the reference's `.items()` loops); a list of ids -> those classes in that order.  Every selected class needs p3 / p4 / p5 prototypes
    and rcnn_8 features; an unknown id, a class without rcnn_8, a repeated id or an empty / too long selection raises ValueError."""
    if selection is None:
        return None
    if support_dict is None:
        raise ValueError("support_classes is set but no support prototypes are loaded (init_model / set_support_dict)")
    if isinstance(selection, str):
        if selection != "all":
            raise ValueError(f"support_classes must be None, 'all' or a list of class ids, not {selection!r}")
        ids = list(support_dict.get("p3", {}).keys())
    else:
        ids = list(selection)
    if not ids:
        raise ValueError("support_classes selects no class")
    if len(ids) > _MAX_CLASSES:
        raise ValueError(f"support_classes selects {len(ids)} classes; one N-way pass covers at most {_MAX_CLASSES}")
    if len(set(ids)) != len(ids):
        raise ValueError(f"support_classes repeats a class id: {ids}")
    for c in ids:
        for k in ("p3", "p4", "p5"):
            if c not in support_dict.get(k, {}):
                raise ValueError(f"support class {c!r} has no {k} prototype in the support set (classes: {list(support_dict.get('p3', {}))})")
        if c not in support_dict.get("rcnn_8", {}):
            raise ValueError(f"support class {c!r} has no rcnn_8 support features: N-way inference needs the second stage of every class")
    return ids


class MLP(nn.Module):
    """ref fsod_cen.py:573-582."""

    def __init__(self, in_features, hidden_features, out_features, act_layer=nn.GELU, drop=0.1):
        super().__init__()
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.act = act_layer()
        self.fc2 = nn.Linear(hidden_features, out_features)
        self.drop = nn.Dropout(drop)

    def forward(self, x):
        if x.is_cuda:                                   # the two Linears on the MFMA GEMM kernel (autograd bindings when training)
            from orehip import autograd as A
            h = self.drop(self.act(A.linear(x.contiguous(), self.fc1.weight, self.fc1.bias)))
            return self.drop(A.linear(h.contiguous(), self.fc2.weight, self.fc2.bias))
        return self.drop(self.fc2(self.drop(self.act(self.fc1(x)))))


def _hip_linear(x2d, weight, bias=None):
    """[R,K] @ W[N,K]^T (+bias) as a 1x1 'conv' on the MFMA implicit-GEMM kernel."""
    import orehip
    R, K = x2d.shape
    w = orehip.pack_conv_weight(weight.detach().reshape(weight.shape[0], K, 1, 1))
    y = orehip.conv2d(x2d.contiguous().view(1, 1, R, K), w, weight.shape[0], 1, shift=None if bias is None else bias.detach().contiguous())
    return y.view(R, weight.shape[0])


class SM_Block(nn.Module):
    """Support 'sparse-MLP' block (ref fsod_cen.py:584-630): H-mixing and W-mixing Linear(dim,dim) over (seg, S) groups,
    softmax re-weighting, projection.  The three big Linears run on the MFMA GEMM kernel; eval only this round."""

    def __init__(self, dim, seg_dim=8, qkv_bias=False, proj_drop=0.0):
        super().__init__()
        self.seg_dim = seg_dim
        self.mlp_h = nn.Linear(dim, dim, bias=qkv_bias)
        self.mlp_w = nn.Linear(dim, dim, bias=qkv_bias)
        self.reweighting = MLP(dim, dim // 2, dim * 2)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)

    def forward(self, x):
        _require_gpu(x, "SM_Block")
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            return self._forward_train(x)
        B, H, W, C = x.shape
        S = C // self.seg_dim
        h = x.reshape(B, H, W, self.seg_dim, S).permute(0, 3, 2, 1, 4).reshape(-1, H * S)
        h = _hip_linear(h, self.mlp_h.weight).reshape(B, self.seg_dim, W, H, S).permute(0, 3, 2, 1, 4).reshape(B, H, W, C)
        w = x.reshape(B, H, W, self.seg_dim, S).permute(0, 3, 1, 2, 4).reshape(-1, W * S)
        w = _hip_linear(w, self.mlp_w.weight).reshape(B, self.seg_dim, H, W, S).permute(0, 2, 3, 1, 4).reshape(B, H, W, C)
        a = (h + w).permute(0, 3, 1, 2).flatten(2).mean(2)
        a = self.reweighting(a).reshape(B, C, 2).permute(2, 0, 1).softmax(0).unsqueeze(2).unsqueeze(2)
        y = w * a[0] + h * a[1]
        return _hip_linear(y.reshape(-1, C), self.proj.weight, self.proj.bias).reshape(B, H, W, C)


def _sm_block_train(self, x):
    """Same arithmetic as the eval forward with the Linears going through orehip.autograd (forward, data- and weight-gradient
    kernels), the mixing layouts as granule transposes (SmDualPermuteFn / SmPermuteFn), the pooled mean without the (h + w) tensor and the
    re-weighted sum in one pass (MeanPairFn, Combine2Fn); the [B, C]-sized re-weighting MLP / softmax / dropout stay torch ops (ref fsod_cen.py:584-630)."""
    from orehip import autograd as A
    B, H, W, C = x.shape
    S = C // self.seg_dim
    dims = (B, H, W, self.seg_dim, S)
    xh, xw = A.sm_dual_permute(x, dims)
    h = A.sm_permute(A.linear(xh.reshape(-1, H * S), self.mlp_h.weight, self.mlp_h.bias), dims, "h", True)
    w = A.sm_permute(A.linear(xw.reshape(-1, W * S), self.mlp_w.weight, self.mlp_w.bias), dims, "w", True)
    a = self.reweighting(A.mean_pair(h, w)).reshape(B, C, 2).permute(2, 0, 1).softmax(0)
    y = A.combine2(w, h, a[0], a[1])
    return self.proj_drop(A.linear(y.reshape(-1, C), self.proj.weight, self.proj.bias).reshape(B, H, W, C))


SM_Block._forward_train = _sm_block_train


@META_ARCH_REGISTRY.register()
class CenterNet2Detector(nn.Module):
    def __init__(self, cfg, pos_encoding=True):
        super().__init__()
        self.backbone = build_backbone(cfg)
        self.proposal_generator = build_proposal_generator(cfg, self.backbone.output_shape())
        self.roi_heads = build_roi_heads(cfg, self.backbone.output_shape())
        self.vis_period = cfg.VIS_PERIOD
        self.input_format = cfg.INPUT.FORMAT
        assert len(cfg.MODEL.PIXEL_MEAN) == len(cfg.MODEL.PIXEL_STD)
        self.register_buffer("pixel_mean", torch.Tensor(cfg.MODEL.PIXEL_MEAN).view(-1, 1, 1))
        self.register_buffer("pixel_std", torch.Tensor(cfg.MODEL.PIXEL_STD).view(-1, 1, 1))
        self.in_features = cfg.MODEL.ROI_HEADS.IN_FEATURES
        self.support_way = cfg.INPUT.FS.SUPPORT_WAY
        self.support_shot = cfg.INPUT.FS.SUPPORT_SHOT
        self.logger = logging.getLogger(__name__)
        C = cfg.MODEL.FPN.OUT_CHANNELS
        assert C == 128, "CenterNet2Detector is hard-wired to 128 FPN channels in the reference (fsod_cen.py:69-78)"
        self.vip_p3, self.vip_p4, self.vip_p5 = SM_Block(C, 32), SM_Block(C, 16), SM_Block(C, 8)
        self.conv1 = nn.Conv2d(C, C // 2, 1)   # unused by the reference forward; kept for checkpoints
        self.conv2 = nn.Conv2d(C, C // 2, 1)
        self.conv3 = nn.Conv2d(2 * C, C, 1)
        self._cfg_engine = dict(
            body=cfg.MODEL.VOVNET.CONV_BODY, fpn_ch=C, strides=tuple(cfg.MODEL.CENTERNET.FPN_STRIDES),
            pixel_mean=tuple(cfg.MODEL.PIXEL_MEAN), pixel_std=tuple(cfg.MODEL.PIXEL_STD),
            score_thresh=cfg.MODEL.CENTERNET.INFERENCE_TH, pre_topk=cfg.MODEL.CENTERNET.PRE_NMS_TOPK_TEST,
            nms_thresh=cfg.MODEL.CENTERNET.NMS_TH_TEST, post_topk=cfg.MODEL.CENTERNET.POST_NMS_TOPK_TEST)
        self.support_dict = None
        self._enrolled_shots = {}          # class id -> the crops and support boxes enrol() installed it from (enrol(replace=False))
        # "fp32" (the reference's precision) or "bf16": operand precision of the MFMA convs of the EVAL engines this detector
        # builds (orehip.set_conv_precision / include/ore_hip.h ORE_CONV_BF16 -- BASELINE configs[4]); set it before the first forward
        self.conv_operands = "fp32"
        # N-way inference (include/ore_hip.h, ore_engine_set_classes): None = the reference's path (only the last support class is
        # detected, pred_classes all 0); "all" = every class of support_dict; a list of class ids = those classes in that order.  One
        # pass then detects every selected class (pred_classes = class ids).  Not a config key: the config tree is the reference's.
        self.support_classes = None
        # True: the result dict of model([request]) / inference() also carries "proposals", the first-stage proposals of that pass
        # (post-NMS top-k) at the requested output size, as detectron2's ProposalNetwork returns them -- what COCOEvaluator scores with
        # proposal recall ("box_proposals").  "instances" is unchanged.  Not with support_classes (proposals are per class there).
        self.output_proposals = False
        self._engine = None
        self._engine_key = None
        self.max_hw = (int(cfg.INPUT.MAX_SIZE_TEST), int(cfg.INPUT.MAX_SIZE_TEST))
        self._test_size = (int(cfg.INPUT.MIN_SIZE_TEST), int(cfg.INPUT.MAX_SIZE_TEST))     # ResizeShortestEdge of "image_raw" requests

    @property
    def device(self):
        return self.pixel_mean.device

    # ---- support prototypes ------------------------------------------------------------------------------------
    def set_support_dict(self, support_dict):
        """{'p3': {cls: [1,C,32,32]}, 'p4': ..., 'p5': ..., 'rcnn_8': ..., 'rcnn_4': ...} (the support_feature.pkl layout)."""
        self.support_dict = {k: {c: f.to(self.device) for c, f in v.items()} for k, v in support_dict.items()}
        self._engine_key = None
        # shots kept by enrol() go with the prototypes they gave: a class that was replaced or dropped here loses them
        p3 = self.support_dict.get("p3", {})
        self._enrolled_shots = {c: e for c, e in self._enrolled_shots.items() if p3.get(c) is e["ref"]}

    def init_model(self, support_file="./support_dir/support_feature.pkl", support_df=None, read_image=None,
                   support_df_path="./datasets/coco/10_shot_support_df.pkl", image_root="./datasets/coco"):
        """ref fsod_cen.py:313-415, minus its two defects: the pickle is read once (not per forward) and tensors go to
        self.device (not a hard-coded .cuda()).  With no support_feature.pkl the reference walks the support dataframe (per class:
        the first SUPPORT_SHOT rows, image + support_box), computes the features, writes the pickle and exits; here the walk
        (`build_support_from_dataframe`) installs the features and writes the same pickle -- and carries on.  `support_df` /
        `read_image` are injectable because the ore dataset is not shipped; left unset they are the reference's paths."""
        if self.support_dict is not None:
            return
        if os.path.exists(support_file):
            with open(support_file, "rb") as f:
                self.set_support_dict(pickle.load(f, encoding="latin1"))
            return
        if support_df is None:
            if not os.path.exists(support_df_path):
                raise FileNotFoundError(f"neither {support_file} nor {support_df_path} found: generating support features needs the "
                                        "few-shot support set (SURVEY 8f row 3): pass support_df / read_image, call "
                                        "compute_support_dict(images, boxes) + save_support_file(), or set_support_dict()")
            import pandas as pd
            support_df = pd.read_pickle(support_df_path)
        self.build_support_from_dataframe(support_df, read_image=read_image, image_root=image_root)
        self.save_support_file(support_file)

    def build_support_from_dataframe(self, support_df, read_image=None, image_root="./datasets/coco"):
        """The dataframe walk of the reference's init_model (ref fsod_cen.py:331-346): for every category the first SUPPORT_SHOT
        rows (reset_index order) give the support crops and their boxes; the compute is compute_support_dict (HIP kernels)."""
        if read_image is None:
            from fewx.data.dataset_mapper import _pil_read_image as read_image
        for cls in support_df["category_id"].unique():
            rows = support_df.loc[support_df["category_id"] == cls, :].reset_index()
            imgs, boxes = [], []
            for index, r in rows.iterrows():
                if index >= self.support_shot:
                    break
                data = read_image(os.path.join(image_root, r["file_path"]), format="BGR")
                imgs.append(torch.as_tensor(np.ascontiguousarray(data.transpose(2, 0, 1))))
                boxes.append(torch.as_tensor(r["support_box"], dtype=torch.float32))
            self.compute_support_dict(imgs, torch.stack(boxes), cls_id=cls, merge=True)
        return self.support_dict

    @torch.no_grad()
    def compute_support_dict(self, support_images, support_boxes, cls_id=0, merge=True):
        """The compute half of the reference's init_model (ref fsod_cen.py:345-392) for one class, on the HIP kernels:
        support crops -> backbone/FPN -> rcnn_8 / rcnn_4 = ROIAlign (8x8, 4x4) of every crop's own box; p3..p5 prototypes =
        avg-pool to 32/16/8 -> SM_Block -> permute(0,3,2,1) (H<->W swap preserved) -> mean over the shots.
        support_images: list of [3,h,w] (or one [N,3,h,w]) uint8/float BGR; support_boxes [N,4].  Returns the dict in the layout of
        support_feature.pkl (CPU tensors) and, with merge=True, installs it (set_support_dict)."""
        import torch.nn.functional as F
        import orehip
        from detectron2.layers import nhwc_view
        dev = self.device
        imgs = list(support_images) if not torch.is_tensor(support_images) else [x for x in support_images]
        div = self.backbone.size_divisibility
        H = (max(int(x.shape[-2]) for x in imgs) + div - 1) // div * div
        W = (max(int(x.shape[-1]) for x in imgs) + div - 1) // div * div
        mean, std = self.pixel_mean.view(-1, 1, 1), self.pixel_std.view(-1, 1, 1)
        batch = torch.zeros(len(imgs), 3, H, W, device=dev)
        for i, x in enumerate(imgs):                                            # ImageList.from_tensors: normalise, zero-pad bottom/right
            x = (x.to(dev).float() - mean) / std
            batch[i, :, : x.shape[-2], : x.shape[-1]] = x
        boxes = torch.as_tensor(support_boxes, dtype=torch.float32, device=dev).reshape(-1, 4).contiguous()
        assert boxes.shape[0] == len(imgs)
        feats = self.backbone(batch)
        levels = [nhwc_view(feats[f]) for f in self.in_features]
        strides = self._cfg_engine["strides"]
        bidx = torch.arange(len(imgs), dtype=torch.int32, device=dev)
        C = levels[0].shape[-1]
        out = {}
        for key, P in (("rcnn_8", self.roi_heads.pooler_resolution), ("rcnn_4", self.roi_heads.pooler_resolution2)):
            r = orehip.roi_align_batched(levels, boxes, bidx, strides, P)        # [N, P*P*C] ordered [pos][c]
            out[key] = {cls_id: r.reshape(len(imgs), P, P, C).permute(0, 3, 1, 2).contiguous().cpu()}
        for i, f in enumerate(self.in_features):
            size = (32, 16, 8)[i]
            sf = feats[f]
            if sf.shape[-2:] != (size, size):
                sf = F.adaptive_avg_pool2d(sf, (size, size))
            v = getattr(self, f"vip_p{3 + i}")(nhwc_view(sf)).permute(0, 3, 2, 1)
            out[f"p{3 + i}"] = {cls_id: v.mean(0, True).contiguous().cpu()}
        if merge:
            cur = {k: dict(v) for k, v in (self.support_dict or {}).items()}
            for k, v in out.items():
                cur.setdefault(k, {}).update(v)
            self.set_support_dict(cur)
        return out

    # ---- enrolment from annotated frames -----------------------------------------------------------------------
    @torch.no_grad()
    def enrol(self, frames, boxes, cls_id, frame_index=None, replace=True):
        """Installs support class `cls_id` from annotated frames: orehip.support_crops (frames: one [h, w, 3] uint8 image in the model's
        channel order or a list of them, boxes [K, 4] XYXY absolute, frame_index [K]: "support crop v1", include/ore_hip.h) ->
        compute_support_dict(crops, support boxes, cls_id, merge=True).  replace=False adds the K shots to the ones this class was
        enrolled with, and the class then holds exactly what one call with all its shots gives: rcnn_8 / rcnn_4 one row per shot in
        enrolment order, p3..p5 the mean over all shots.  The feature kernels a pass takes depend on its batch size, so rows computed
        two at a time and five at a time differ in the last bit; the shots' crops and boxes (uint8, on the device) are therefore what
        is kept per enrolled class (until set_support_dict replaces or drops it), and the features are computed over all of them in
        one pass: an addition costs a pass over all the class's shots.  A class installed any other way has
        no kept shots, and adding to it is a ValueError.  The cached engines are dropped as by set_support_dict, so
        support_classes = "all" sees the class at the next forward.
        Returns the crops and support boxes of this call's K shots: ([K, 3, 240, 240] uint8 on the device, [K, 4] float32 on the host)."""
        import orehip
        crops, sboxes = orehip.support_crops(frames, boxes, frame_index, device=self.device)
        all_crops, all_boxes = crops, sboxes
        if not replace and self.support_dict is not None and cls_id in self.support_dict.get("p3", {}):
            old = self._enrolled_shots.get(cls_id)
            if old is None:
                raise ValueError(f"support class {cls_id!r} was not installed by enrol(): its shots are not known, so none can be added "
                                 "to it (enrol it with replace=True)")
            all_crops, all_boxes = torch.cat([old["crops"], crops]), torch.cat([old["boxes"], sboxes])
        self.compute_support_dict(all_crops, all_boxes, cls_id=cls_id, merge=True)
        self._enrolled_shots[cls_id] = {"crops": all_crops, "boxes": all_boxes, "ref": self.support_dict["p3"][cls_id]}
        return crops, sboxes

    def forget(self, cls_id):
        """Removes support class `cls_id` from every level of support_dict (KeyError for an unknown id) and drops the cached engines as
        set_support_dict does; with the last class gone, support_dict is None again."""
        if self.support_dict is None or not any(cls_id in v for v in self.support_dict.values()):
            raise KeyError(cls_id)
        cur = {k: {c: f for c, f in v.items() if c != cls_id} for k, v in self.support_dict.items()}
        if not cur.get("p3"):
            self.support_dict = None
            self._engine_key = None
            self._enrolled_shots = {}
        else:
            self.set_support_dict(cur)

    def save_support_file(self, support_file="./support_dir/support_feature.pkl"):
        """Writes self.support_dict in the reference's pickle layout (CPU tensors keyed by level then class id)."""
        os.makedirs(os.path.dirname(support_file) or ".", exist_ok=True)
        with open(support_file, "wb") as f:
            pickle.dump({k: {c: t.detach().cpu() for c, t in v.items()} for k, v in self.support_dict.items()}, f)

    # ---- engine -------------------------------------------------------------------------------------------------
    def _state_key(self):
        """Changes whenever any parameter or buffer is written through torch (optimizer steps -- FlatSGD bumps the version counters
        for its raw-pointer kernel --, load_state_dict, in-place edits).  Version counters only grow, so their sum is a valid key
        for a fixed set of tensor objects; the list is collected once and dropped whenever tensors may have been REPLACED
        (`_apply`: .to() / .float() / .cuda(); `load_state_dict(assign=True)`), together with an epoch that enters the key."""
        ts = self.__dict__.get("_key_tensors")
        if ts is None:
            ts = self.__dict__["_key_tensors"] = list(self.parameters()) + list(self.buffers())
        return (self.__dict__.get("_key_epoch", 0), sum(map(_TENSOR_VERSION, ts)))      # (a C-level loop: ~200 tensors per forward)

    def _invalidate_state_key(self):
        self.__dict__.pop("_key_tensors", None)
        self.__dict__["_key_epoch"] = self.__dict__.get("_key_epoch", 0) + 1

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self._invalidate_state_key()
        return out

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        self._invalidate_state_key()
        return out

    def make_engine(self, max_batch: int = 1, classes=None, max_hw=None):
        """A fresh engine (own buffers, own hipGraph) for the current parameters and support set.  `engine()` caches one; a server
        that keeps several images in flight on separate streams makes one per stream (bench.py --inflight), or folds concurrent
        requests into one pass with max_batch > 1 (Engine.eval_forward_batch).  classes = a resolved support_classes selection: the
        engine also gets one class slot per selected class (Engine.set_classes / detect_classes), max_batch >= len(classes).
        max_hw = (max_h, max_w): the largest input the engine's buffers are sized for instead of cfg.INPUT.MAX_SIZE_TEST squared (the
        test-time-augmentation wrapper's variants exceed it)."""
        max_hw = self.max_hw if max_hw is None else (int(max_hw[0]), int(max_hw[1]))
        if classes:
            max_batch = max(max_batch, len(classes))
        import orehip
        from detectron2.modeling.backbone.vovnet import _STAGE_SPECS
        c = self._cfg_engine
        spec = _STAGE_SPECS[c["body"]]
        blocks = tuple(spec["block_per_stage"])
        if any(b > 1 for b in blocks) and self.conv_operands == "bf16s":
            raise ValueError(f"MODEL.VOVNET.CONV_BODY {c['body']} has identity blocks {blocks}: the engine has no bf16 storage form "
                             "of them (conv_operands 'bf16s')")
        dev = self.device
        assert dev.type == "cuda", "CenterNet2Detector inference runs on the MI355X only"
        prev = orehip.set_conv_precision(self.conv_operands)      # the engine keeps the mode in force at its creation
        try:
            e = orehip.Engine(stem=spec["stem"], conv=spec["stage_conv_ch"], out=spec["stage_out_ch"], layers=spec["layer_per_block"],
                              fpn_ch=c["fpn_ch"], strides=c["strides"], pixel_mean=c["pixel_mean"], pixel_std=c["pixel_std"],
                              score_thresh=c["score_thresh"], pre_topk=c["pre_topk"], nms_thresh=c["nms_thresh"],
                              post_topk=c["post_topk"], max_batch=max_batch, max_h=max_hw[0], max_w=max_hw[1],
                              device=dev.index or 0, depthwise=bool(spec.get("dw", False)), blocks=blocks)
        finally:
            orehip.set_conv_precision(prev)
        e.load_state_dict(self.state_dict())
        assert self.support_dict is not None, "support prototypes not set (init_model / set_support_dict)"
        cls_id = list(self.support_dict["p3"].keys())[-1]   # the reference keeps only the last class
        e.set_support({k: self.support_dict[k][cls_id] for k in ("p3", "p4", "p5")})
        e.finalize()
        rh = self.roi_heads
        if "rcnn_8" in self.support_dict and hasattr(rh, "bbox_reg_weights"):
            stages = getattr(rh, "bbox_reg_weights_per_stage", (rh.bbox_reg_weights,))
            if len(stages) > 1:                       # the cascade: len(ROI_BOX_CASCADE_HEAD.IOUS) stages inside the engine's graph
                e.set_roi_cascade(self.state_dict(), self.support_dict["rcnn_8"][cls_id], stages, rh.test_score_thresh,
                                  rh.test_nms_thresh, rh.test_topk)
            else:
                e.set_roi_head(self.state_dict(), self.support_dict["rcnn_8"][cls_id], rh.bbox_reg_weights, rh.test_score_thresh,
                               rh.test_nms_thresh, rh.test_topk)
        if classes:
            sd = self.state_dict()
            e.set_classes(classes)
            for k, c in enumerate(classes):
                e.set_support({lv: self.support_dict[lv][c] for lv in ("p3", "p4", "p5")}, slot=k)
                e.set_roi_support(sd, self.support_dict["rcnn_8"][c], slot=k)
        return e

    def _support_selection(self):
        sel = resolve_support_classes(self.support_dict, self.support_classes) if self.support_classes is not None else None
        return tuple(sel) if sel is not None else None

    def _engine_key_now(self):
        return (self._state_key(), str(self.device), self.conv_operands, self._support_selection())

    def engine(self):
        key = self._engine_key_now()
        if self._engine is None or self._engine_key != key:
            if self._engine is not None:
                self._engine.close()
            self._engine, self._engine_key = self.make_engine(classes=key[3]), key
        return self._engine

    # ---- forward ------------------------------------------------------------------------------------------------
    def forward(self, batched_inputs):
        if not self.training:
            self.init_model()
            return self.inference(batched_inputs)
        from .train_forward import train_forward
        for x in batched_inputs:                                  # gt_classes forced to 0 (ref fsod_cen.py:158-159)
            if "instances" in x and x["instances"].has("gt_classes"):
                x["instances"].gt_classes = torch.zeros_like(x["instances"].gt_classes)
        return train_forward(self, batched_inputs)

    @staticmethod
    def gradless_parameter_prefixes():
        """Parameters of the reference's dead branches: they exist for checkpoint compatibility, never receive
        a gradient, and therefore stay out of the gradient bucket / optimizer like `grad is None` parameters do in torch."""
        return ("conv1.", "conv2.", "roi_heads.fc2.", "roi_heads.fc3.")

    # ---- raw images ---------------------------------------------------------------------------------------------
    def _upload_raw(self, raw):
        """The upload half of `_resolve_raw`: an [h, w, 3] uint8 image (numpy array, CPU tensor or device tensor) as a contiguous device
        tensor; host memory goes through the pinned staging buffer this model owns, asynchronously on the current stream."""
        dev = self.device
        assert dev.type == "cuda", "CenterNet2Detector inference runs on the MI355X only"
        if isinstance(raw, np.ndarray):
            raw = torch.from_numpy(np.ascontiguousarray(raw))
        if raw.dim() != 3 or raw.shape[2] != 3 or raw.dtype != torch.uint8:
            raise ValueError(f"image_raw must be [h, w, 3] uint8, got {tuple(raw.shape)} {raw.dtype}")
        h, w = int(raw.shape[0]), int(raw.shape[1])
        if raw.is_cuda:
            raw = raw.to(dev).contiguous()
        else:
            n = h * w * 3
            stage = self.__dict__.get("_raw_stage")
            if stage is not None:
                stage[1].synchronize()                            # the copy out of the buffer issued by the previous request
            if stage is None or stage[0].numel() < n:
                stage = self.__dict__["_raw_stage"] = (torch.empty(max(n, 1 << 20), dtype=torch.uint8, pin_memory=True), torch.cuda.Event())
            stage[0][:n].view(h, w, 3).copy_(raw)
            raw = torch.empty(h, w, 3, dtype=torch.uint8, device=dev)
            raw.copy_(stage[0][:n].view(h, w, 3), non_blocking=True)
            stage[1].record()
        return raw

    def _resolve_raw(self, inp):
        """A request that carries "image_raw" -- the unresized [h, w, 3] uint8 image in the model's channel order, or the other one with
        "swap_rb": numpy array, CPU tensor or device tensor -- instead of "image": the image goes to the device (host memory through a
        pinned staging buffer this model owns, asynchronously on the current stream), is resized there to cfg.INPUT.MIN_SIZE_TEST /
        MAX_SIZE_TEST (orehip.resize_bilinear_u8: the bytes of the CPU mapper's Pillow resize) and the request comes back in its
        "image" form, "height" / "width" defaulting to the raw size.  Everything behind treats it as if it had come in that way."""
        import orehip
        if "image" in inp:
            raise ValueError('a request carries either "image" or "image_raw", not both')
        raw = self._upload_raw(inp["image_raw"])
        h, w = int(raw.shape[0]), int(raw.shape[1])
        nh, nw = orehip.resize_shortest_edge_shape(h, w, self._test_size[0], self._test_size[1])
        out = {k: v for k, v in inp.items() if k not in ("image_raw", "swap_rb")}
        out["image"] = orehip.resize_bilinear_u8(raw, nh, nw, swap_rb=bool(inp.get("swap_rb", False)))
        out.setdefault("height", h)
        out.setdefault("width", w)
        return out

    @torch.no_grad()
    def inference_proposals(self, batched_inputs, use_graph=True):
        """The built hot path: image -> proposals (Instances with proposal_boxes / objectness_logits / scores / pred_classes)."""
        assert not self.training
        assert len(batched_inputs) == 1, "only 1 query image in test (ref fsod_cen.py:438-439)"
        img = batched_inputs[0]["image"].to(self.device)
        if img.dtype != torch.uint8:
            img = img.float()
        img = img.contiguous()
        e = self.engine()
        e.eval_forward(img, use_graph=use_graph)
        boxes, scores, _ = e.proposals()
        return [make_proposals((img.shape[-2], img.shape[-1]), boxes.clone(), scores.clone())]

    def _proposals_of_last_pass(self, e, inp, img_hw):
        """The first-stage proposals engine `e` holds from its last pass, cloned, through detector_postprocess to the request's output
        size (scale, clip, drop empty): Instances with proposal_boxes / objectness_logits.  One more host wait: the proposal count."""
        from detectron2.structures import Boxes, Instances
        boxes, scores, _ = e.proposals()
        p = Instances((int(img_hw[0]), int(img_hw[1])))
        p.proposal_boxes = Boxes(boxes.clone())
        p.objectness_logits = scores.clone()
        return detector_postprocess(p, inp.get("height", img_hw[0]), inp.get("width", img_hw[1]))

    @property
    def output_proposals(self):
        return "inference" in self.__dict__

    @output_proposals.setter
    def output_proposals(self, on):
        # the switch replaces this object's `inference`; off, the class's method -- and its fast path -- is what runs, untouched
        if on:
            self.__dict__["inference"] = self._inference_with_proposals
        else:
            self.__dict__.pop("inference", None)

    @torch.no_grad()
    def _inference_with_proposals(self, batched_inputs, detected_instances=None, do_postprocess=True):
        """`inference` with output_proposals on: the checked path, then the proposals of the same engine pass beside "instances"
        (with do_postprocess only: without it the result is the bare Instances list, as in `inference`)."""
        assert not self.training
        self.init_model()
        assert len(batched_inputs) == 1, "only 1 query image in test (ref fsod_cen.py:438-439)"
        inp = batched_inputs[0]
        if self.support_classes is not None:
            raise ValueError("output_proposals does not combine with support_classes: an N-way pass has one proposal set per class")
        if "image_raw" in inp:
            inp = self._resolve_raw(inp)
        out = self._inference_checked(inp, inp["image"], do_postprocess)
        if do_postprocess:
            out[0]["proposals"] = self._proposals_of_last_pass(self._engine, inp, inp["image"].shape[-2:])
        return out

    @torch.no_grad()
    def inference(self, batched_inputs, detected_instances=None, do_postprocess=True):
        assert not self.training
        self.init_model()
        assert len(batched_inputs) == 1, "only 1 query image in test (ref fsod_cen.py:438-439)"
        inp = batched_inputs[0]
        if "image_raw" in inp:
            inp = self._resolve_raw(inp)
        img = inp["image"]
        e = self._engine
        if do_postprocess and e is not None and self._engine_key is not None and getattr(e, "has_roi", False):
            # the whole call -- both stages AND detector_postprocess (fsod_cen.py:557-571) -- is one hipGraph replay behind one C-ABI
            # call; the image may still be on the host (the engine copies it in).  The only host sync is the detection count.
            # The cached engine is launched FIRST and validated (parameter version counters, ~12 us of host work for 174 tensors) while
            # the device runs the pass; an engine found stale -- weights edited since it was built -- has its result dropped and the
            # pass is repeated on a fresh one below.  An engine owns copies of the weights, so the dropped pass touched nothing else.
            from detectron2.structures import Boxes, Instances
            if img.dtype != torch.uint8 and img.dtype != torch.float32:
                img = img.float()
            img = img.contiguous()
            H, W = img.shape[-2:]
            oh, ow = int(inp.get("height", H)), int(inp.get("width", W))
            import orehip
            try:
                # a fresh tensor, filled behind the graph (N-way engines: every selected class in the same pass)
                rec = e.detect_classes_begin(img, oh, ow) if getattr(e, "class_ids", None) else e.detect_begin(img, oh, ow)
            except orehip.OreError:
                rec = None                                        # e.g. the cached engine belongs to another device / size: the checked path below decides
            if rec is None:
                return self._inference_checked(inp, img, do_postprocess)
            try:
                fresh = self._engine_key == self._engine_key_now()
                res = Instances((oh, ow))                         # the result objects are made while the device works, too
                bx = Boxes.__new__(Boxes)
                out = [{"instances": res}]
            except BaseException:
                e.detect_end(rec)                                 # never leave a pass pending that writes into a tensor about to be freed
                raise
            boxes, scores, classes = e.detect_end(rec)
            if not fresh:
                e = self.engine()                                 # rebuilds
                boxes, scores, classes = e.detect_classes(img, oh, ow) if getattr(e, "class_ids", None) else e.detect(img, oh, ow)
            # three views of one record cut at the same count by detect_end: [k, 4] fp32, [k] fp32, [k] int64 -- what Boxes() and
            # Instances.set() would check again, per image, on the protocol's critical path
            bx.tensor = boxes
            res._fields = {"pred_boxes": bx, "scores": scores, "pred_classes": classes}
            return out
        return self._inference_checked(inp, img, do_postprocess)

    def _inference_checked(self, inp, img, do_postprocess):
        """The eval call with the engine validated BEFORE it is used (first call, stale engine, other entry conditions)."""
        if "image_raw" in inp:
            inp = self._resolve_raw(inp)
            img = inp["image"]
        batched_inputs = [inp]
        e = self.engine()
        if getattr(e, "class_ids", None):
            # N-way: both stages of every selected class, the merge and detector_postprocess in one replay; without do_postprocess the
            # output size is the input size (scale 1: clip to the image, drop empty boxes)
            from detectron2.structures import Boxes, Instances
            if img.dtype != torch.uint8 and img.dtype != torch.float32:
                img = img.float()
            img = img.contiguous()
            H, W = img.shape[-2:]
            oh, ow = (int(inp.get("height", H)), int(inp.get("width", W))) if do_postprocess else (int(H), int(W))
            boxes, scores, classes = e.detect_classes(img, oh, ow)
            res = Instances((oh, ow))
            res.pred_boxes = Boxes(boxes)
            res.scores = scores
            res.pred_classes = classes
            return [{"instances": res}] if do_postprocess else [res]
        if do_postprocess and getattr(e, "has_roi", False):
            from detectron2.structures import Boxes, Instances
            if img.dtype != torch.uint8 and img.dtype != torch.float32:
                img = img.float()
            img = img.contiguous()
            H, W = img.shape[-2:]
            oh, ow = int(inp.get("height", H)), int(inp.get("width", W))
            boxes, scores, classes = e.detect(img, oh, ow)        # fresh tensors, filled behind the graph
            res = Instances((oh, ow))
            res.pred_boxes = Boxes(boxes)
            res.scores = scores
            res.pred_classes = classes
            return [{"instances": res}]
        img = img.to(self.device)
        img = (img if img.dtype == torch.uint8 else img.float()).contiguous()
        H, W = img.shape[-2:]
        images = ImageList(torch.empty(0), [(H, W)])
        if getattr(e, "has_roi", False):
            # both stages in ONE hipGraph replay; the only host sync is reading the detection count
            from detectron2.structures import Boxes, Instances
            e.eval_forward(img, use_graph=True)
            boxes, scores, _ = e.detections()
            res = Instances((H, W))
            res.pred_boxes = Boxes(boxes.clone())
            res.scores = scores.clone()
            res.pred_classes = torch.zeros(len(scores), dtype=torch.int64, device=scores.device)
            results = [res]
        else:
            proposals = self.inference_proposals(batched_inputs)
            Hp, Wp = (H + 31) // 32 * 32, (W + 31) // 32 * 32
            features = {f"p{l}": e.buffer(f"p{l}", (1, Hp >> l, Wp >> l)) for l in (3, 4, 5)}
            cls_id = list(self.support_dict["p3"].keys())[-1]
            support = [self.support_dict["rcnn_8"][cls_id], self.support_dict["rcnn_4"][cls_id]]
            results, _ = self.roi_heads(images, features, support, proposals, None)
        if do_postprocess:
            return CenterNet2Detector._postprocess(results, batched_inputs, images.image_sizes)
        return results

    @torch.no_grad()
    def inference_many(self, requests, do_postprocess=True, max_fold: int = 8):
        """Serving entry point beside the reference's one-image `inference`: `requests` is a list of single-image inputs (the dicts
        the reference passes one at a time).  Requests of equal image size and dtype are folded, up to `max_fold` per engine pass
        (Engine.eval_forward_batch: dense stages batched, detection tail and second stage per image); results come back in request
        order and equal the one-at-a-time results (tests/test_hip_parity.py).  With support_classes set (N-way inference) the requests
        are answered one image at a time, each by the one-pass N-way call of `inference`: a pass holds one query image and its classes.
        With output_proposals on they are answered one image at a time as well."""
        from detectron2.structures import Boxes, Instances
        assert not self.training
        self.init_model()
        if self.support_classes is not None or self.output_proposals:
            return [self.inference([r], do_postprocess=do_postprocess)[0] for r in requests]
        requests = [self._resolve_raw(r) if "image_raw" in r else r for r in requests]
        key = (self._state_key(), str(self.device), self.conv_operands, max_fold)
        if getattr(self, "_fold_engine_key", None) != key:
            if getattr(self, "_fold_engine", None) is not None:
                self._fold_engine.close()
            self._fold_engine, self._fold_engine_key = self.make_engine(max_batch=max_fold), key
        e = self._fold_engine
        assert getattr(e, "has_roi", False), "inference_many needs the second stage inside the engine (support set with rcnn_8 features)"
        imgs = []
        for r in requests:
            img = r["image"].to(self.device)
            imgs.append((img if img.dtype == torch.uint8 else img.float()).contiguous())
        groups = {}
        for i, im in enumerate(imgs):
            groups.setdefault((tuple(im.shape), im.dtype), []).append(i)
        results = [None] * len(requests)
        for idxs in groups.values():
            for j in range(0, len(idxs), max_fold):
                part = idxs[j:j + max_fold]
                e.eval_forward_batch(torch.stack([imgs[i] for i in part]).contiguous(), use_graph=True)
                for b, i in enumerate(part):
                    boxes, scores, _ = e.detections(b)
                    H, W = imgs[i].shape[-2:]
                    res = Instances((H, W))
                    res.pred_boxes = Boxes(boxes.clone())
                    res.scores = scores.clone()
                    res.pred_classes = torch.zeros(len(scores), dtype=torch.int64, device=scores.device)
                    results[i] = res
        if do_postprocess:
            sizes = [tuple(im.shape[-2:]) for im in imgs]
            return CenterNet2Detector._postprocess(results, requests, sizes)
        return results

    def preprocess_image(self, batched_inputs):
        """ref fsod_cen.py:540-555 (kept for API parity; the engine fuses this into stem_1)."""
        images = [x["image"].to(self.device) for x in batched_inputs]
        images = [(x - self.pixel_mean) / self.pixel_std for x in images]
        return ImageList.from_tensors(images, self.backbone.size_divisibility)

    @staticmethod
    def _postprocess(instances, batched_inputs, image_sizes):
        out = []
        for res, inp, size in zip(instances, batched_inputs, image_sizes):
            r = detector_postprocess(res, inp.get("height", size[0]), inp.get("width", size[1]))
            out.append({"instances": r})
        return out
