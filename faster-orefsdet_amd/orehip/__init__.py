"""ctypes binding of libore_hip.so (include/ore_hip.h) -- the only way the Python host side reaches
the HIP kernels.  PyTorch is used for device memory (tensor.data_ptr()) and streams only.

There is NO CPU fallback: if the library is missing or a call fails, an exception is raised.

The package is the surface; the code lives in one submodule per subsystem, and only the forward conv/op wrappers and the Engine are
still in this file.  Every name a submodule defines is re-exported below by name, bound to the one object the submodule uses (the
caches are those very dicts).  Two names are rebound by their own module after import, so the package keeps their initial None:
_lib (lib()) and _OVERLAY_ATLAS (overlay_atlas()); go through the functions.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from ._capi import (_PKG, CSRC, HEADER, ESE_PARTS, OreError, build, ConvDesc, ConvPlan, DetectDesc, ModelCfg, _PARAM_TYPES,
    _RESULT_TYPES, _prototypes, _PROTOTYPES, SYMBOLS, _lib, lib, _chk, _RAW_STREAM, _stream, _ptr, _f32, _i32s, _Arr, _from_ptr)

# The four names that callers rebind on the package.  They are defined here and nowhere else, and the functions that consult them (lib
# and build; roi_align_bwd; _s2_image_groups) read orehip.NAME when called, so a new value reaches them.
LIB_PATH = os.path.join(_PKG, "lib", "libore_hip.so")
ROI_BWD_DETERMINISTIC = True          # False: the fp32-atomics form of rounds 1-4 (order-dependent in the last bits; A/B aid)
ROI_BWD_MODE = "tiled"                # the deterministic form: "tiled" (gather, one block per map tile, no atomics) | "fixed" (64-bit fixed-point atomics)
# The stride-2 gradient kernels address a tensor through 32-bit byte offsets and refuse one of 2 GiB or more (ORE_EINVAL).  The bindings
# therefore hand them the batch in groups of whole images whose tensors stay below this many bytes (a margin of 1 MiB for the rows a last
# step may name): one group -- one launch, as ever -- for everything but the support batch of a very large step.  A weight gradient adds the
# groups in order with beta = 1, so it stays deterministic; the order of that sum then depends on the grouping, i.e. on the shapes alone.
_S2_MAX_BYTES = (1 << 31) - (1 << 20)

from .detect import (_detect_spec, _detect_desc, detect, detect_batch, CocoEvalDesc, CocoEvalImages, coco_eval, ProposalRecallDesc,
    proposal_recall_sizes, proposal_recall, nms, _roi_levels, roi_align, roi_align_batched, roi_align_bwd, roi_predict,
    roi_cascade_refine, cascade_relabel)
from .image import (to_device, RESIZE_FORM_LDS, RESIZE_FORM_WORKSPACE, resize_shortest_edge_shape, resize_plan, resize_form,
    _RESIZE_TABLES, _RESIZE_TABLES_MAX, _RESIZE_WS, _table_uploaded, _table_on_stream, _cached_table, _resize_tables, resize_bilinear_u8,
    SUPPORT_JOB_INTS, SUPPORT_FILL, _SJ_H, _SJ_RECT, _SJ_DST, _SJ_XB, _SJ_YB, _SJ_KX, _SJ_KY, _SJ_KSX, _SJ_KSY, _SJ_FORM, _SJ_D, _SJ_X0,
    _SJ_BOX, _SUPPORT_BUF, _support_box, _support_refused, support_crop_form, support_crop_plan, support_crops, BATCH_CANVAS_JOB_INTS,
    _BCJ_SRC, _BCJ_H, _BCJ_W, _BCJ_DST, _BCJ_HC, _BCJ_WC, BatchCanvasGeom, BatchCanvasPlan, _canvas_group, batch_canvas_plan,
    batch_canvas)
from .tta_tile import (TTA_MAX_CANDIDATES, tta_hflip_u8, TTAPool, tta_collect, tta_merge, record_views, TILE_MAX_SIDE, TILE_MAX_TILES,
    TILE_EDGE_LEFT, TILE_EDGE_TOP, TILE_EDGE_RIGHT, TILE_EDGE_BOTTOM, _tile_axis, tile_plan, tile_edges, tile_gather_host,
    tile_collect_host, TilePool, tile_gather_u8, tile_collect)
from .overlay import (OVERLAY_MAX_SIDE, OVERLAY_TEXT, OVERLAY_NAME, OVERLAY_PALETTE, _OVERLAY_ATLAS, _OVERLAY_TABLES,
    _OVERLAY_TABLES_MAX, _OVERLAY_WS, _OVERLAY_WS_MAX, overlay_atlas, overlay_names_table, _overlay_palette, _overlay_color_by,
    _overlay_table_dev, overlay_draw, _blend8, overlay_instance_table, overlay_host)
from .track import (TRACK_MAX_TRACKS, TRACK_WIDE_MAX_TRACKS, TRACK_WIDE_MAX_ROWS, TRACK_WIDE_DEFAULTS, TRACK_DEFAULTS, _TRACK_HEADER,
    _track_params, track_state_empty, track_host, BoxTracker, WideBoxTracker)
from .belt import (BELT_MAX_HALF_BINS, BELT_BINS, BELT_DEFAULTS, belt_state_empty, belt_shift_host, BeltTracker, WideBeltTracker)
from .rectify import (RECTIFY_MAX_SIDE, _rectify_m9, _rectify_hw, _rectify_fill, rectify_host, rectify_u8, homography_from_quad,
    Rectifier)
from .heatmap import (HEATMAP_MEAN, HEATMAP_MAX_LEVELS, HEATMAP_MAX_MAP_SIDE, HEATMAP_MAX_INPUT_SIDE, HEATMAP_MAX_STRIDE, HEATMAP_LUTS,
    _HEATMAP_TRANSFORMS, _HEATMAP_NORMS, _HEATMAP_ALPHA_MODES, _HEATMAP_LEVEL_BUFFERS, _HEATMAP_WS, _HEATMAP_WS_MAX, heatmap_lut,
    _heatmap_style, _heatmap_geometry, heat_kind, HeatSource, HeatLevels, heatmap_levels, _heatmap_levels_arg, heatmap_draw,
    sigmoid_host, heatmap_levels_host, _heatmap_taps, heatmap_host)
from .train import (centernet_targets, centernet_loss_sums, centernet_loss_grad, sample_rois, roi_losses, sgd_step, GRAD_NORM_KINDS,
    grad_norm_geometry, grad_norm_workspace, grad_norms, sgd_step_norm, pack_conv_weight_dev, PackJob, _PACK_TABLES,
    pack_conv_weights_multi, _WGWS, _wgrad_ws, conv2d_wgrad, _s2_out_hw, _s2_image_groups, conv2d_wgrad_s2, conv2d_dgrad_s2,
    stem1_wgrad, _dw_out, dwpw, dwpw_prefers_composition, dw3x3, dw3x3_wgrad, relu_affine_bwd, colsum, colsum_segments,
    correlation_train_fwd, correlation_train_bwd, groupnorm_apply, groupnorm_bwd, prod_colsum, scale_add_channels,
    adaptive_avgpool_nhwc, group_mean, sm_permute, combine2, combine2_bwd, maxpool3x3s2_bwd, sumpool2x2)


# ---------------------------------------------------------------------------------------------------
# layout helpers: the library is NHWC; torch.channels_last IS that layout for a logical NCHW tensor
# ---------------------------------------------------------------------------------------------------
def to_nhwc(x_nchw: torch.Tensor) -> torch.Tensor:
    """[B,C,H,W] any layout -> contiguous [B,H,W,C] fp32."""
    return x_nchw.permute(0, 2, 3, 1).contiguous().float()


def as_nchw(x_nhwc: torch.Tensor) -> torch.Tensor:
    """[B,H,W,C] -> logical [B,C,H,W] view (channels_last strides, zero copy)."""
    return x_nhwc.permute(0, 3, 1, 2)


def pack_conv_weight(w_oihw: torch.Tensor) -> torch.Tensor:
    """OIHW (any device) -> packed [Cout16][kh*kw*Cin] on the weight's device."""
    w = w_oihw.detach().float().cpu().contiguous()
    co, ci, kh, kw = w.shape
    n = lib().ore_packed_weight_floats(co, ci, kh, kw)
    dst = np.empty(n, dtype=np.float32)
    _chk(lib().ore_pack_conv_weight_host(w.data_ptr(), co, ci, kh, kw, dst.ctypes.data), "ore_pack_conv_weight_host")
    return torch.from_numpy(dst).to(w_oihw.device)


def pack_conv_weight_bf16(w_oihw: torch.Tensor) -> torch.Tensor:
    """OIHW fp32 (any device) -> bf16 packed [Cout16][kh*kw][round_up(Cin, 32)] on the weight's device (ORE_ST_BF16 convs)."""
    w = w_oihw.detach().float().cpu().contiguous()
    co, ci, kh, kw = w.shape
    n = lib().ore_packed_weight_bf16_elems(co, ci, kh, kw)
    dst = np.empty(n, dtype=np.uint16)
    _chk(lib().ore_pack_conv_weight_bf16_host(w.data_ptr(), co, ci, kh, kw, dst.ctypes.data), "ore_pack_conv_weight_bf16_host")
    return torch.from_numpy(dst.view(np.int16)).view(torch.bfloat16).to(w_oihw.device)


def winograd_covers(Cout: int, Cin: int) -> bool:
    """True if a Winograd build exists for a 3x3 stride-1 layer of these widths (ore_winograd_covers)."""
    return bool(lib().ore_winograd_covers(int(Cout), int(Cin)))


def winograd_weight(w_packed: torch.Tensor, Cout: int, Cin: int) -> torch.Tensor:
    """Packed 3x3 weights ([Cout16][9][Cin], pack_weight) -> their Winograd F(2x2,3x3) form U [16][Cout16][Cin] on the device."""
    _f32(w_packed)
    U = torch.empty(int(lib().ore_winograd_weight_floats(Cout, Cin)), device=w_packed.device, dtype=torch.float32)
    _chk(lib().ore_winograd_weight_fwd(_ptr(w_packed), Cout, Cin, _ptr(U), _stream()), "ore_winograd_weight_fwd")
    return U


def _bf16_in_with_slack(x: torch.Tensor, Cin: int, in_coff: int, ld: int) -> torch.Tensor:
    """ore_hip.h (ORE_ST_BF16): when Cin % 32 == 16 and the slice ends at the row end, the last K chunk of the LAST row reads 16
    channels (32 bytes) past the tensor against zero weights -- the bytes must exist and be finite (0 * NaN = NaN).  A tensor whose
    storage already extends that far (a view into a wider buffer: the caller owns what lies there, as the header says) is taken as
    it is; a plain tensor, whose storage ends with its last element, is copied once into a buffer with 16 zeroed elements of slack."""
    if Cin % 32 == 0 or in_coff + Cin != ld:
        return x
    end = x.storage_offset() + x.numel()
    if x.untyped_storage().nbytes() // 2 - end >= 16:
        return x
    buf = torch.empty(x.numel() + 16, device=x.device, dtype=torch.bfloat16)
    buf[x.numel():].zero_()
    buf[:x.numel()].copy_(x.reshape(-1))
    return buf[:x.numel()].view(x.shape)


def conv2d(x: torch.Tensor, w_packed: torch.Tensor, Cout: int, k: int, stride: int = 1, pad: Optional[int] = None, *,
           in_coff: int = 0, Cin: Optional[int] = None, scale=None, shift=None, relu_cout: int = 0, in_mul=None,
           in_add=None, in_relu: bool = False, add: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
           out_coff: int = 0, splitk: int = 0, workspace: Optional[torch.Tensor] = None, want_colsum: bool = False,
           w_wino: Optional[torch.Tensor] = None, out_f32: bool = False):
    """x: [B,H,W,ld] NHWC fp32.  Returns `out` ([B,Ho,Wo,out_ld]); only channels [out_coff, out_coff+Cout) are written.
    w_wino: the same weights in Winograd F(2x2,3x3) form (winograd_weight); lets the large-M 3x3 layers run on the Winograd kernel.
    bf16 storage (ORE_ST_BF16): x / w_packed (pack_conv_weight_bf16) / add are torch.bfloat16; `out` is bf16, or fp32 when out_f32."""
    st_bf16 = x.dtype == torch.bfloat16
    if st_bf16:
        assert x.is_contiguous() and w_packed.dtype == torch.bfloat16 and (add is None or add.dtype == torch.bfloat16)
    else:
        _f32(x)
    B, H, W, ld = x.shape
    Cin = Cin if Cin is not None else ld - in_coff
    if st_bf16:
        x = _bf16_in_with_slack(x, Cin, in_coff, ld)
    pad = k // 2 if pad is None else pad
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    out_dt = torch.bfloat16 if (st_bf16 and not out_f32) else torch.float32
    if out is None:
        out = torch.empty(B, Ho, Wo, Cout, device=x.device, dtype=out_dt)
    assert out.dtype == out_dt and out.is_contiguous()
    assert out.shape[:3] == (B, Ho, Wo)
    M = B * Ho * Wo
    if workspace is None and splitk != 1:
        workspace = _default_ws(x.device)
    d = ConvDesc()
    d.in_, d.in_ld, d.in_coff = _ptr(x), ld, in_coff
    d.B, d.H, d.W, d.Cin = B, H, W, Cin
    d.storage = (2 if out_f32 else 1) if st_bf16 else 0
    d.w = _ptr(w_packed if st_bf16 else _f32(w_packed))
    d.Cout, d.kh, d.kw, d.stride, d.pad = Cout, k, k, stride, pad
    d.scale, d.shift, d.relu_cout = _ptr(scale), _ptr(shift), relu_cout
    d.in_mul, d.in_add, d.in_relu = _ptr(in_mul), _ptr(in_add), int(in_relu)
    if add is not None:
        assert add.is_contiguous()
        d.add, d.add_ld, d.add_coff = _ptr(add), add.shape[-1], 0
    d.out, d.out_ld, d.out_coff = _ptr(out), out.shape[-1], out_coff
    d.splitk = splitk
    d.w_wino = _ptr(w_wino)
    if workspace is not None:
        d.workspace, d.workspace_floats = _ptr(workspace), workspace.numel()
    colsum = None
    if want_colsum:
        rows = lib().ore_conv_colsum_rows(C.byref(d))
        colsum = torch.zeros(rows, (Cout + 15) // 16 * 16, device=x.device, dtype=torch.float32)
        d.colsum = _ptr(colsum)
    _chk(lib().ore_conv2d_fwd(C.byref(d), _stream()), "ore_conv2d_fwd")
    return (out, colsum) if want_colsum else out


def conv2d_levels(x_rows: torch.Tensor, HW: Sequence[Tuple[int, int]], B: int, w_packed: torch.Tensor, Cout: int, k: int, *,
                  in_coff: int = 0, Cin: Optional[int] = None, scale=None, shift=None, ep_stride: int = 0, relu_cout: int = 0,
                  in_mul=None, in_add=None, in_relu: bool = False, out: Optional[torch.Tensor] = None, out_coff: int = 0,
                  splitk: int = 0, w_wino: Optional[torch.Tensor] = None, out_f32: bool = False, w_wino_level_stride: int = 0,
                  w_level_stride: int = 0) -> torch.Tensor:
    """One launch over several pyramid levels: x_rows [sum_l B*H_l*W_l, ld] level-major (fp32, or bf16 = ORE_ST_BF16 storage)."""
    st_bf16 = x_rows.dtype == torch.bfloat16
    if not st_bf16:
        _f32(x_rows)
    rows, ld = x_rows.shape
    assert rows == sum(B * h * w for h, w in HW)
    Cin = Cin if Cin is not None else ld - in_coff
    if st_bf16:
        x_rows = _bf16_in_with_slack(x_rows, Cin, in_coff, ld)
    out_dt = torch.bfloat16 if (st_bf16 and not out_f32) else torch.float32
    if out is None:
        out = torch.empty(rows, Cout, device=x_rows.device, dtype=out_dt)
    assert out.dtype == out_dt and out.is_contiguous()
    ws = _default_ws(x_rows.device)
    d = ConvDesc()
    d.in_, d.in_ld, d.in_coff = _ptr(x_rows), ld, in_coff
    d.B, d.H, d.W, d.Cin = B, 0, 0, Cin
    d.storage = (2 if out_f32 else 1) if st_bf16 else 0
    d.w = _ptr(w_packed)
    d.Cout, d.kh, d.kw, d.stride, d.pad = Cout, k, k, 1, k // 2
    d.scale, d.shift, d.relu_cout = _ptr(scale), _ptr(shift), relu_cout
    d.in_mul, d.in_add, d.in_relu = _ptr(in_mul), _ptr(in_add), int(in_relu)
    d.out, d.out_ld, d.out_coff = _ptr(out), out.shape[-1], out_coff
    d.splitk, d.workspace, d.workspace_floats = splitk, _ptr(ws), ws.numel()
    d.w_wino = _ptr(w_wino)
    d.w_wino_level_stride = int(w_wino_level_stride)   # != 0: the levels are different layers of one shape, w_wino = [L][stride] (Winograd only)
    d.w_level_stride = int(w_level_stride)             # the same for bf16 storage: w_packed = [L][stride] bf16 (weight-stationary 3x3 kernel)
    _chk(lib().ore_conv2d_levels_fwd(C.byref(d), len(HW), _i32s(h for h, _ in HW), _i32s(w for _, w in HW), ep_stride, _stream()),
         "ore_conv2d_levels_fwd")
    return out


def correlation_levels(q_rows: torch.Tensor, HW: Sequence[Tuple[int, int]], B: int, k11, k13, k31, Cc: int, q_coff: int = 0,
                       out: Optional[torch.Tensor] = None, out_coff: int = 0) -> torch.Tensor:
    _f32(q_rows)
    if out is None:
        out = torch.empty(q_rows.shape[0], Cc, device=q_rows.device, dtype=torch.float32)
    _chk(lib().ore_correlation_levels_fwd(_ptr(q_rows), q_rows.shape[-1], q_coff, B, len(HW), _i32s(h for h, _ in HW),
                                          _i32s(w for _, w in HW), Cc, _ptr(_f32(k11)), _ptr(_f32(k13)), _ptr(_f32(k31)), _ptr(out),
                                          out.shape[-1], out_coff, _stream()), "ore_correlation_levels_fwd")
    return out


def groupnorm_affine_levels(x_rows: torch.Tensor, HW: Sequence[int], B: int, groups: int, gamma, beta, eps: float = 1e-5):
    _f32(x_rows)
    Cc = x_rows.shape[-1]
    L = len(HW)
    mul = torch.empty(L * B, Cc, device=x_rows.device)
    add = torch.empty(L * B, Cc, device=x_rows.device)
    ws = torch.empty(sum(B * ((hw + 63) // 64) for hw in HW) * groups * 2 + 64, device=x_rows.device)
    _chk(lib().ore_groupnorm_affine_levels_fwd(_ptr(x_rows), Cc, 0, B, L, _i32s(HW), Cc, groups, eps, _ptr(_f32(gamma)), _ptr(_f32(beta)),
                                               _ptr(mul), _ptr(add), _ptr(ws), _stream()), "ore_groupnorm_affine_levels_fwd")
    return mul, add


def ese_gate_from_colsum(part: torch.Tensor, HW: int, fc_w: torch.Tensor, fc_b: torch.Tensor) -> torch.Tensor:
    """part [P, C] (B = 1): the fused column sums of the concat conv."""
    _f32(part)
    P, Cc = part.shape
    gate = torch.empty(1, Cc, device=part.device, dtype=torch.float32)
    mean_ws = torch.empty(Cc, device=part.device, dtype=torch.float32)
    _chk(lib().ore_ese_gate_from_colsum_fwd(_ptr(part), P, 1, HW, Cc, _ptr(_f32(fc_w.reshape(Cc, Cc))), _ptr(_f32(fc_b)), _ptr(gate),
                                            _ptr(mean_ws), _stream()), "ore_ese_gate_from_colsum_fwd")
    return gate


def ese_gate_scaled_weight(part: torch.Tensor, HW: int, fc_w: torch.Tensor, fc_b: torch.Tensor, w_packed: torch.Tensor):
    """ese_gate_from_colsum for one image plus, in the same launch, the gate-scaled copy of a consumer's packed 1x1 weight [rows, C]
    (ore_ese_gate_scaled_weight_fwd).  Returns (gate [1, C], w_packed * gate[None, :])."""
    _f32(part); _f32(w_packed)
    P, Cc = part.shape
    assert w_packed.dim() == 2 and w_packed.shape[1] == Cc
    gate = torch.empty(1, Cc, device=part.device, dtype=torch.float32)
    mean_ws = torch.empty(Cc, device=part.device, dtype=torch.float32)
    ws = torch.empty_like(w_packed)
    _chk(lib().ore_ese_gate_scaled_weight_fwd(_ptr(part), P, HW, Cc, _ptr(_f32(fc_w.reshape(Cc, Cc))), _ptr(_f32(fc_b)), _ptr(gate),
                                              _ptr(mean_ws), _ptr(w_packed), w_packed.shape[0], _ptr(ws), _stream()),
         "ore_ese_gate_scaled_weight_fwd")
    return gate, ws


_WS: Dict[str, torch.Tensor] = {}


def _default_ws(device) -> torch.Tensor:
    k = str(device)
    if k not in _WS:
        _WS[k] = torch.zeros(lib().ore_conv_workspace_floats(), device=device, dtype=torch.float32)  # counters (zero) + slabs
    return _WS[k]


def stem1(img: torch.Tensor, Hp: int, Wp: int, mean: Sequence[float], std: Sequence[float], w_oihw: torch.Tensor,
          scale: torch.Tensor, shift: torch.Tensor, out_bf16: bool = False) -> torch.Tensor:
    """img [B,3,H,W] uint8 or fp32 (planar) -> [B,Hp/2,Wp/2,Cout] fp32, or bf16 (rounded once; fp32 arithmetic) when out_bf16."""
    assert img.is_contiguous() and img.dtype in (torch.uint8, torch.float32)
    B, _, H, W = img.shape
    Cout = w_oihw.shape[0]
    out = torch.empty(B, Hp // 2, Wp // 2, Cout, device=img.device, dtype=torch.bfloat16 if out_bf16 else torch.float32)
    m = (C.c_float * 3)(*mean)
    s = (C.c_float * 3)(*std)
    fn = lib().ore_stem1_bf16_fwd if out_bf16 else lib().ore_stem1_fwd
    _chk(fn(_ptr(img), int(img.dtype == torch.uint8), B, H, W, Hp, Wp, m, s, _ptr(_f32(w_oihw)), _ptr(scale), _ptr(shift), Cout, _ptr(out),
            Cout, 0, _stream()), fn.__name__)
    return out


def maxpool3x3s2(x: torch.Tensor, in_mul: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, out_coff: int = 0) -> torch.Tensor:
    """MaxPool2d(3, 2, ceil_mode=True) on NHWC (optionally of x * in_mul[b][c], in_mul > 0).  `out` [B,Ho,Wo,ld] + out_coff: write the
    result into a channel slice of a wider buffer (the next block's concat buffer) instead of a fresh tensor.  bf16 in -> bf16 out
    (the product with the fp32 multiplier is rounded once)."""
    bf = x.dtype == torch.bfloat16
    assert x.is_contiguous() and (bf or x.dtype == torch.float32)
    B, H, W, Cc = x.shape
    Ho, Wo = maxpool3x3s2_out_hw(H, W)
    if out is None:
        out = torch.empty(B, Ho, Wo, Cc, device=x.device, dtype=x.dtype)
    else:
        assert out.dtype == x.dtype and out.is_contiguous()
        assert tuple(out.shape[:3]) == (B, Ho, Wo) and out_coff + Cc <= out.shape[-1] and out_coff % 4 == 0
    fn = lib().ore_maxpool3x3s2_bf16_fwd if bf else lib().ore_maxpool3x3s2_fwd
    _chk(fn(_ptr(x), Cc, 0, B, H, W, Cc, _ptr(in_mul), _ptr(out), out.shape[-1], out_coff, _stream()), fn.__name__)
    return out


def maxpool3x3s2_out_hw(H: int, W: int) -> Tuple[int, int]:
    def osz(n):
        o = (n - 3 + 1) // 2 + 1 if n >= 3 else 1
        if (o - 1) * 2 >= n:
            o -= 1
        return max(o, 1)
    return osz(H), osz(W)


def ese_gate(x: torch.Tensor, fc_w: torch.Tensor, fc_b: torch.Tensor) -> torch.Tensor:
    """relu6(fc(mean_hw(x)) + 3) / 6 per image: [B,C] fp32, from an fp32 or a bf16 map."""
    bf = x.dtype == torch.bfloat16
    assert x.is_contiguous() and (bf or x.dtype == torch.float32)
    B, H, W, Cc = x.shape
    gate = torch.empty(B, Cc, device=x.device, dtype=torch.float32)
    ws = torch.empty(B * (ESE_PARTS + 1) * Cc, device=x.device, dtype=torch.float32)
    fn = lib().ore_ese_gate_bf16_fwd if bf else lib().ore_ese_gate_fwd
    _chk(fn(_ptr(x), Cc, 0, B, H * W, Cc, _ptr(_f32(fc_w.reshape(Cc, Cc))), _ptr(_f32(fc_b)), _ptr(gate), _ptr(ws), _stream()), fn.__name__)
    return gate


def ese_gate_pool(part: torch.Tensor, fc_w: torch.Tensor, fc_b: torch.Tensor, x: torch.Tensor, w_packed: Optional[torch.Tensor] = None):
    """One image: gate from the concat conv's fused column sums `part` [P, C], the gate-scaled copy of `w_packed` [rows, C] (or None)
    and maxpool3x3s2(x * gate) in one launch (ore_ese_gate_pool_fwd).  x [1,H,W,C] fp32 or bf16.  Returns (gate [1,C], pooled, scaled)."""
    _f32(part)
    P, Cc = part.shape
    _, H, W, Cx = x.shape
    assert x.shape[0] == 1 and Cx == Cc and x.is_contiguous()
    Ho, Wo = maxpool3x3s2_out_hw(H, W)
    gate = torch.empty(1, Cc, device=x.device, dtype=torch.float32)
    out = torch.empty(1, Ho, Wo, Cc, device=x.device, dtype=x.dtype)
    bf = x.dtype == torch.bfloat16
    ws = None
    if w_packed is not None:
        _f32(w_packed)
        ws = torch.empty(w_packed.shape, device=x.device, dtype=x.dtype)
    fn = lib().ore_ese_gate_pool_bf16_fwd if bf else lib().ore_ese_gate_pool_fwd
    _chk(fn(_ptr(part), P, H * W, Cc, _ptr(_f32(fc_w.reshape(Cc, Cc))), _ptr(_f32(fc_b)), _ptr(gate), _ptr(w_packed),
            0 if w_packed is None else w_packed.shape[0], _ptr(ws), _ptr(x), Cc, 0, H, W, _ptr(out), Cc, 0, _stream()), fn.__name__)
    return gate, out, ws


def scale_channels(x: torch.Tensor, gate: torch.Tensor) -> torch.Tensor:
    _f32(x)
    B, H, W, Cc = x.shape
    y = torch.empty_like(x)
    _chk(lib().ore_scale_channels_fwd(_ptr(x), Cc, 0, B, H * W, Cc, _ptr(_f32(gate)), _ptr(y), Cc, 0, _stream()), "ore_scale_channels_fwd")
    return y


def _rows_ld(t: torch.Tensor) -> Tuple[int, int]:
    """(rows, ld) of a contiguous fp32 [..., ld] map."""
    _f32(t)
    return t.numel() // t.shape[-1], t.shape[-1]


def ese_gate_residual(part: torch.Tensor, fc_w: torch.Tensor, fc_b: torch.Tensor, y: torch.Tensor, x: Optional[torch.Tensor],
                      out: torch.Tensor, y_coff: int = 0, x_coff: int = 0, out_coff: int = 0) -> torch.Tensor:
    """The tail of an OSA identity block for one image in one launch (ore_ese_gate_residual_fwd): the gate [1, C] from the concat
    conv's fused column sums `part` [P, C], and out[..., out_coff + c] = y[..., y_coff + c] * gate[c] + x[..., x_coff + c] over the
    rows of the maps ([..., ld] each, the same row count).  x = None: out = y * gate.  Returns the gate; `out` is written in place."""
    _f32(part)
    P, Cc = part.shape
    HW, y_ld = _rows_ld(y)
    rows_o, out_ld = _rows_ld(out)
    assert rows_o == HW and (x is None or _rows_ld(x)[0] == HW), "y, x and out have the same rows"
    gate = torch.empty(1, Cc, device=part.device, dtype=torch.float32)
    _chk(lib().ore_ese_gate_residual_fwd(_ptr(part), P, HW, Cc, _ptr(_f32(fc_w.reshape(Cc, Cc))), _ptr(_f32(fc_b)), _ptr(gate), _ptr(y), y_ld,
                                         y_coff, _ptr(x), 0 if x is None else x.shape[-1], x_coff, _ptr(out), out_ld, out_coff, _stream()),
         "ore_ese_gate_residual_fwd")
    return gate


def scale_residual(y: torch.Tensor, gate: torch.Tensor, x: Optional[torch.Tensor], out: torch.Tensor, y_coff: int = 0, x_coff: int = 0,
                   out_coff: int = 0) -> torch.Tensor:
    """The same tail for B images with the gates given (ore_scale_residual_fwd): y, x, out [B, ..., ld], gate [B, C]."""
    _f32(gate)
    B, Cc = gate.shape
    rows, y_ld = _rows_ld(y)
    rows_o, out_ld = _rows_ld(out)
    assert y.shape[0] == B and rows % B == 0 and rows_o == rows and (x is None or _rows_ld(x)[0] == rows), "y, x and out have the same rows"
    _chk(lib().ore_scale_residual_fwd(_ptr(y), y_ld, y_coff, _ptr(gate), _ptr(x), 0 if x is None else x.shape[-1], x_coff, B, rows // B, Cc,
                                      _ptr(out), out_ld, out_coff, _stream()), "ore_scale_residual_fwd")
    return out


def support_kernels(proto_chw: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    _f32(proto_chw)
    Cc, s, s2 = proto_chw.shape
    assert s == s2
    k11 = torch.empty(Cc, device=proto_chw.device)
    k13 = torch.empty(Cc, 3, device=proto_chw.device)
    k31 = torch.empty(Cc, 3, device=proto_chw.device)
    _chk(lib().ore_support_kernels_fwd(_ptr(proto_chw), Cc, s, _ptr(k11), _ptr(k13), _ptr(k31), _stream()), "ore_support_kernels_fwd")
    return k11, k13, k31


def correlation(q: torch.Tensor, k11, k13, k31, out: Optional[torch.Tensor] = None, q_coff: int = 0, out_coff: int = 0,
                Cc: Optional[int] = None) -> torch.Tensor:
    _f32(q)
    B, H, W, ld = q.shape
    Cc = Cc if Cc is not None else ld
    if out is None:
        out = torch.empty(B, H, W, Cc, device=q.device, dtype=torch.float32)
    _chk(lib().ore_correlation_fwd(_ptr(q), ld, q_coff, B, H, W, Cc, _ptr(_f32(k11)), _ptr(_f32(k13)), _ptr(_f32(k31)), _ptr(out),
                                   out.shape[-1], out_coff, _stream()), "ore_correlation_fwd")
    return out


def groupnorm_affine(x: torch.Tensor, groups: int, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5):
    _f32(x)
    B, H, W, Cc = x.shape
    mul = torch.empty(B, Cc, device=x.device)
    add = torch.empty(B, Cc, device=x.device)
    ws = torch.empty(B * ((H * W + 63) // 64) * groups * 2, device=x.device)
    _chk(lib().ore_groupnorm_affine_fwd(_ptr(x), Cc, 0, B, H * W, Cc, groups, eps, _ptr(_f32(gamma)), _ptr(_f32(beta)), _ptr(mul),
                                        _ptr(add), _ptr(ws), _stream()), "ore_groupnorm_affine_fwd")
    return mul, add


def set_conv_precision(mode: str) -> str:
    """"fp32" (default), "bf16" (operands of the MFMA conv kernels rounded to bf16, fp32 tensors) or "bf16s" (bf16 STORAGE: engines
    created under it keep bf16 activations / weights in HBM and LDS) -- include/ore_hip.h, ore_conv_set_precision; engines keep the mode
    in force when they were created.  Returns the previous mode."""
    prev = get_conv_precision()
    _chk(lib().ore_conv_set_precision({"fp32": 0, "bf16": 1, "bf16s": 2}[mode]), "ore_conv_set_precision")
    return prev


def get_conv_precision() -> str:
    return ("fp32", "bf16", "bf16s")[int(lib().ore_conv_get_precision())]


# ORE_LAUNCH_* of include/ore_hip.h, in that order
CONV_LAUNCHERS = ("none", "k_conv3x3_wino", "k_conv3x3_wino_nu", "k_conv_gd", "k_conv3x3_patch<4>", "k_conv3x3_patch<8>", "k_conv3x3_patch_db",
                  "k_conv3x3_ws<2,64>", "k_conv3x3_ws<2,128>", "k_conv_kd", "k_conv_rf", "k_conv_gs", "k_conv_kw", "k_conv_igemm",
                  "k_conv3x3_ws<bf16 storage>")


def conv_last_launch() -> Tuple[str, int]:
    """(launcher, split-K S) of this thread's last conv2d / conv2d_levels call (ore_conv_last_launch; a test hook)."""
    s = C.c_int32(1)
    code = int(lib().ore_conv_last_launch(C.byref(s)))
    return CONV_LAUNCHERS[code], int(s.value)


def conv_plan(d: ConvDesc, levels: Optional[Sequence[Tuple[int, int]]] = None, ep_stride: int = 0) -> ConvPlan:
    """The plan an ore_conv2d_fwd (levels None) or ore_conv2d_levels_fwd call with this descriptor makes now (ore_conv_plan); raises
    OreError with the call's error when no kernel takes it."""
    pl = ConvPlan()
    if levels is None:
        rc = lib().ore_conv_plan(C.byref(d), 0, None, None, 0, C.byref(pl))
    else:
        rc = lib().ore_conv_plan(C.byref(d), len(levels), _i32s(h for h, _ in levels), _i32s(w for _, w in levels), ep_stride, C.byref(pl))
    _chk(rc, "ore_conv_plan")
    return pl


@contextlib.contextmanager
def conv_overrides(*codes: Sequence[int]):
    """Tuning aids for the duration of a block: ore_conv_set_plan_override(*code) for each code (padded with zeros to its five
    arguments); every override is reset to the automatic plan on exit, also when the block raises."""
    try:
        for c in codes:
            c = tuple(c) + (0,) * (5 - len(c))
            _chk(lib().ore_conv_set_plan_override(*c), "ore_conv_set_plan_override")
        yield
    finally:
        lib().ore_conv_reset_plan_overrides()


def flop_counter(reset: bool = False) -> Tuple[float, int]:
    """(algorithmic FLOPs, calls) of the per-op conv entry points since the last reset (ore_flop_counter_read)."""
    v, n = C.c_double(0.0), C.c_int64(0)
    _chk(lib().ore_flop_counter_read(C.byref(v), C.byref(n), int(reset)), "ore_flop_counter_read")
    return float(v.value), int(n.value)


def event_pair_overhead_us(reps: int = 200) -> float:
    """Median (event, empty launch, event) time on the current stream (see ore_event_pair_overhead_us)."""
    v = C.c_double(0.0)
    _chk(lib().ore_event_pair_overhead_us(_stream(), reps, C.byref(v)), "ore_event_pair_overhead_us")
    return float(v.value)


def compose_roi_head(sd, support_8: torch.Tensor, prefix: str = "roi_heads.", stage: int = 0):
    """The eval second stage between ROIAlign and fc1's ReLU is linear in the pooled features:
         a = conv3(cat(x, s)) + cat(conv1(x), conv2(s));  h = relu(fc1(flatten(a)))        (fsod_roi_heads.py:500-520)
    so it folds, once per (weights, support set), into h = relu(W' x_flat + b') with x_flat ordered [pos][channel]
    (the ROIAlign kernel's output order).  Returns (W' [fc, 64*C] fp32, b' [fc] fp32) on the CPU; done in fp64.
    stage: which box_head[stage].fc1 of a cascade closes the chain (conv1 / conv2 / conv3 are shared by the stages)."""
    f64 = torch.float64
    W3 = sd[prefix + "conv3.weight"].detach().cpu().to(f64).flatten(1)
    b3 = sd[prefix + "conv3.bias"].detach().cpu().to(f64)
    W1 = sd[prefix + "conv1.weight"].detach().cpu().to(f64).flatten(1)
    b1 = sd[prefix + "conv1.bias"].detach().cpu().to(f64)
    W2 = sd[prefix + "conv2.weight"].detach().cpu().to(f64).flatten(1)
    b2 = sd[prefix + "conv2.bias"].detach().cpu().to(f64)
    fw = sd[prefix + f"box_head.{int(stage)}.fc1.weight"].detach().cpu().to(f64)
    fb = sd[prefix + f"box_head.{int(stage)}.fc1.bias"].detach().cpu().to(f64)
    Cc = W1.shape[1]
    P = fw.shape[1] // Cc
    s = support_8.detach().cpu().to(torch.float32).mean(0).to(f64).reshape(Cc, P)        # mean over shots in fp32 like the reference
    Wc = W3[:, :Cc].clone()
    Wc[: W1.shape[0]] += W1
    const = W3[:, Cc:] @ s + b3[:, None]
    const[: W1.shape[0]] += b1[:, None]
    const[W1.shape[0]:] += W2 @ s + b2[:, None]
    f3 = fw.reshape(fw.shape[0], Cc, P)                                                    # [o][c][pos]  (NCHW flatten)
    Wp = torch.einsum("ocp,cd->opd", f3, Wc).reshape(fw.shape[0], P * Cc)                  # [o][pos*C + c']
    bp = fb + torch.einsum("ocp,cp->o", f3, const)
    return Wp.to(torch.float32).contiguous(), bp.to(torch.float32).contiguous()


# ---------------------------------------------------------------------------------------------------
class Engine:
    """ore_engine: whole eval hot path (backbone+FPN -> correlation -> head -> top-k/NMS) behind one call."""

    def __init__(self, *, stem=(64, 64, 128), conv=(64, 80, 96, 112), out=(112, 256, 384, 512), layers=3, fpn_ch=128,
                 strides=(8, 16, 32), pixel_mean=(103.530, 116.280, 123.675), pixel_std=(1.0, 1.0, 1.0),
                 score_thresh=1e-5, pre_topk=1000, nms_thresh=0.6, post_topk=256, max_batch=1, max_h=640, max_w=640,
                 device: int = 0, depthwise: bool = False, blocks: Sequence[int] = (1, 1, 1, 1)):
        """depthwise: one of the *-dw-* bodies (stem (64, 64, 64)): stem_2 / stem_3 and the stage layers are depthwise-separable units
        (ore_dwpw_fwd), load_state_dict takes the reference's dw names.  Refused (OreError) in the bf16 storage mode.
        blocks: OSA blocks per stage (ore_engine_set_blocks): (1, 1, 2, 2) is V-39-eSE, (1, 1, 4, 3) V-57-eSE, (1, 3, 9, 3) V-99-eSE, with
        layers=5; load_state_dict then also takes the names of the identity blocks OSAk_2 ...  Refused (OreError) for a depthwise
        engine, in the bf16 storage mode, and for a count outside 1..16."""
        cfg = ModelCfg()
        cfg.stem_ch[:] = stem
        cfg.stage_conv_ch[:] = conv
        cfg.stage_out_ch[:] = out
        cfg.layers_per_block, cfg.fpn_ch = layers, fpn_ch
        cfg.strides[:] = strides
        cfg.pixel_mean[:] = pixel_mean
        cfg.pixel_std[:] = pixel_std
        cfg.score_thresh, cfg.pre_topk, cfg.nms_thresh, cfg.post_topk = score_thresh, pre_topk, nms_thresh, post_topk
        cfg.max_batch, cfg.max_h, cfg.max_w = max_batch, max_h, max_w
        self.cfg = cfg
        self.device = torch.device("cuda", device)
        self.pre_topk = pre_topk
        self.fpn_ch = fpn_ch
        self._h = C.c_void_p()
        _chk(lib().ore_engine_create(C.byref(cfg), device, C.byref(self._h)), "ore_engine_create")
        self.depthwise = bool(depthwise)
        if self.depthwise:
            _chk(lib().ore_engine_set_depthwise(self._h, 1), "ore_engine_set_depthwise")
        self.blocks = tuple(int(b) for b in blocks)
        assert len(self.blocks) == 4, blocks
        if any(b != 1 for b in self.blocks):
            _chk(lib().ore_engine_set_blocks(self._h, _i32s(self.blocks)), "ore_engine_set_blocks")

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().ore_engine_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load_state_dict(self, sd) -> None:
        """All tensors by their reference state_dict names; unknown keys are ignored by the engine."""
        for k, v in sd.items():
            t = v.detach().float().cpu().contiguous()
            shape = (C.c_int64 * max(t.dim(), 1))(*t.shape)
            _chk(lib().ore_engine_set_tensor(self._h, k.encode(), t.data_ptr(), shape, t.dim()), f"ore_engine_set_tensor({k})")

    def set_support(self, protos: Dict[str, torch.Tensor], slot: Optional[int] = None) -> None:
        """{'p3': [1,C,32,32], 'p4': [1,C,16,16], 'p5': [1,C,8,8]} -- support_feature.pkl prototypes.  slot=k: the prototypes of N-way
        class slot k instead (ore_engine_set_support_slot; after finalize() and set_classes())."""
        for lvl in (3, 4, 5):
            t = protos[f"p{lvl}"].detach().float().cpu().contiguous()
            t = t.reshape(t.shape[-3], t.shape[-2], t.shape[-1])
            if slot is None:
                _chk(lib().ore_engine_set_support(self._h, lvl, t.data_ptr(), t.shape[0], t.shape[1]), "ore_engine_set_support")
            else:
                _chk(lib().ore_engine_set_support_slot(self._h, int(slot), lvl, t.data_ptr(), t.shape[0], t.shape[1]),
                     "ore_engine_set_support_slot")

    def set_classes(self, ids: Sequence[int]) -> None:
        """N-way inference (include/ore_hip.h): class slot k answers for support class ids[k]; len(ids) <= max_batch and <= 16.  [] turns
        it off.  Each slot then needs set_support(..., slot=k) and, with a second stage, set_roi_support(..., slot=k)."""
        ids = [int(i) for i in ids]
        arr = (C.c_int64 * max(len(ids), 1))(*ids)
        _chk(lib().ore_engine_set_classes(self._h, len(ids), arr), "ore_engine_set_classes")
        self.class_ids = ids

    def set_roi_support(self, sd, support_8: torch.Tensor, slot: int, prefix: str = "roi_heads.") -> None:
        """The second stage of N-way class slot `slot`: DSA-mix + flatten + fc1 composed with that class's rcnn_8 support features
        (compose_roi_head), after set_roi_head() and set_classes()."""
        for k in range(getattr(self, "roi_stages", 1)):          # a cascade engine: every stage's fc1 composed with the class's features
            Wp, bp = compose_roi_head(sd, support_8, prefix, stage=k)
            if k == 0:
                _chk(lib().ore_engine_set_roi_support_slot(self._h, int(slot), Wp.data_ptr(), bp.data_ptr()), "ore_engine_set_roi_support_slot")
            else:
                _chk(lib().ore_engine_set_roi_support_slot_stage(self._h, int(slot), k, Wp.data_ptr(), bp.data_ptr()),
                     "ore_engine_set_roi_support_slot_stage")

    def finalize(self) -> None:
        _chk(lib().ore_engine_finalize(self._h), "ore_engine_finalize")

    def set_roi_head(self, sd, support_8: torch.Tensor, reg_weights=(10.0, 10.0, 5.0, 5.0), score_thresh: float = 0.0,
                     nms_thresh: float = 0.9, topk: int = 100, prefix: str = "roi_heads.") -> None:
        """Second stage inside the engine graph: composes DSA-mix + flatten + fc1 once (compose_roi_head) and uploads it."""
        Wp, bp = compose_roi_head(sd, support_8, prefix)
        f = lambda k: sd[prefix + k].detach().float().cpu().contiguous()
        cw, cb, bw, bb = f("box_predictor.0.cls_score.weight"), f("box_predictor.0.cls_score.bias"), f("box_predictor.0.bbox_pred.weight"), f("box_predictor.0.bbox_pred.bias")
        assert cw.shape[0] == 2 and bw.shape[0] == 4, "one foreground class, class-agnostic box regression"
        pooled = int(round((Wp.shape[1] // self.fpn_ch) ** 0.5))
        rw = (C.c_float * 4)(*reg_weights)
        _chk(lib().ore_engine_set_roi_head(self._h, Wp.data_ptr(), bp.data_ptr(), Wp.shape[0], pooled, cw.data_ptr(), cb.data_ptr(),
                                           bw.data_ptr(), bb.data_ptr(), rw, score_thresh, nms_thresh, topk), "ore_engine_set_roi_head")
        self.has_roi = True
        self.roi_stages = 1
        self._det_cap = min(max(int(topk), 1), 320)        # rows of the result tensors ore_engine_detect_fwd fills

    def set_roi_cascade(self, sd, support_8: torch.Tensor, reg_weights, score_thresh: float = 0.0, nms_thresh: float = 0.9, topk: int = 100,
                        prefix: str = "roi_heads.") -> None:
        """The second stage as a cascade of len(reg_weights) stages (ore_engine_set_roi_cascade): reg_weights = one 4-tuple per stage
        (MODEL.ROI_BOX_CASCADE_HEAD.BBOX_REG_WEIGHTS); box_head.k.fc1 is composed per stage, box_predictor.k uploaded per stage.  One
        stage is set_roi_head: the same launches."""
        K = len(reg_weights)
        if K < 1 or any(len(w) != 4 for w in reg_weights):
            raise OreError(f"set_roi_cascade: reg_weights must hold one 4-tuple per stage, got {reg_weights!r}")
        if prefix + f"box_head.{K - 1}.fc1.weight" not in sd:
            raise OreError(f"set_roi_cascade: {K} cascade stages asked for, the state dict has no {prefix}box_head.{K - 1}")
        f = lambda k: sd[prefix + k].detach().float().cpu().contiguous()      # noqa: E731
        keep, cols = [], [[] for _ in range(6)]
        for k in range(K):
            Wp, bp = compose_roi_head(sd, support_8, prefix, stage=k)
            ts = (Wp, bp, f(f"box_predictor.{k}.cls_score.weight"), f(f"box_predictor.{k}.cls_score.bias"),
                  f(f"box_predictor.{k}.bbox_pred.weight"), f(f"box_predictor.{k}.bbox_pred.bias"))
            assert ts[2].shape[0] == 2 and ts[4].shape[0] == 4, "one foreground class, class-agnostic box regression"
            keep.append(ts)
            for c, t in zip(cols, ts):
                c.append(t.data_ptr())
        arrs = [(C.c_void_p * K)(*c) for c in cols]
        pooled = int(round((keep[0][0].shape[1] // self.fpn_ch) ** 0.5))
        rw = (C.c_float * (4 * K))(*[float(v) for w in reg_weights for v in w])
        _chk(lib().ore_engine_set_roi_cascade(self._h, K, arrs[0], arrs[1], keep[0][0].shape[0], pooled, arrs[2], arrs[3], arrs[4], arrs[5], rw,
                                              score_thresh, nms_thresh, topk), "ore_engine_set_roi_cascade")
        self.has_roi = True
        self.roi_stages = K
        self._det_cap = min(max(int(topk), 1), 320)

    def detections(self, b: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(boxes [k,4], scores [k], source proposal index [k]) of the second stage for image b -- one sync to read the count."""
        k = int(self.buffer(f"det_count#{b}")[0, 0].item())
        return self.buffer(f"det_boxes#{b}")[:k], self.buffer(f"det_scores#{b}")[:k, 0], self.buffer(f"det_src#{b}")[:k, 0]

    def backbone(self, img: torch.Tensor) -> Dict[str, torch.Tensor]:
        """img [B,3,H,W] u8/f32 on device -> {'p3','p4','p5'} as logical NCHW views of engine-owned NHWC buffers."""
        assert img.is_cuda and img.is_contiguous()
        B, _, H, W = img.shape
        _chk(lib().ore_engine_backbone_fwd(self._h, img.data_ptr(), int(img.dtype == torch.uint8), B, H, W, _stream()),
             "ore_engine_backbone_fwd")
        Hp, Wp = (H + 31) // 32 * 32, (W + 31) // 32 * 32
        return {f"p{l}": self.buffer(f"p{l}", (B, Hp >> l, Wp >> l)) for l in (3, 4, 5)}

    def eval_forward(self, img: torch.Tensor, use_graph: bool = True) -> None:
        """img [3,H,W] u8/f32 on device.  Enqueues the whole path; results via .buffer()/.proposals()."""
        assert img.is_cuda and img.is_contiguous() and img.dim() == 3
        _, H, W = img.shape
        _chk(lib().ore_engine_eval_fwd(self._h, img.data_ptr(), int(img.dtype == torch.uint8), H, W, int(use_graph), _stream()),
             "ore_engine_eval_fwd")

    def detect_begin(self, img: torch.Tensor, out_h: int, out_w: int) -> torch.Tensor:
        """First half of `detect`: enqueue the pass (ore_engine_detect_begin) and return the result record it will fill.  Host work
        done before `detect_end` runs in the shadow of the device pass."""
        assert img.is_contiguous() and img.dim() == 3
        _, H, W = img.shape
        R = self.__dict__.get("_rec_rows") or self.__dict__.setdefault("_rec_rows", int(lib().ore_det_record_rows()))   # ORE_DET_RECORD_ROWS of the loaded library (= the engine's roi_cap)
        rec = torch.empty(R * 7, dtype=torch.float32, device=self.device)  # [R][4] f32 | [R] f32 | [R] i64, written by the last kernel
        _chk(lib().ore_engine_detect_begin(self._h, img.data_ptr(), int(img.dtype == torch.uint8), H, W, int(out_h), int(out_w),
                                           rec.data_ptr(), _stream()), "ore_engine_detect_begin")
        return rec

    def detect_classes_begin(self, img: torch.Tensor, out_h: int, out_w: int) -> torch.Tensor:
        """detect_begin for the N-way pass (ore_engine_detect_classes_begin); end it with detect_end."""
        assert img.is_contiguous() and img.dim() == 3
        _, H, W = img.shape
        R = self.__dict__.get("_rec_rows") or self.__dict__.setdefault("_rec_rows", int(lib().ore_det_record_rows()))
        rec = torch.empty(R * 7, dtype=torch.float32, device=self.device)
        _chk(lib().ore_engine_detect_classes_begin(self._h, img.data_ptr(), int(img.dtype == torch.uint8), H, W, int(out_h), int(out_w),
                                                   rec.data_ptr(), _stream()), "ore_engine_detect_classes_begin")
        return rec

    def detect_classes(self, img: torch.Tensor, out_h: int, out_w: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """`detect` over every class of set_classes() in ONE pass: per class both stages with that class's supports, then the merge
        (score descending, ties by class slot then row, top-k) and detector_postprocess.  Returns (boxes [n,4], scores [n], class ids [n])."""
        return self.detect_end(self.detect_classes_begin(img, out_h, out_w))

    def eval_classes_forward(self, img: torch.Tensor, use_graph: bool = True) -> None:
        """The N-way pass without a result record: class slot k's results are .proposals(k) / .detections(k) / .buffer("name#k"), the
        dense buffers read back as a K-image batch (block k = slot k)."""
        assert img.is_cuda and img.is_contiguous() and img.dim() == 3
        _, H, W = img.shape
        _chk(lib().ore_engine_eval_classes_fwd(self._h, img.data_ptr(), int(img.dtype == torch.uint8), H, W, int(use_graph), _stream()),
             "ore_engine_eval_classes_fwd")

    def detect_end(self, rec: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Second half: wait for the count (ore_engine_detect_end) and cut the record into (boxes [n,4], scores [n], classes [n] int64)."""
        n = C.c_int32(0)
        _chk(lib().ore_engine_detect_end(self._h, _stream(), C.byref(n)), "ore_engine_detect_end")
        k, R = n.value, self._rec_rows                                     # one strided view each: the protocol pays per torch call
        return rec.as_strided((k, 4), (4, 1)), rec.as_strided((k,), (1,), R * 4), rec.view(torch.int64).as_strided((k,), (1,), R * 5 // 2)

    def detect(self, img: torch.Tensor, out_h: int, out_w: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """The reference's eval call for one image, end to end (ore_engine_detect_begin + _end): image [3,H,W] u8/f32 on
        the device or on the host -> both stages + detector_postprocess as one hipGraph replay whose last kernel writes the results into
        a freshly allocated tensor, the count through a device-mapped pinned word the call polls.
        Returns (boxes [n,4], scores [n], classes [n] int64) -- the caller's own tensors, nothing of the engine aliases them."""
        return self.detect_end(self.detect_begin(img, out_h, out_w))

    def eval_forward_batch(self, imgs: torch.Tensor, use_graph: bool = True) -> None:
        """imgs [B,3,H,W] u8/f32 on device, B <= max_batch: dense stages batched, detection tail + second stage per image
        (ore_engine_eval_batch_fwd).  Image b's results: .proposals(b) / .detections(b) / .buffer("name#b")."""
        assert imgs.is_cuda and imgs.is_contiguous() and imgs.dim() == 4
        B, _, H, W = imgs.shape
        _chk(lib().ore_engine_eval_batch_fwd(self._h, imgs.data_ptr(), int(imgs.dtype == torch.uint8), B, H, W, int(use_graph), _stream()),
             "ore_engine_eval_batch_fwd")

    def last_flops(self) -> float:
        return float(lib().ore_engine_last_flops(self._h))

    def set_profiling(self, enable: bool) -> None:
        _chk(lib().ore_engine_set_profiling(self._h, int(enable)), "ore_engine_set_profiling")

    def read_profile(self) -> Tuple[float, float, int]:
        """(conv kernel ms, conv algorithmic FLOPs, conv launches) accumulated over eager forwards since the last read."""
        ms, fl, n = C.c_double(), C.c_double(), C.c_int32()
        _chk(lib().ore_engine_read_profile(self._h, C.byref(ms), C.byref(fl), C.byref(n)), "ore_engine_read_profile")
        return ms.value, fl.value, n.value

    def profile_executed_flops(self) -> float:
        """Of the FLOPs the last read_profile() reported, the multiplies actually executed (Winograd layers: algorithmic / 2.25)."""
        return float(lib().ore_engine_profile_executed_flops(self._h))

    def buffer(self, name: str, bhw: Optional[Tuple[int, int, int]] = None) -> torch.Tensor:
        """Zero-copy torch view of a named engine buffer.  With bhw=(B,H,W): logical NCHW view of the channel slice."""
        p = C.c_void_p()
        dims = (C.c_int64 * 4)()
        _chk(lib().ore_engine_buffer(self._h, name.encode(), C.byref(p), dims), f"ore_engine_buffer({name})")
        rows, ch, ld, coff = (int(x) for x in dims)
        dt = {"pre_loc": torch.int64, "keep_idx": torch.int64, "pre_level": torch.int32, "counts": torch.int32, "det_src": torch.int64,
              "det_count": torch.int32, "roi_ok": torch.int32,
              "final_classes": torch.int64}.get(name.split("#")[0], torch.float32)
        if lib().ore_engine_buffer_is_bf16(self._h, name.encode()):
            dt = torch.bfloat16                               # activation buffers of a bf16-storage engine
        flat = _from_ptr(p.value, rows * ld, dt, self.device)
        t = flat.view(rows, ld)[:, coff:coff + ch]
        if bhw is not None:
            B, H, W = bhw
            assert B * H * W == rows, (bhw, rows)
            t = t.reshape(B, H, W, ch) if coff == 0 and ch == ld else flat.view(B, H, W, ld)[..., coff:coff + ch]
            return t.permute(0, 3, 1, 2)
        return t

    def buffer_dims(self, name: str) -> Tuple[int, int, int, int, int]:
        """(device address, rows, channels, ld, coff) of a named engine buffer (ore_engine_buffer); host only.  The channel layout
        holds from finalize() on, the row count is the last pass's."""
        p, dims = C.c_void_p(), (C.c_int64 * 4)()
        _chk(lib().ore_engine_buffer(self._h, name.encode(), C.byref(p), dims), f"ore_engine_buffer({name})")
        return (p.value,) + tuple(int(x) for x in dims)

    def last_geometry(self) -> dict:
        """The geometry of the last pass (ore_engine_last_geometry): {"B", "H", "W", "levels": [(h, w, stride)] for p3 .. p5, "serial":
        the count of passes this engine has begun}."""
        g = (C.c_int32 * 16)()
        _chk(lib().ore_engine_last_geometry(self._h, g), "ore_engine_last_geometry")
        return {"B": g[0], "H": g[1], "W": g[2], "levels": [(g[3 + 3 * l], g[4 + 3 * l], g[5 + 3 * l]) for l in range(3)],
                "serial": int(g[12]) | (int(g[13]) << 31)}

    def heat_source(self, kind: str, slot: int = 0) -> "HeatSource":
        """What a heat map of the last pass reads (heat_kind lists the kinds): views of this engine's level buffers, the pass's geometry
        and its serial.  slot = the image of the batch -- the class slot of an N-way pass.  Pass the result to heatmap_draw /
        heatmap_levels before the engine begins another pass; afterwards they raise."""
        what = heat_kind(kind)
        geo = self.last_geometry()
        if geo["serial"] == 0:
            raise OreError("heat_source: this engine has not run a pass yet")
        if isinstance(slot, bool) or not isinstance(slot, (int, np.integer)) or not 0 <= int(slot) < geo["B"]:
            raise OreError(f"heat_source: slot {slot!r}: the last pass has {geo['B']} image(s) / class slot(s)")
        src = HeatSource.__new__(HeatSource)
        src.hw, src.strides, src.ptrs, src.ld, src.coff, src._keep = [], [], [], [], [], []
        chs, bf16 = set(), set()
        for name in what["buffers"]:
            h, w, s = geo["levels"][int(name[-1]) - 3]
            ptr, rows, ch, ld, coff = self.buffer_dims(name)
            if rows != geo["B"] * h * w:
                raise OreError(f"heat_source: buffer {name} has {rows} rows, the geometry says {geo['B']} x {h} x {w}")
            src.hw.append((h, w)); src.strides.append(s); src.ptrs.append(ptr); src.ld.append(ld); src.coff.append(coff)
            chs.add(ch)
            bf16.add(bool(lib().ore_engine_buffer_is_bf16(self._h, name.encode())))
        assert len(chs) == 1 and len(bf16) == 1, (chs, bf16)
        src.in_hw, src.batch, src.slot, src.ch, src.kind = (geo["H"], geo["W"]), geo["B"], int(slot), chs.pop(), kind
        src.device, src.is_bf16 = self.device, bf16.pop()
        src.engine, src.serial = self, geo["serial"]
        _heatmap_geometry(src.hw, src.strides, src.in_hw)
        src._set_what(what["channel"], what["transform"], what["norm"])
        return src

    def proposals(self, b: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(boxes [n,4], scores [n], keep_idx [n]) of image b -- reads the device-side count (one sync)."""
        n = int(self.buffer(f"counts#{b}")[1, 0].item())
        return self.buffer(f"out_boxes#{b}")[:n], self.buffer(f"out_scores#{b}")[:n, 0], self.buffer(f"keep_idx#{b}")[:n, 0]
