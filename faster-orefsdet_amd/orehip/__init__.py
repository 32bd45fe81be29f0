"""ctypes binding of libore_hip.so (include/ore_hip.h) -- the only way the Python host side reaches
the HIP kernels.  PyTorch is used for device memory (tensor.data_ptr()) and streams only.

There is NO CPU fallback: if the library is missing or a call fails, an exception is raised.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
import re
import subprocess
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(_PKG, "lib", "libore_hip.so")
CSRC = os.path.join(_PKG, "csrc")
HEADER = os.path.join(os.path.dirname(_PKG), "include", "ore_hip.h")
ESE_PARTS = 512


class OreError(RuntimeError):
    pass


def build(verbose: bool = False) -> str:
    """Compile libore_hip.so in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    out = subprocess.run(["make", "-C", CSRC, "-j8"], capture_output=True, text=True)
    if out.returncode != 0:
        raise OreError("building libore_hip.so failed:\n" + out.stdout[-4000:] + out.stderr[-4000:])
    if verbose:
        print(out.stdout[-2000:])
    return LIB_PATH


class ConvDesc(C.Structure):
    _fields_ = [("in_", C.c_void_p), ("in_ld", C.c_int32), ("in_coff", C.c_int32),
                ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("Cin", C.c_int32),
                ("w", C.c_void_p),
                ("Cout", C.c_int32), ("kh", C.c_int32), ("kw", C.c_int32), ("stride", C.c_int32), ("pad", C.c_int32),
                ("scale", C.c_void_p), ("shift", C.c_void_p), ("relu_cout", C.c_int32),
                ("in_mul", C.c_void_p), ("in_add", C.c_void_p), ("in_relu", C.c_int32),
                ("add", C.c_void_p), ("add_ld", C.c_int32), ("add_coff", C.c_int32),
                ("out", C.c_void_p), ("out_ld", C.c_int32), ("out_coff", C.c_int32),
                ("splitk", C.c_int32), ("workspace", C.c_void_p), ("workspace_floats", C.c_size_t), ("colsum", C.c_void_p),
                ("w_wino", C.c_void_p), ("storage", C.c_int32), ("w_wino_level_stride", C.c_int64), ("w_level_stride", C.c_int64)]


class ConvPlan(C.Structure):
    """ore_conv_plan_t: the kernel, build, split-K and grid of one conv call (ore_conv_plan)."""
    _fields_ = [("launcher", C.c_int32), ("error", C.c_int32), ("bm", C.c_int32), ("bn", C.c_int32), ("build", C.c_int32 * 4),
                ("splitk", C.c_int32), ("steps_per_split", C.c_int32), ("xmap", C.c_int32), ("gx", C.c_int32), ("gy", C.c_int32)]

    def astuple(self) -> Tuple[int, ...]:
        return (self.launcher, self.bm, self.bn, *self.build, self.splitk, self.steps_per_split, self.xmap, self.gx, self.gy)


class DetectDesc(C.Structure):
    _fields_ = [("n_levels", C.c_int32), ("head", C.c_void_p * 8), ("head_ld", C.c_int32),
                ("H", C.c_int32 * 8), ("W", C.c_int32 * 8), ("stride", C.c_int32 * 8),
                ("score_thresh", C.c_float), ("pre_topk", C.c_int32), ("nms_thresh", C.c_float), ("post_topk", C.c_int32),
                ("pre_boxes", C.c_void_p), ("pre_scores", C.c_void_p), ("pre_loc", C.c_void_p), ("pre_level", C.c_void_p),
                ("keep_idx", C.c_void_p), ("counts", C.c_void_p), ("out_boxes", C.c_void_p), ("out_scores", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t)]


class ModelCfg(C.Structure):
    _fields_ = [("stem_ch", C.c_int32 * 3), ("stage_conv_ch", C.c_int32 * 4), ("stage_out_ch", C.c_int32 * 4),
                ("layers_per_block", C.c_int32), ("fpn_ch", C.c_int32), ("strides", C.c_int32 * 3),
                ("pixel_mean", C.c_float * 3), ("pixel_std", C.c_float * 3),
                ("score_thresh", C.c_float), ("pre_topk", C.c_int32), ("nms_thresh", C.c_float), ("post_topk", C.c_int32),
                ("max_batch", C.c_int32), ("max_h", C.c_int32), ("max_w", C.c_int32)]


# The C-ABI's parameter and return types.  Every pointer (T*, T* const*, T a[n], struct and handle pointers) is a c_void_p, which takes
# an int address, None, bytes, a ctypes array, byref() or a c_void_p.
_PARAM_TYPES = {"int32_t": C.c_int32, "int64_t": C.c_int64, "size_t": C.c_size_t, "float": C.c_float}
_RESULT_TYPES = {"int": C.c_int, "int32_t": C.c_int32, "size_t": C.c_size_t, "double": C.c_double, "const char*": C.c_char_p,
                 "void": None}


def _prototypes(path: str) -> Dict[str, Tuple[Optional[type], List[type]]]:
    """{name: (restype, argtypes)} of every `ret ore_name(params);` the header declares, in its order.  A type outside the tables
    above is an error: no function of the library is called untyped."""
    with open(path) as f:
        src = re.sub(r"/\*.*?\*/|//[^\n]*", " ", f.read(), flags=re.S)
    src = re.sub(r"^\s*#[^\n]*", " ", src, flags=re.M)
    protos = {}
    for stmt in re.split(r"[;{}]", src):
        m = re.fullmatch(r"\s*(.+?)\s*\b(ore_\w+)\s*\((.*)\)\s*", stmt, flags=re.S)
        if m is None:
            continue
        ret, name, params = " ".join(m[1].split()).replace(" *", "*"), m[2], " ".join(m[3].split())
        if ret not in _RESULT_TYPES:
            raise OreError(f"{path}: {name}: no ctypes type for the return type '{ret}'")
        args = []
        for p in ([] if params == "void" else params.split(",")):
            scalar = re.fullmatch(r"\s*(?:const\s+)?(\w+)\s+\w+\s*", p)
            if "*" in p or "[" in p:
                args.append(C.c_void_p)
            elif scalar is not None and scalar[1] in _PARAM_TYPES:
                args.append(_PARAM_TYPES[scalar[1]])
            else:
                raise OreError(f"{path}: {name}: no ctypes type for the parameter '{p.strip()}'")
        protos[name] = (_RESULT_TYPES[ret], args)
    return protos


_PROTOTYPES = _prototypes(HEADER)
SYMBOLS = tuple(_PROTOTYPES)          # every function include/ore_hip.h declares
_lib = None


def lib() -> C.CDLL:
    """libore_hip.so with argtypes / restype of every function set from the header's prototypes."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OreError(f"{LIB_PATH} not found: build it with `make -C {CSRC}` (there is no CPU fallback)")
        L = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in _PROTOTYPES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = L
    return _lib


def _chk(rc: int, what: str):
    if rc != 0:
        raise OreError(f"{what} failed ({rc}): {lib().ore_last_error().decode()}")


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream() -> int:
    """The current torch stream of the current device as a hipStream_t (the raw-handle query is ~10x cheaper than building a
    torch.cuda.Stream object per launch; thousands of launches per training step go through here)."""
    if _RAW_STREAM is not None:
        return _RAW_STREAM(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    if t is None:
        return None
    assert t.is_cuda, "libore_hip.so works on device memory only"
    return t.data_ptr()


def _f32(t: torch.Tensor) -> torch.Tensor:
    assert t.dtype == torch.float32 and t.is_contiguous(), (t.dtype, t.is_contiguous())
    return t


def _i32s(seq) -> C.Array:
    """The values as a host int32_t array (per-level sizes and strides)."""
    v = list(seq)
    return (C.c_int32 * len(v))(*v)


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


ROI_BWD_DETERMINISTIC = True          # False: the fp32-atomics form of rounds 1-4 (order-dependent in the last bits; A/B aid)
ROI_BWD_MODE = "tiled"                # the deterministic form: "tiled" (gather, one block per map tile, no atomics) | "fixed" (64-bit fixed-point atomics)


def roi_align_bwd(dout: torch.Tensor, feats_like: Sequence[torch.Tensor], boxes: torch.Tensor, strides=(8, 16, 32), min_level: int = 3,
                  pooled: int = 8, dfeats: Optional[Sequence[torch.Tensor]] = None, box_image: Optional[torch.Tensor] = None) -> List[torch.Tensor]:
    """dout [n, pooled*pooled*C]; returns/accumulates into per-level gradient buffers shaped like feats_like ([H,W,ld] NHWC)."""
    L = len(feats_like)
    n = boxes.shape[0]
    tiled = ROI_BWD_DETERMINISTIC and ROI_BWD_MODE == "tiled" and pooled <= 16
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
    if ROI_BWD_DETERMINISTIC and (n > n_img or box_image is None and n > 1):
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


def to_device(t: torch.Tensor, dev) -> torch.Tensor:
    """Host tensor -> device without a blocking pageable copy (a pageable hipMemcpy drains the stream first: one hidden host sync per
    small upload): staged through torch's cached pinned allocator and issued asynchronously.  Device tensors pass through."""
    dev = torch.device(dev)
    if t.is_cuda:
        return t if t.device == dev or dev.index is None else t.to(dev)
    if dev.type != "cuda":
        return t.to(dev)
    return t.pin_memory().to(dev, non_blocking=True)


# ---------------------------------------------------------------------------------------------------
# image resize: Pillow's Image.resize(size, BILINEAR) on the device (csrc/ore_resize.hip, csrc/ore_resize_plan.cpp)
# ---------------------------------------------------------------------------------------------------
RESIZE_FORM_LDS, RESIZE_FORM_WORKSPACE = 1, 2            # ORE_RESIZE_FORM_* (include/ore_hip.h)


def resize_shortest_edge_shape(h: int, w: int, size: int, max_size: int) -> Tuple[int, int]:
    """(nh, nw) of detectron2 v0.5's ResizeShortestEdge.get_transform (d2z:data/transforms/augmentation_impl.py): the short side
    scaled to `size`, everything rescaled when the long side then exceeds `max_size`, int(x + 0.5) at the end -- the arithmetic of
    DatasetMapperWithSupport._resize_flip."""
    scale = size * 1.0 / min(h, w)
    nh, nw = (size, scale * w) if h < w else (scale * h, size)
    if max(nh, nw) > max_size:
        s2 = max_size * 1.0 / max(nh, nw)
        nh, nw = nh * s2, nw * s2
    return int(nh + 0.5), int(nw + 0.5)


def resize_plan(n_in: int, n_out: int) -> Tuple[np.ndarray, np.ndarray]:
    """One axis of the resample (ore_resize_plan, host only): bounds [n_out, 2] int32 = (first source index, count) and coeffs
    [n_out, ksize] int32, Pillow's 22-bit fixed-point weights.  A pixel is clip8((2^21 + sum(src * coeff)) >> 22)."""
    ks = int(lib().ore_resize_ksize(int(n_in), int(n_out)))
    if ks <= 0:
        raise OreError(f"resize_plan: sizes {n_in} -> {n_out} outside [1, 8192]")
    bounds, coeffs = np.empty((n_out, 2), dtype=np.int32), np.empty((n_out, ks), dtype=np.int32)
    _chk(lib().ore_resize_plan(int(n_in), int(n_out), bounds.ctypes.data, coeffs.ctypes.data, None), "ore_resize_plan")
    return bounds, coeffs


def resize_form(h: int, w: int, nh: int, nw: int) -> int:
    """The form resize_bilinear_u8 takes for this size pair: RESIZE_FORM_LDS (one launch) or RESIZE_FORM_WORKSPACE (two)."""
    return int(lib().ore_resize_form(int(h), int(w), int(nh), int(nw)))


_RESIZE_TABLES: Dict[tuple, torch.Tensor] = {}
_RESIZE_TABLES_MAX = 32
_RESIZE_WS: Dict[tuple, torch.Tensor] = {}


def _table_uploaded(tab: torch.Tensor, cur: int) -> None:
    """Mark a cached device table as uploaded just now, asynchronously, on the current stream `cur`: the event behind the copy is
    what a use on another stream has to wait for."""
    tab._ore_stream, tab._ore_event, tab._ore_arrived = cur, torch.cuda.Event(), False
    tab._ore_event.record(torch.cuda.current_stream(tab.device))


def _table_on_stream(tab: torch.Tensor, cur: int) -> None:
    """Make a cached table safe to read from work enqueued next on the current stream `cur`.  On the stream that uploaded it, stream
    order is enough.  Another stream is made to wait for the upload's event until that event is seen complete (the wait is enqueued
    on the device; the host does not block), and the table is marked as used there so that an eviction does not free it early."""
    if tab._ore_stream == cur:
        return
    stream = torch.cuda.current_stream(tab.device)
    if not tab._ore_arrived:
        tab._ore_arrived = tab._ore_event.query()
        if not tab._ore_arrived:
            stream.wait_event(tab._ore_event)
    tab.record_stream(stream)


def _resize_tables(dev, h: int, w: int, nh: int, nw: int) -> torch.Tensor:
    """The device tables of one size pair, cached.  A new table is planned on the host into pinned memory and copied behind the
    current stream's work, so the launch that follows on that stream reads it complete.  The cache is bounded: the oldest table
    leaves when a new one would be the 33rd.  Nothing here is captured in a graph, so a launch that still reads an evicted table is
    protected by stream order alone: torch's allocator hands the block to later work of the stream it was allocated on, and a table
    used on another stream is marked for that stream (record_stream) at that use.  A use on another stream than the uploading one
    first waits, on the device, for the event behind the upload (_table_on_stream)."""
    key = (str(dev), h, w, nh, nw)
    tab = _RESIZE_TABLES.get(key)
    cur = _stream()
    if tab is None:
        n = int(lib().ore_resize_table_ints(h, w, nh, nw))
        if n <= 0:
            raise OreError(f"resize_bilinear_u8: {h}x{w} -> {nh}x{nw}: sides must be in [1, 8192]")
        host = torch.empty(n, dtype=torch.int32, pin_memory=True)
        _chk(lib().ore_resize_tables_host(h, w, nh, nw, host.data_ptr()), "ore_resize_tables_host")
        while len(_RESIZE_TABLES) >= _RESIZE_TABLES_MAX:
            _RESIZE_TABLES.pop(next(iter(_RESIZE_TABLES)))
        tab = _RESIZE_TABLES[key] = host.to(dev, non_blocking=True)
        _table_uploaded(tab, cur)
    else:
        _table_on_stream(tab, cur)
    return tab


def resize_bilinear_u8(img_hwc_u8: torch.Tensor, nh: int, nw: int, swap_rb: bool = False, out: Optional[torch.Tensor] = None,
                       stream: Optional["torch.cuda.Stream"] = None, form: int = 0) -> torch.Tensor:
    """[h, w, 3] uint8 device tensor (interleaved, what an image reader gives) -> [3, nh, nw] uint8 planar, byte for byte
    np.asarray(Image.fromarray(img).resize((nw, nh), Image.BILINEAR)).transpose(2, 0, 1); swap_rb exchanges channels 0 and 2.
    form: 0 = the library's choice (resize_form), or RESIZE_FORM_LDS / RESIZE_FORM_WORKSPACE to force one."""
    if stream is not None:
        with torch.cuda.stream(stream):
            return resize_bilinear_u8(img_hwc_u8, nh, nw, swap_rb, out, None, form)
    assert img_hwc_u8.is_cuda and img_hwc_u8.dtype == torch.uint8 and img_hwc_u8.dim() == 3 and img_hwc_u8.shape[2] == 3 and \
        img_hwc_u8.is_contiguous(), "resize_bilinear_u8 takes a contiguous [h, w, 3] uint8 device tensor"
    h, w = int(img_hwc_u8.shape[0]), int(img_hwc_u8.shape[1])
    nh, nw = int(nh), int(nw)
    dev = img_hwc_u8.device
    with torch.cuda.device(dev):
        tab = _resize_tables(dev, h, w, nh, nw)
        if out is None:
            out = torch.empty(3, nh, nw, dtype=torch.uint8, device=dev)
        assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (3, nh, nw) and out.is_contiguous()
        ws, ws_bytes = None, 0
        if form == RESIZE_FORM_WORKSPACE or (form == 0 and resize_form(h, w, nh, nw) == RESIZE_FORM_WORKSPACE):
            ws_bytes = int(lib().ore_resize_workspace_bytes(h, w, nh, nw))
            ws_key = (str(dev), _stream())                          # per stream: two streams' passes must not share an intermediate
            ws = _RESIZE_WS.get(ws_key)
            if ws is None or ws.numel() < ws_bytes:
                ws = _RESIZE_WS[ws_key] = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        _chk(lib().ore_resize_bilinear_u8_fwd(_ptr(img_hwc_u8), h, w, _ptr(out), nh, nw, int(bool(swap_rb)), _ptr(tab), int(form), _ptr(ws),
                                              ws_bytes, _stream()), "ore_resize_bilinear_u8_fwd")
    return out


# ---------------------------------------------------------------------------------------------------
# support crops: annotated frames -> the S x S crops and support boxes of a support set (csrc/ore_support.hip, csrc/ore_support_plan.cpp)
# ---------------------------------------------------------------------------------------------------
SUPPORT_JOB_INTS = 32                                    # ORE_SUPPORT_JOB_INTS; the record's words are ORE_SJ_* (include/ore_hip.h)
SUPPORT_FILL = (104, 116, 124)                           # round(cfg.MODEL.PIXEL_MEAN): padding normalises to about 0
_SJ_H, _SJ_RECT, _SJ_DST, _SJ_XB, _SJ_YB, _SJ_KX, _SJ_KY, _SJ_KSX, _SJ_KSY, _SJ_FORM, _SJ_D, _SJ_X0, _SJ_BOX = 2, 4, 8, 12, 13, 14, 15, 16, 17, 18, 24, 25, 27
_SUPPORT_BUF: Dict[tuple, dict] = {}                     # (device, stream) -> pinned job buffers with their uploads' events, the device copy, the workspace


def _support_box(box) -> np.ndarray:
    b = np.ascontiguousarray(np.asarray(box, dtype=np.float32).reshape(4))
    return b


def _support_refused(h, w, box, size, context, index=None) -> ValueError:
    which = "box" if index is None else f"box {index}"
    return ValueError(f"support crop: {which} {[float(v) for v in box]} lies outside its {h}x{w} frame, or a size is out of range "
                      f"(frame sides 1 .. 8192, 2 * context {context} < size {size} <= 8192)")


def support_crop_form(h: int, w: int, box, size: int = 240, context: int = 16) -> int:
    """The form the crop of this box takes (ore_support_crop_form): RESIZE_FORM_LDS (served by the one launch that covers every such
    job of a call) or RESIZE_FORM_WORKSPACE (a horizontal and a vertical launch through a workspace slice)."""
    b = _support_box(box)
    form = int(lib().ore_support_crop_form(int(h), int(w), b.ctypes.data, int(size), int(context)))
    if form == 0:
        raise _support_refused(h, w, b, size, context)
    return form


def support_crop_plan(h: int, w: int, box, size: int = 240, context: int = 16) -> dict:
    """The plan of one support crop (ore_support_crop_plan, host only; the contract is "support crop v1" of include/ore_hip.h):
    {"D", "origin" (x0, y0), "src" (rx0, ry0, rx1, ry1), "dst" (dx0, dy0, dx1, dy1), "box" float32 [4] inside the crop, "form",
    "workspace_bytes", and the job's resample tables "x_bounds" [nw, 2], "x_coeffs" [nw, ksx], "y_bounds" [nh, 2], "y_coeffs" [nh, ksy]}."""
    L = lib()
    h, w, size, context = int(h), int(w), int(size), int(context)
    b = _support_box(box)
    n = int(L.ore_support_crop_job_ints(h, w, b.ctypes.data, size, context))
    if n == 0:
        raise _support_refused(h, w, b, size, context)
    buf = np.zeros(SUPPORT_JOB_INTS + n, dtype=np.int32)
    _chk(L.ore_support_crop_plan(h, w, b.ctypes.data, size, context, None, SUPPORT_JOB_INTS, 0, buf.ctypes.data, buf.ctypes.data),
         "ore_support_crop_plan")
    r = buf[:SUPPORT_JOB_INTS]
    src, dst = tuple(int(v) for v in r[_SJ_RECT:_SJ_RECT + 4]), tuple(int(v) for v in r[_SJ_DST:_SJ_DST + 4])
    nw, nh, ksx, ksy = dst[2] - dst[0], dst[3] - dst[1], int(r[_SJ_KSX]), int(r[_SJ_KSY])
    return {"D": int(r[_SJ_D]), "origin": (int(r[_SJ_X0]), int(r[_SJ_X0 + 1])), "src": src, "dst": dst,
            "box": r[_SJ_BOX:_SJ_BOX + 4].view(np.float32).copy(), "form": int(r[_SJ_FORM]),
            "workspace_bytes": int(L.ore_support_crop_workspace_bytes(h, w, b.ctypes.data, size, context)),
            "x_bounds": buf[r[_SJ_XB]:r[_SJ_XB] + nw * 2].reshape(nw, 2).copy(), "x_coeffs": buf[r[_SJ_KX]:r[_SJ_KX] + nw * ksx].reshape(nw, ksx).copy(),
            "y_bounds": buf[r[_SJ_YB]:r[_SJ_YB] + nh * 2].reshape(nh, 2).copy(), "y_coeffs": buf[r[_SJ_KY]:r[_SJ_KY] + nh * ksy].reshape(nh, ksy).copy()}


def support_crops(frames, boxes, frame_index=None, size: int = 240, context: int = 16, fill=SUPPORT_FILL,
                  out: Optional[torch.Tensor] = None, device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Support crops of K boxes ("support crop v1", include/ore_hip.h).  frames: one [h, w, 3] uint8 tensor / array or a list of them
    (sizes may differ; a host frame is uploaded once through pinned memory), boxes [K, 4] XYXY absolute, frame_index [K] (default: all
    0).  Returns (crops [K, 3, size, size] uint8 on the device, planar, the frames' channel order; support boxes [K, 4] float32 on the
    host).  All K jobs are planned on the host into one pinned buffer, uploaded with one copy, and run by at most three launches on
    the current stream; the host does not wait for the device: a pinned buffer is written again only once the upload that read it
    is seen complete (an event query), and while none is free another one is added.  The buffers are cached per (device, stream)
    and do not touch the resize tables' cache.  A box outside its frame: ValueError naming its index."""
    L = lib()
    size, context = int(size), int(context)
    if torch.is_tensor(frames) or isinstance(frames, np.ndarray):
        frames = [frames]
    frames = [torch.from_numpy(np.ascontiguousarray(f)) if isinstance(f, np.ndarray) else f for f in frames]
    if device is None:
        device = next((f.device for f in frames if f.is_cuda), None) or torch.device("cuda", torch.cuda.current_device())
    dev = torch.device(device)
    bx = np.ascontiguousarray(torch.as_tensor(boxes).detach().cpu().numpy() if torch.is_tensor(boxes) else np.asarray(boxes), dtype=np.float32).reshape(-1, 4)
    K = len(bx)
    fi = np.zeros(K, dtype=np.int64) if frame_index is None else np.asarray(torch.as_tensor(frame_index).cpu().numpy(), dtype=np.int64).reshape(-1)
    if K < 1 or len(fi) != K or (fi < 0).any() or (fi >= len(frames)).any():
        raise ValueError(f"support_crops: {K} boxes, {len(fi)} frame indices into {len(frames)} frames")
    fill = tuple(int(v) for v in fill)
    if len(fill) != 3 or min(fill) < 0 or max(fill) > 255:
        raise ValueError(f"support_crops: fill must be three bytes, not {fill}")
    for f in frames:
        if f.dtype != torch.uint8 or f.dim() != 3 or f.shape[2] != 3:
            raise ValueError(f"support_crops takes [h, w, 3] uint8 frames, not {tuple(f.shape)} {f.dtype}")
    with torch.cuda.device(dev):
        used = sorted(set(int(i) for i in fi))
        on_dev = {i: (frames[i] if frames[i].is_cuda else frames[i].contiguous().pin_memory().to(dev, non_blocking=True)).contiguous() for i in used}
        # sizes first: table words and workspace slice of every job
        n_tab, n_ws = [], []
        for k in range(K):
            h, w = int(frames[fi[k]].shape[0]), int(frames[fi[k]].shape[1])
            n = int(L.ore_support_crop_job_ints(h, w, bx[k].ctypes.data, size, context))
            if n == 0:
                raise _support_refused(h, w, bx[k], size, context, k)
            n_tab.append(n)
            n_ws.append(int(L.ore_support_crop_workspace_bytes(h, w, bx[k].ctypes.data, size, context)))
        total, ws_bytes = K * SUPPORT_JOB_INTS + sum(n_tab), sum(n_ws)
        cur = _stream()
        st = _SUPPORT_BUF.setdefault((str(dev), cur), {"pinned": [], "dev": None, "ws": None})
        # a pinned buffer whose last upload has completed (queried, not waited for); a backlog on the stream adds a buffer instead
        slot = next((p for p in st["pinned"] if p["host"].numel() >= total and (p["event"] is None or p["event"].query())), None)
        if slot is None:
            st["pinned"] = [p for p in st["pinned"] if p["host"].numel() >= total or not (p["event"] is None or p["event"].query())]     # outgrown and idle: dropped
            slot = {"host": torch.empty(total, dtype=torch.int32, pin_memory=True), "event": None}
            st["pinned"].append(slot)
        if st["dev"] is None or st["dev"].numel() < total:
            st["dev"] = torch.empty(total, dtype=torch.int32, device=dev)
        if ws_bytes and (st["ws"] is None or st["ws"].numel() < ws_bytes):
            st["ws"] = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        st["last"] = slot                                                      # the latest call's plan (tools/bench_support.py replays it)
        host, base = slot["host"], slot["host"].data_ptr()
        t_off, w_off = K * SUPPORT_JOB_INTS, 0
        for k in range(K):
            f = on_dev[int(fi[k])]
            _chk(L.ore_support_crop_plan(int(f.shape[0]), int(f.shape[1]), bx[k].ctypes.data, size, context, f.data_ptr(), t_off, w_off,
                                         base + 4 * k * SUPPORT_JOB_INTS, base), "ore_support_crop_plan")
            t_off += n_tab[k]
            w_off += n_ws[k]
        st["dev"][:total].copy_(host[:total], non_blocking=True)               # the call's one upload
        slot["event"] = torch.cuda.Event()
        slot["event"].record(torch.cuda.current_stream(dev))
        if out is None:
            out = torch.empty(K, 3, size, size, dtype=torch.uint8, device=dev)
        assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (K, 3, size, size) and out.is_contiguous()
        _chk(L.ore_support_crop_u8_fwd(_ptr(st["dev"]), base, total, K, size, fill[0] | fill[1] << 8 | fill[2] << 16, _ptr(out),
                                       _ptr(st["ws"]) if ws_bytes else None, ws_bytes, cur), "ore_support_crop_u8_fwd")
        rec = host[:K * SUPPORT_JOB_INTS].view(K, SUPPORT_JOB_INTS)
        sboxes = rec[:, _SJ_BOX:_SJ_BOX + 4].contiguous().view(torch.float32).clone()
    return out, sboxes


# ---------------------------------------------------------------------------------------------------
# batch canvases of a training step ("batch canvas v1", include/ore_hip.h; csrc/ore_batch_canvas.hip)
# ---------------------------------------------------------------------------------------------------
BATCH_CANVAS_JOB_INTS = 8                                # ORE_BATCH_CANVAS_JOB_INTS
_BCJ_SRC, _BCJ_H, _BCJ_W, _BCJ_DST, _BCJ_HC, _BCJ_WC = 0, 2, 3, 4, 6, 7


class BatchCanvasGeom(tuple):
    """What of a batch-canvas plan is a launch argument -- and therefore fixed in a captured launch: (n_query, (Hq, Wq), query_u8,
    n_support, (Hs, Ws), support_u8, table_bytes, slab_bytes).  Two plans with equal geometry are served by the same launch."""
    __slots__ = ()
    n_query = property(lambda s: s[0])
    q_canvas = property(lambda s: s[1])
    q_u8 = property(lambda s: s[2])
    n_support = property(lambda s: s[3])
    s_canvas = property(lambda s: s[4])
    s_u8 = property(lambda s: s[5])
    table_bytes = property(lambda s: s[6])
    slab_bytes = property(lambda s: s[7])

    @property
    def out_floats(self) -> int:
        return self.n_query * 3 * self.q_canvas[0] * self.q_canvas[1] + self.n_support * 3 * self.s_canvas[0] * self.s_canvas[1]


class BatchCanvasPlan:
    """One step's raw images packed for ore_batch_canvas_fwd: `host` = ONE pinned uint8 buffer [table | slab] (the table: one row of
    BATCH_CANVAS_JOB_INTS int32 words per job, query rows first; the slab: every image planar at its own size, each at a 16-byte
    boundary), `used` = the bytes of it that a step has to upload, `table` = the rows as an int32 [jobs, 8] view of the buffer,
    `geom` = the launch's fixed arguments."""

    def __init__(self, host, used, table, geom):
        self.host, self.used, self.table, self.geom = host, int(used), table, geom


def _canvas_group(images, what: str):
    """A group's images as a flat list of [3, h, w] host tensors of one dtype (a [N, 3, h, w] tensor counts as N images), and the
    tensors as given, each with the index of its first image: [(first, [n, 3, h, w])]."""
    flat, blocks = [], []
    for t in images:
        t = torch.as_tensor(t)
        if t.is_cuda:
            raise ValueError(f"batch_canvas_plan packs host images; a {what} image lives on {t.device}")
        blocks.append((len(flat), t if t.dim() == 4 else t[None]))
        if t.dim() == 4:
            flat.extend(t[i] for i in range(t.shape[0]))
        else:
            flat.append(t)
    for t in flat:
        if t.dim() != 3 or t.shape[0] != 3 or t.shape[1] < 1 or t.shape[2] < 1:
            raise ValueError(f"batch_canvas_plan takes [3, h, w] images, not a {what} image of shape {tuple(t.shape)}")
        if t.dtype not in (torch.uint8, torch.float32):
            raise ValueError(f"batch_canvas_plan takes raw uint8 or fp32 images, not a {what} image of {t.dtype}")
        if t.dtype != flat[0].dtype:
            raise ValueError(f"batch_canvas_plan: the {what} images mix {flat[0].dtype} and {t.dtype}; one dtype per group")
    return flat, blocks


def batch_canvas_plan(queries, supports=(), div: int = 32, q_canvas: Optional[Tuple[int, int]] = None,
                      s_canvas: Optional[Tuple[int, int]] = None, capacity: Optional[Tuple[int, int]] = None,
                      full_slab: bool = False) -> BatchCanvasPlan:
    """Host plan of one step's batch canvases: the query images (a list of [3, h, w] host tensors, sizes may differ) and the support
    crops (a list of [3, h, w] or [N, 3, h, w] host tensors) packed into one pinned buffer, table and slab together, so that ONE
    host-to-device copy per step replaces one upload per image.  A group's canvas is its largest height and width rounded up to `div`
    (ImageList.from_tensors), or `q_canvas` / `s_canvas` as given.  `capacity` = (query jobs, support jobs) of the launch (default: the
    images given); rows beyond the images given are empty jobs, whose canvases come out all zero.  `full_slab`: the slab is sized for
    images that fill their canvases -- the geometry, and with it the launch, then depends on nothing but the canvases, the capacities
    and the dtypes (a captured launch).  ValueError: an image larger than its canvas, two dtypes within a group, more images than the
    capacity, an image on the device."""
    both = [_canvas_group(queries, "query"), _canvas_group(supports, "support")]
    groups, blocks = [b[0] for b in both], [b[1] for b in both]
    cap =[len(groups[0]), len(groups[1])] if capacity is None else [int(capacity[0]), int(capacity[1])]
    canv, u8 = [], []
    for g, (imgs, given, what) in enumerate(zip(groups, (q_canvas, s_canvas), ("query", "support"))):
        if len(imgs) > cap[g]:
            raise ValueError(f"batch_canvas_plan: {len(imgs)} {what} images, the capacity is {cap[g]}")
        if given is not None:
            Hc, Wc = int(given[0]), int(given[1])
        elif imgs:
            Hc, Wc = (-(-max(int(t.shape[d]) for t in imgs) // div) * div for d in (1, 2))
        else:
            Hc, Wc = 0, 0
        for i, t in enumerate(imgs):
            if t.shape[1] > Hc or t.shape[2] > Wc:
                raise ValueError(f"batch_canvas_plan: {what} image {i} of {t.shape[1]} x {t.shape[2]} is larger than its {Hc} x {Wc} canvas")
        if cap[g] and (Hc < 1 or Wc < 4 or Wc % 4 or max(Hc, Wc) > 8192):
            raise ValueError(f"batch_canvas_plan: {what} canvas {Hc} x {Wc} (sides 1 .. 8192, the width a multiple of 4)")
        canv.append((Hc, Wc))
        u8.append(bool(imgs[0].dtype == torch.uint8) if imgs else True)
    if cap[0] + cap[1] < 1 or cap[0] + cap[1] > 65535:
        raise ValueError(f"batch_canvas_plan: {cap[0]} + {cap[1]} jobs (1 .. 65535 in all)")
    up16 = lambda n: (n + 15) // 16 * 16                 # noqa: E731
    esz = [1 if u else 4 for u in u8]
    table_bytes = up16((cap[0] + cap[1]) * BATCH_CANVAS_JOB_INTS * 4)
    packed = sum(up16(3 * int(t.shape[1]) * int(t.shape[2]) * esz[g]) for g in range(2) for t in groups[g])
    slab_bytes = sum(cap[g] * up16(3 * canv[g][0] * canv[g][1] * esz[g]) for g in range(2)) if full_slab else max(packed, 16)
    geom = BatchCanvasGeom((cap[0], canv[0], u8[0], cap[1], canv[1], u8[1], table_bytes, slab_bytes))
    host = torch.empty(table_bytes + slab_bytes, dtype=torch.uint8, pin_memory=torch.cuda.is_available())
    table = host[:(cap[0] + cap[1]) * BATCH_CANVAS_JOB_INTS * 4].view(torch.int32).view(cap[0] + cap[1], BATCH_CANVAS_JOB_INTS)
    jobs = cap[0] + cap[1]
    rows = np.zeros((jobs, BATCH_CANVAS_JOB_INTS), dtype=np.int64)
    first = (0, cap[0])
    for g in range(2):
        j0, n = first[g], len(groups[g])
        rows[j0:j0 + n, _BCJ_H] = [int(t.shape[1]) for t in groups[g]]
        rows[j0:j0 + n, _BCJ_W] = [int(t.shape[2]) for t in groups[g]]
        rows[j0:j0 + cap[g], _BCJ_HC], rows[j0:j0 + cap[g], _BCJ_WC] = canv[g]
        rows[j0:j0 + cap[g], _BCJ_DST] = (first[g] and cap[0] * 3 * canv[0][0] * canv[0][1]) + np.arange(cap[g]) * (3 * canv[g][0] * canv[g][1])
    nbytes = 3 * rows[:, _BCJ_H] * rows[:, _BCJ_W] * np.repeat(esz, cap)
    src = np.concatenate([[0], np.cumsum((nbytes + 15) // 16 * 16)])                     # every image at a 16-byte boundary
    rows[:, _BCJ_SRC] = src[:-1]
    for at in (_BCJ_SRC, _BCJ_DST):
        rows[:, at + 1], rows[:, at] = rows[:, at] >> 32, rows[:, at] & 0xffffffff
    table.copy_(torch.from_numpy(rows.astype(np.uint32).view(np.int32)))
    for g in range(2):
        for i0, t in blocks[g]:                                                           # a tensor of crops whose images tile the slab: one copy
            n, j = int(t.shape[0]), first[g] + i0
            nb = int(nbytes[j])
            for k in ([None] if nb % 16 == 0 or n == 1 else range(n)):
                a = table_bytes + int(src[j + (k or 0)])
                piece = host[a:a + (n if k is None else 1) * nb]
                piece = (piece if u8[g] else piece.view(torch.float32)).view(-1, *t.shape[1:])
                piece.copy_(t if k is None else t[k:k + 1])
    return BatchCanvasPlan(host, table_bytes + int(src[-1]), table, geom)


def batch_canvas(buf: torch.Tensor, geom: BatchCanvasGeom, pixel_mean: torch.Tensor, pixel_std: torch.Tensor,
                 out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The query and the support canvas of a step from ONE launch (ore_batch_canvas_fwd): buf = the device copy of a BatchCanvasPlan's
    buffer (`plan.host[:plan.used]` at its start; a buffer of a captured launch is written again before every replay), geom = the
    plan's geometry, pixel_mean / pixel_std = the model's buffers on the device.  Returns (xq [n_query, 3, Hq, Wq], xs [n_support, 3, Hs,
    Ws]) fp32, both views of `out` (allocated if not given): (float(raw) - mean) / std inside every image, +0.0 in the padding -- the
    tensors the mixed-size branch of train_forward.train_core builds with a handful of torch ops per image."""
    assert buf.is_cuda and buf.dtype == torch.uint8 and buf.is_contiguous() and buf.numel() >= geom.table_bytes + geom.slab_bytes, \
        "batch_canvas: buf is the uint8 device buffer [table | slab] of the plan's geometry"
    mean, std = _f32(pixel_mean.reshape(-1)), _f32(pixel_std.reshape(-1))
    assert mean.numel() == 3 and std.numel() == 3 and mean.device == buf.device and std.device == buf.device
    n = geom.out_floats
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=buf.device)
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= n
    with torch.cuda.device(buf.device):
        _chk(lib().ore_batch_canvas_fwd(buf.data_ptr() + geom.table_bytes, geom.slab_bytes, _ptr(buf), geom.n_query, geom.q_canvas[0],
                                        geom.q_canvas[1], int(geom.q_u8), geom.n_support, geom.s_canvas[0], geom.s_canvas[1], int(geom.s_u8),
                                        _ptr(mean), _ptr(std), _ptr(out), out.numel(), _stream()), "ore_batch_canvas_fwd")
    flat = out.view(-1)
    nq = geom.n_query * 3 * geom.q_canvas[0] * geom.q_canvas[1]
    return (flat[:nq].view(geom.n_query, 3, *geom.q_canvas), flat[nq:n].view(geom.n_support, 3, *geom.s_canvas))


# ---------------------------------------------------------------------------------------------------
# test-time augmentation tail (csrc/ore_tta.hip): flipped variants, per-variant collection, the merge
# ---------------------------------------------------------------------------------------------------
TTA_MAX_CANDIDATES = 8192                                # rows one ore_tta_merge_fwd takes (include/ore_hip.h)


def tta_hflip_u8(img_chw_u8: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[3, nh, nw] uint8 planar device image with its columns reversed (img[:, :, ::-1]) -- the flipped TTA variant, a copy of the
    resized variant's bytes (ore_tta_hflip_u8_fwd).  Enqueued on the current stream."""
    assert img_chw_u8.is_cuda and img_chw_u8.dtype == torch.uint8 and img_chw_u8.dim() == 3 and img_chw_u8.is_contiguous(), \
        "tta_hflip_u8 takes a contiguous [c, h, w] uint8 device tensor"
    if out is None:
        out = torch.empty_like(img_chw_u8)
    assert out.is_cuda and out.dtype == torch.uint8 and out.shape == img_chw_u8.shape and out.is_contiguous()
    c, nh, nw = (int(v) for v in img_chw_u8.shape)
    with torch.cuda.device(img_chw_u8.device):
        _chk(lib().ore_tta_hflip_u8_fwd(_ptr(img_chw_u8), _ptr(out), c * nh, nw, _stream()), "ore_tta_hflip_u8_fwd")
    return out


class TTAPool:
    """Device buffers of one TTA merge: the candidate pool of `variants` x `rows` rows (boxes, scores, class ids), its running row
    count, the per-variant counts and the merge workspace."""

    def __init__(self, variants: int, rows: int, device):
        self.variants, self.rows, self.cap = int(variants), int(rows), int(variants) * int(rows)
        if not 1 <= self.cap <= TTA_MAX_CANDIDATES:
            raise OreError(f"TTAPool: {variants} variants x {rows} rows = {self.cap} candidates, one merge takes 1 .. {TTA_MAX_CANDIDATES}")
        dev = torch.device(device)
        self.boxes = torch.zeros(self.cap, 4, dtype=torch.float32, device=dev)
        self.scores = torch.zeros(self.cap, dtype=torch.float32, device=dev)
        self.classes = torch.zeros(self.cap, dtype=torch.int64, device=dev)
        self.n = torch.zeros(1, dtype=torch.int32, device=dev)
        self.var_counts = torch.zeros(self.variants, dtype=torch.int32, device=dev)
        self.ws_bytes = int(lib().ore_tta_merge_workspace_bytes(self.cap))
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=dev)


def tta_collect(pool: TTAPool, variant: int, boxes, scores, classes, n, max_rows: int, *, flip: bool, variant_w: int,
                sx: float, sy: float, pre: Optional[Tuple[float, float]] = None) -> None:
    """Append one variant's detection rows, inverse-transformed, to the pool (ore_tta_collect_fwd; no host sync).  boxes [.., 4] /
    scores / classes (int64, or None: all 0): device tensors whose rows are contiguous; n: an int32 device tensor holding the row count
    (read by the kernel) or a host int; at most max_rows rows are taken.  sx, sy (and pre = (px, py)) are the inverse resize ratios,
    computed in double by the caller and rounded to fp32 here."""
    n_dev, n_host = (_ptr(n), 0) if torch.is_tensor(n) else (None, int(n))
    px, py = pre if pre is not None else (1.0, 1.0)
    with torch.cuda.device(pool.boxes.device):
        _chk(lib().ore_tta_collect_fwd(_ptr(boxes), _ptr(scores), _ptr(classes), n_dev, n_host, int(max_rows), int(bool(flip)), int(variant_w),
                                       float(np.float32(sx)), float(np.float32(sy)), int(pre is not None), float(np.float32(px)),
                                       float(np.float32(py)), _ptr(pool.boxes), _ptr(pool.scores), _ptr(pool.classes), _ptr(pool.n), pool.cap,
                                       _ptr(pool.var_counts), int(variant), _stream()), "ore_tta_collect_fwd")


def tta_merge(pool: TTAPool, out_h: int, out_w: int, score_thresh: float, nms_thresh: float, topk: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """fast_rcnn_inference_single_image over the pool (ore_tta_merge_fwd; no host sync): returns (record, count) -- a fresh fp32 tensor
    laid out [R][4] boxes | [R] scores | [R] int64 classes with R = topk rounded up to even, and the int32 device count of its valid rows.
    `record_views(record, R, count)` cuts it."""
    R = int(topk) + (int(topk) & 1)
    dev = pool.boxes.device
    rec = torch.empty(R * 7, dtype=torch.float32, device=dev)
    cnt = torch.empty(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _chk(lib().ore_tta_merge_fwd(_ptr(pool.boxes), _ptr(pool.scores), _ptr(pool.classes), _ptr(pool.n), pool.cap, int(out_h), int(out_w),
                                     float(score_thresh), float(nms_thresh), int(topk), _ptr(rec), R, _ptr(cnt), _ptr(pool.ws), pool.ws_bytes,
                                     _stream()), "ore_tta_merge_fwd")
    return rec, cnt


def record_views(rec: torch.Tensor, R: int, k: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(boxes [k, 4], scores [k], classes [k] int64) of a result record of R rows (the layout of Engine.detect_end)."""
    return rec.as_strided((k, 4), (4, 1)), rec.as_strided((k,), (1,), R * 4), rec.view(torch.int64).as_strided((k,), (1,), R * 5 // 2)


# ---------------------------------------------------------------------------------------------------
# tiled inference (csrc/ore_tile.hip): the tile plan, the gather of every tile in one launch, the per-source collection with the seam
# rule.  tile_gather_u8 / tile_collect are the kernels, tile_gather_host / tile_collect_host the numpy statements of the same contracts.
# ---------------------------------------------------------------------------------------------------
TILE_MAX_SIDE, TILE_MAX_TILES = 8192, 128                # limits of ore_tile_gather_u8_fwd (include/ore_hip.h)
TILE_EDGE_LEFT, TILE_EDGE_TOP, TILE_EDGE_RIGHT, TILE_EDGE_BOTTOM = 1, 2, 4, 8


def _tile_axis(L: int, t: int, o: int) -> Tuple[int, int, int, List[int]]:
    """One axis of tile_plan: (extent, stride, count, starts)."""
    L, t, o = int(L), int(t), int(o)
    if L < 1 or t < 1 or not 0 <= o < t:
        raise ValueError(f"tile_plan: length {L} (>= 1), tile {t} (>= 1), overlap {o} (0 .. tile - 1)")
    e, s = min(t, L), t - o
    n = 1 if L <= t else -((t - L) // s) + 1             # ceil((L - t) / s) + 1
    return e, s, n, [min(k * s, L - e) for k in range(n)]


def tile_plan(h: int, w: int, tile_hw: Tuple[int, int], overlap_hw: Tuple[int, int]) -> dict:
    """The tiles of an [h, w] frame, pure integer: dict(th, tw, ny, nx, stride_y, stride_x, origins).  Per axis with length L, tile t
    and overlap o (0 <= o < t): the extent is min(t, L); L <= t gives one tile at 0; otherwise the stride is t - o, there are
    ceil((L - t) / stride) + 1 tiles and tile k starts at min(k * stride, L - extent) -- the last tile is flush with the far edge and
    nothing is ever padded.  All tiles have the same extent (th, tw); origins lists (y0, x0) row-major (iy * nx + ix)."""
    th, sy, ny, ys = _tile_axis(h, tile_hw[0], overlap_hw[0])
    tw, sx, nx, xs = _tile_axis(w, tile_hw[1], overlap_hw[1])
    return dict(th=th, tw=tw, ny=ny, nx=nx, stride_y=sy, stride_x=sx, origins=[(y, x) for y in ys for x in xs])


def tile_edges(plan: dict, index: int, h: int, w: int) -> int:
    """The `edges` bits of tile `index` of a plan over an [h, w] frame: a bit is set where the frame continues beyond the tile."""
    y0, x0 = plan["origins"][index]
    return (TILE_EDGE_LEFT if x0 > 0 else 0) | (TILE_EDGE_TOP if y0 > 0 else 0) | \
        (TILE_EDGE_RIGHT if x0 + plan["tw"] < w else 0) | (TILE_EDGE_BOTTOM if y0 + plan["th"] < h else 0)


def tile_gather_host(frame_hwc_u8, plan: dict, swap_rb: bool = False) -> np.ndarray:
    """The gather contract on the host: [ny * nx, 3, th, tw] uint8, tile i = frame[y0 : y0 + th, x0 : x0 + tw] of plan["origins"][i]
    transposed to planar, channels 0 and 2 exchanged with swap_rb."""
    frame = np.asarray(frame_hwc_u8)
    assert frame.dtype == np.uint8 and frame.ndim == 3 and frame.shape[2] == 3, "tile_gather_host takes an [h, w, 3] uint8 frame"
    th, tw = plan["th"], plan["tw"]
    out = np.stack([frame[y:y + th, x:x + tw].transpose(2, 0, 1) for y, x in plan["origins"]])
    return np.ascontiguousarray(out[:, ::-1] if swap_rb else out)


def tile_collect_host(boxes, scores, classes=None, *, sx: float, sy: float, ox: float, oy: float, src_hw: Tuple[int, int], edges: int,
                      margin: float):
    """The collect contract on the host, fp32 throughout: the seam rule on the source-local rows (a comparison with NaN is false, so
    such a row is kept), then x' = fl(fl(x * sx) + ox), y' = fl(fl(y * sy) + oy) on the kept rows, in row order.  Returns (boxes
    [k, 4] float32, scores [k] float32, classes [k] int64, kept: bool mask over the input rows)."""
    b = np.ascontiguousarray(boxes, dtype=np.float32).reshape(-1, 4)
    s = np.asarray(scores, dtype=np.float32).reshape(-1)
    c = np.zeros(len(s), dtype=np.int64) if classes is None else np.asarray(classes, dtype=np.int64).reshape(-1)
    m, edges = np.float32(margin), int(edges)
    x_hi, y_hi = np.float32(src_hw[1]) - m, np.float32(src_hw[0]) - m
    cut = np.zeros(len(s), dtype=bool)
    with np.errstate(all="ignore"):
        if edges & TILE_EDGE_LEFT:
            cut |= b[:, 0] < m
        if edges & TILE_EDGE_TOP:
            cut |= b[:, 1] < m
        if edges & TILE_EDGE_RIGHT:
            cut |= b[:, 2] > x_hi
        if edges & TILE_EDGE_BOTTOM:
            cut |= b[:, 3] > y_hi
        k = b[~cut]
        out = np.empty_like(k)
        out[:, 0::2] = k[:, 0::2] * np.float32(sx) + np.float32(ox)
        out[:, 1::2] = k[:, 1::2] * np.float32(sy) + np.float32(oy)
    return out, s[~cut], c[~cut], ~cut


class TilePool(TTAPool):
    """The merge pool of one tiled frame: a TTAPool of `sources` x `rows` candidates (ore_tta_merge_fwd reads it unchanged) with, per
    source, the rows appended (src_counts, the TTAPool's var_counts) and the rows the seam rule rejected (src_dropped)."""

    def __init__(self, sources: int, rows: int, device):
        super().__init__(sources, rows, device)
        self.sources, self.src_counts = self.variants, self.var_counts
        self.src_dropped = torch.zeros(self.sources, dtype=torch.int32, device=self.boxes.device)


def tile_gather_u8(frame_hwc_u8: torch.Tensor, plan: dict, swap_rb: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[h, w, 3] uint8 device frame (interleaved) -> [ny * nx, 3, th, tw] uint8 planar tiles of tile_plan(h, w, ...), byte for byte
    tile_gather_host, in one launch (ore_tile_gather_u8_fwd) on the current stream.  tiles[i] and tiles[i : i + B] are the images
    Engine.eval_forward / eval_forward_batch take."""
    assert frame_hwc_u8.is_cuda and frame_hwc_u8.dtype == torch.uint8 and frame_hwc_u8.dim() == 3 and frame_hwc_u8.shape[2] == 3 and \
        frame_hwc_u8.is_contiguous(), "tile_gather_u8 takes a contiguous [h, w, 3] uint8 device tensor"
    h, w = int(frame_hwc_u8.shape[0]), int(frame_hwc_u8.shape[1])
    n, th, tw = int(plan["ny"]) * int(plan["nx"]), int(plan["th"]), int(plan["tw"])
    dev = frame_hwc_u8.device
    if out is None:
        out = torch.empty(n, 3, th, tw, dtype=torch.uint8, device=dev)
    assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (n, 3, th, tw) and out.is_contiguous()
    with torch.cuda.device(dev):
        _chk(lib().ore_tile_gather_u8_fwd(_ptr(frame_hwc_u8), h, w, th, tw, int(plan["stride_y"]), int(plan["stride_x"]), int(plan["ny"]),
                                          int(plan["nx"]), int(bool(swap_rb)), _ptr(out), _stream()), "ore_tile_gather_u8_fwd")
    return out


def tile_collect(pool: TilePool, source: int, boxes, scores, classes, n, max_rows: int, *, sx: float, sy: float, ox: float, oy: float,
                 src_hw: Tuple[int, int], edges: int, margin: float) -> None:
    """Append one source's detection rows -- a tile's, or the full-frame pass's -- to the pool behind the seam rule and the transform
    of tile_collect_host (ore_tile_collect_fwd; no host sync).  boxes [.., 4] / scores / classes (int64, or None: all 0): device tensors
    whose rows are contiguous; n: an int32 device tensor holding the row count (read by the kernel) or a host int; at most max_rows
    rows are taken.  sx, sy, ox, oy and margin are rounded to fp32 here; source 0 restarts the pool."""
    n_dev, n_host = (_ptr(n), 0) if torch.is_tensor(n) else (None, int(n))
    with torch.cuda.device(pool.boxes.device):
        _chk(lib().ore_tile_collect_fwd(_ptr(boxes), _ptr(scores), _ptr(classes), n_dev, n_host, int(max_rows), float(np.float32(sx)),
                                        float(np.float32(sy)), float(np.float32(ox)), float(np.float32(oy)), int(src_hw[0]), int(src_hw[1]),
                                        int(edges), float(np.float32(margin)), _ptr(pool.boxes), _ptr(pool.scores), _ptr(pool.classes),
                                        _ptr(pool.n), pool.cap, _ptr(pool.src_counts), _ptr(pool.src_dropped), int(source), _stream()),
             "ore_tile_collect_fwd")


# ---------------------------------------------------------------------------------------------------
# detection overlay (csrc/ore_overlay.hip): boxes, scores and class names drawn onto a frame; render contract "overlay v1" of
# include/ore_hip.h.  overlay_draw is the kernel, overlay_host the numpy statement of the same contract: both give the same bytes.
# ---------------------------------------------------------------------------------------------------
OVERLAY_MAX_SIDE, OVERLAY_TEXT, OVERLAY_NAME = 8192, 40, 32          # ORE_OVERLAY_MAX_SIDE; characters of a label; bytes of a name
# the default palette, RGB (a BGR frame takes it reversed along the last axis): the one place it is defined
OVERLAY_PALETTE = np.array([[230, 25, 75], [60, 180, 75], [255, 225, 25], [0, 130, 200], [245, 130, 48], [145, 30, 180], [70, 240, 240],
                            [240, 50, 230], [210, 245, 60], [250, 190, 212], [0, 128, 128], [220, 190, 255], [170, 110, 40],
                            [255, 250, 200], [128, 0, 0], [170, 255, 195], [128, 128, 0], [255, 215, 180], [0, 0, 128], [128, 128, 128]],
                           dtype=np.uint8)
_OVERLAY_ATLAS: Optional[np.ndarray] = None
_OVERLAY_TABLES: Dict[tuple, torch.Tensor] = {}
_OVERLAY_TABLES_MAX = 32
_OVERLAY_WS: Dict[tuple, torch.Tensor] = {}
_OVERLAY_WS_MAX = 16


def overlay_atlas() -> np.ndarray:
    """[95, 11, 6] uint8 (0 / 1): the glyphs of ASCII 32 .. 126 of Pillow's embedded bitmap font, every one a 6 x 11 cell of coverage
    0 or 255.  Built once; the kernel, overlay_host and the tests read this one table."""
    global _OVERLAY_ATLAS
    if _OVERLAY_ATLAS is None:
        from PIL import ImageFont
        font = ImageFont.load_default_imagefont()
        atlas = np.zeros((95, 11, 6), dtype=np.uint8)
        for ch in range(32, 127):
            m = font.getmask(chr(ch))
            if m.size != (6, 11):
                raise OreError(f"overlay_atlas: glyph {ch} of Pillow's bitmap font is {m.size}, not 6 x 11")
            cov = np.asarray(m, dtype=np.uint8).reshape(11, 6)
            if not np.isin(cov, (0, 255)).all():
                raise OreError(f"overlay_atlas: glyph {ch} of Pillow's bitmap font is not 0 / 255")
            atlas[ch - 32] = cov != 0
        atlas.setflags(write=False)
        _OVERLAY_ATLAS = atlas
    return _OVERLAY_ATLAS


def overlay_names_table(names) -> np.ndarray:
    """Class names as the kernel's table: [n, 32] uint8, ASCII, NUL-padded (longer names are cut at 32 bytes)."""
    names = [] if names is None else list(names)
    tab = np.zeros((len(names), OVERLAY_NAME), dtype=np.uint8)
    for i, nm in enumerate(names):
        raw = str(nm).encode("ascii", "replace")[:OVERLAY_NAME]
        tab[i, :len(raw)] = np.frombuffer(raw, dtype=np.uint8)
    return tab


def _overlay_palette(palette) -> np.ndarray:
    pal = OVERLAY_PALETTE if palette is None else np.ascontiguousarray(np.asarray(palette))
    if pal.dtype != np.uint8 or pal.ndim != 2 or pal.shape[1] != 3 or not 1 <= pal.shape[0] <= 256:
        raise OreError(f"overlay: the palette is [1 .. 256, 3] uint8, got {pal.shape} {pal.dtype}")
    return pal


def _overlay_color_by(color_by: str, ids=None, has_ids: bool = True) -> int:
    """0 instance, 1 class, 2 track ("overlay v1, track colouring": needs ids)."""
    if color_by not in ("instance", "class", "track"):
        raise OreError(f'overlay: color_by is "instance", "class" or "track", not {color_by!r}')
    if color_by == "track" and ids is None and has_ids:
        raise OreError('overlay: color_by "track" needs ids (the ids of a BoxTracker update)')
    return ("instance", "class", "track").index(color_by)


def _overlay_table_dev(dev, key: tuple, make) -> torch.Tensor:
    """A constant table (atlas, palette, names) on the device, uploaded once and cached under `key` (make() builds the numpy table on a
    miss); never built inside a stream capture.  Stream order, the upload's event for a use on another stream, and record_stream
    protect a table as they do the resize tables (_resize_tables, _table_on_stream)."""
    key = (str(dev),) + key
    tab = _OVERLAY_TABLES.get(key)
    cur = _stream()
    if tab is None:
        if torch.cuda.is_current_stream_capturing():
            raise OreError("overlay_draw: a table is not on the device yet; draw once outside the stream capture first")
        arr = np.array(make(), dtype=np.uint8).reshape(-1)        # a writable copy: the atlas is read-only
        host = torch.empty(max(arr.size, 1), dtype=torch.uint8, pin_memory=True)
        host[:arr.size].copy_(torch.from_numpy(arr))
        while len(_OVERLAY_TABLES) >= _OVERLAY_TABLES_MAX:
            _OVERLAY_TABLES.pop(next(iter(_OVERLAY_TABLES)))
        tab = _OVERLAY_TABLES[key] = host.to(dev, non_blocking=True)
        _table_uploaded(tab, cur)
    else:
        _table_on_stream(tab, cur)
    return tab


def overlay_draw(frame_hwc_u8: torch.Tensor, boxes: torch.Tensor, scores: torch.Tensor, classes: Optional[torch.Tensor] = None,
                 n_dev: Optional[torch.Tensor] = None, *, out: Optional[torch.Tensor] = None, score_thresh: float = 0.0, line_width: int,
                 text_scale: int, edge_alpha: int = 128, label_alpha: int = 204, palette=None, color_by: str = "instance",
                 names=None, ids: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Detection rows drawn onto a contiguous [h, w, 3] uint8 device frame (ore_overlay_draw_fwd; the render contract "overlay v1" of
    include/ore_hip.h), enqueued on the current stream, no host sync.  boxes [n, 4] fp32 xyxy at the frame's size, scores [n] fp32,
    classes [n] int64 or None (all 0): device tensors whose rows are contiguous.  n_dev: an int32 device tensor holding the row count
    (read by the kernel; at most boxes.shape[0] rows are taken), or None: every row.  out=None returns a fresh frame, out=frame draws
    in place.  palette: [k, 3] uint8 in the frame's channel order (None: OVERLAY_PALETTE, RGB); color_by "instance" or "class";
    names: class names (None: no names, the labels are the percentages); text_scale 0 draws no labels.  ids [n] int64 (a BoxTracker
    update's) with color_by "track": "overlay v1, track colouring" -- rows with a negative id are not drawn, the colour follows the id
    and "#<id> " leads the label; with another color_by the ids are ignored."""
    f = frame_hwc_u8
    assert f.is_cuda and f.dtype == torch.uint8 and f.dim() == 3 and f.shape[2] == 3 and f.is_contiguous(), \
        "overlay_draw takes a contiguous [h, w, 3] uint8 device tensor"
    h, w = int(f.shape[0]), int(f.shape[1])
    dev = f.device
    rows = int(boxes.shape[0])
    assert boxes.dtype == torch.float32 and scores.dtype == torch.float32 and (classes is None or classes.dtype == torch.int64)
    assert (rows == 0 or boxes.stride(-1) == 1 and boxes.stride(0) == 4) and int(scores.shape[0]) == rows and \
        (classes is None or int(classes.shape[0]) == rows), "overlay_draw: boxes [n, 4], scores [n], classes [n], rows contiguous"
    assert rows <= 1 or (scores.stride(0) == 1 and (classes is None or classes.stride(0) == 1))
    assert all(t is None or t.device == dev for t in (boxes, scores, classes)), "overlay_draw: the rows live on the frame's device"
    if n_dev is not None and not (torch.is_tensor(n_dev) and n_dev.dtype == torch.int32 and n_dev.device == dev and n_dev.numel() >= 1):
        raise OreError("overlay_draw: n_dev is an int32 tensor on the frame's device (the kernel reads its first element)")
    if out is None:
        out = torch.empty_like(f)
    assert out.is_cuda and out.dtype == torch.uint8 and out.shape == f.shape and out.is_contiguous() and out.device == dev
    pal = _overlay_palette(palette)
    by = _overlay_color_by(color_by, ids)
    if ids is not None and not (torch.is_tensor(ids) and ids.dtype == torch.int64 and ids.device == dev and ids.dim() == 1 and
                                int(ids.shape[0]) == rows and (rows <= 1 or ids.stride(0) == 1)):
        raise OreError("overlay_draw: ids is a contiguous int64 tensor [n] on the frame's device")
    names = () if names is None else tuple(str(nm) for nm in names)
    with torch.cuda.device(dev):
        pal_d = _overlay_table_dev(dev, ("palette", None if palette is None else pal.tobytes()), lambda: pal)
        atlas_d = _overlay_table_dev(dev, ("atlas",), overlay_atlas) if int(text_scale) >= 1 else None
        names_d = _overlay_table_dev(dev, ("names", names), lambda: overlay_names_table(names)) if names else None
        ws_bytes = int(lib().ore_overlay_workspace_bytes(rows))
        ws_key = (str(dev), _stream())                              # per stream: two streams' draws must not share an instance table
        ws = _OVERLAY_WS.get(ws_key)
        if ws is None or ws.numel() < ws_bytes:
            while ws is None and len(_OVERLAY_WS) >= _OVERLAY_WS_MAX:    # streams come and go: the oldest stream's workspace leaves
                _OVERLAY_WS.pop(next(iter(_OVERLAY_WS)))                  # (its block returns to the stream it was allocated on)
            ws = _OVERLAY_WS[ws_key] = torch.empty(max(ws_bytes, int(lib().ore_overlay_workspace_bytes(int(lib().ore_det_record_rows())))),
                                                   dtype=torch.uint8, device=dev)
        if ids is None:
            _chk(lib().ore_overlay_draw_fwd(_ptr(f), _ptr(out), h, w, _ptr(boxes) if rows else None, _ptr(scores) if rows else None,
                                            _ptr(classes) if rows else None, _ptr(n_dev), rows, rows, float(np.float32(score_thresh)),
                                            int(line_width), int(text_scale), int(edge_alpha), int(label_alpha), _ptr(pal_d), len(pal), by,
                                            _ptr(names_d), len(names), _ptr(atlas_d), _ptr(ws), ws.numel(), _stream()), "ore_overlay_draw_fwd")
        else:
            _chk(lib().ore_overlay_draw_ids_fwd(_ptr(f), _ptr(out), h, w, _ptr(boxes) if rows else None, _ptr(scores) if rows else None,
                                                _ptr(classes) if rows else None, _ptr(ids) if rows else None, _ptr(n_dev), rows, rows,
                                                float(np.float32(score_thresh)), int(line_width), int(text_scale), int(edge_alpha),
                                                int(label_alpha), _ptr(pal_d), len(pal), by, _ptr(names_d), len(names), _ptr(atlas_d),
                                                _ptr(ws), ws.numel(), _stream()), "ore_overlay_draw_ids_fwd")
    return out


def _blend8(p: np.ndarray, c, a: int) -> np.ndarray:
    return ((p.astype(np.int32) * (255 - a) + np.asarray(c, dtype=np.int32) * a + 127) // 255).astype(np.uint8)


def overlay_instance_table(boxes, scores, classes, n, h: int, w: int, score_thresh: float, text_scale: int, palette: np.ndarray, color_by: int,
                           names_tab: np.ndarray, ids=None) -> List[dict]:
    """The instance table of the render contract, in draw order, as the prepare step of the kernel builds it: per drawn row the
    integer rectangle, colour, text colour, label text and label rectangle.  Host arithmetic in numpy fp32, one operation at a time.
    color_by 2 ("overlay v1, track colouring") reads ids [n] int64: negative ids are not drawn, the id picks the colour and leads the text."""
    by_track = color_by == 2
    if by_track:
        if ids is None:
            raise OreError('overlay: color_by "track" needs ids')
        tid = np.asarray(ids, dtype=np.int64).reshape(-1)
    b = np.ascontiguousarray(np.asarray(boxes, dtype=np.float32)).reshape(-1, 4)
    s = np.asarray(scores, dtype=np.float32).reshape(-1)
    c = np.zeros(len(s), dtype=np.int64) if classes is None else np.asarray(classes, dtype=np.int64).reshape(-1)
    n = len(s) if n is None else min(max(int(n), 0), len(s))
    b, s, c = b[:n], s[:n], c[:n]
    S = int(text_scale)
    with np.errstate(all="ignore"):
        ok = np.isfinite(b).all(1) & np.isfinite(s) & (s >= np.float32(score_thresh))
        if by_track:
            if len(tid) < n:
                raise OreError(f"overlay: {len(tid)} ids for {n} rows")
            tid = tid[:n]
            ok &= tid >= 0
        X0 = np.clip(np.floor(b[:, 0]), 0, w)
        Y0 = np.clip(np.floor(b[:, 1]), 0, h)
        X1 = np.clip(np.ceil(b[:, 2]), 0, w) - 1
        Y1 = np.clip(np.ceil(b[:, 3]), 0, h) - 1
        ok &= (X1 >= X0) & (Y1 >= Y0)
        area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
        pct = np.clip(np.rint(s * np.float32(100.0)), 0, 100)
    area = np.where(np.isnan(area), np.float32(0), area)
    idx = np.arange(n)
    table: List[Optional[dict]] = [None] * int(ok.sum())
    for i in idx[ok]:
        rank = int((ok & ((area > area[i]) | ((area == area[i]) & (idx < i)))).sum())
        col = palette[int((tid[i] if by_track else c[i] if color_by else i) % len(palette))].astype(np.int32)
        q = {"row": int(i), "rect": (int(X0[i]), int(Y0[i]), int(X1[i]), int(Y1[i])), "col": col, "tcol": col + ((255 - col) * 7) // 10, "text": b""}
        if S >= 1:
            name = b""
            if 0 <= c[i] < len(names_tab):
                name = bytes(names_tab[c[i]]).split(b"\0")[0]
            text = (b"#%d " % int(tid[i]) if by_track else b"") + ((name + b" ") if name else b"") + b"%d%%" % int(pct[i])
            q["text"] = text = text[:OVERLAY_TEXT]
            lw, lh = len(text) * 6 * S + 2 * S, 13 * S
            q["label"] = (min(max(int(X0[i]), 0), max(w - lw, 0)), min(max(int(Y0[i]), 0), max(h - lh, 0)), lw, lh)
        table[rank] = q
    return table


def overlay_host(frame_hwc_u8, boxes, scores, classes=None, n=None, *, out=None, score_thresh: float = 0.0, line_width: int, text_scale: int,
                 edge_alpha: int = 128, label_alpha: int = 204, palette=None, color_by: str = "instance", names=None, ids=None) -> np.ndarray:
    """overlay_draw on the host: the numpy statement of the render contract "overlay v1" (include/ore_hip.h), byte for byte what the
    kernel draws.  Takes numpy arrays or CPU tensors; n = the row count (None: every row).  Returns an [h, w, 3] uint8 array: a fresh
    one, or `out` (the frame itself: in place)."""
    as_np = lambda t: t.detach().cpu().numpy() if torch.is_tensor(t) else (None if t is None else np.asarray(t))
    frame = as_np(frame_hwc_u8)
    if frame.dtype != np.uint8 or frame.ndim != 3 or frame.shape[2] != 3:
        raise OreError(f"overlay_host takes an [h, w, 3] uint8 frame, got {frame.shape} {frame.dtype}")
    h, w = frame.shape[:2]
    L, S = int(line_width), int(text_scale)
    rows = len(as_np(scores))
    if not (1 <= h <= OVERLAY_MAX_SIDE and 1 <= w <= OVERLAY_MAX_SIDE and 1 <= L <= 16 and 0 <= S <= 8 and 0 <= int(edge_alpha) <= 255 and
            0 <= int(label_alpha) <= 255 and rows <= int(lib().ore_det_record_rows())):
        raise OreError(f"overlay_host: frame {h}x{w} (sides 1 .. {OVERLAY_MAX_SIDE}), {rows} rows, line_width {L} (1 .. 16), text_scale {S} (0 .. 8), "
                       f"alphas {edge_alpha} / {label_alpha} (0 .. 255)")
    pal = _overlay_palette(palette)
    table = overlay_instance_table(as_np(boxes), as_np(scores), as_np(classes), n, h, w, score_thresh, S, pal, _overlay_color_by(color_by, ids),
                                   overlay_names_table(names), ids=as_np(ids))
    if out is None:
        img = frame.copy()
    else:
        img = out if out is frame_hwc_u8 or out is frame else as_np(out)
        if img is not frame:
            img[...] = frame
    atlas = overlay_atlas()
    for q in table:
        X0, Y0, X1, Y1 = q["rect"]
        xs, ys = np.arange(X0, X1 + 1), np.arange(Y0, Y1 + 1)
        edge = ((xs - X0 < L) | (X1 - xs < L))[None, :] | ((ys - Y0 < L) | (Y1 - ys < L))[:, None]
        reg = img[Y0:Y1 + 1, X0:X1 + 1]
        reg[edge] = _blend8(reg[edge], q["col"], int(edge_alpha))
        if S >= 1:
            lx, ly, lw, lh = q["label"]
            xs, ys = np.arange(lx, min(lx + lw, w)), np.arange(ly, min(ly + lh, h))
            reg = img[ly:ly + len(ys), lx:lx + len(xs)]
            reg[...] = _blend8(reg, 0, int(label_alpha))
            gx, gy = xs - lx - S, ys - ly - S
            chars = np.frombuffer(q["text"], dtype=np.uint8).astype(np.int64) - 32
            okx, oky = (gx >= 0) & (gx < len(chars) * 6 * S), (gy >= 0) & (gy < 11 * S)
            cell = np.clip(gx // (6 * S), 0, len(chars) - 1)
            ch = chars[cell]
            u, v = np.clip((gx - cell * 6 * S) // S, 0, 5), np.clip(gy // S, 0, 10)
            okx &= (ch >= 0) & (ch < 95)
            on = atlas[np.clip(ch, 0, 94)[None, :], v[:, None], u[None, :]].astype(bool) & okx[None, :] & oky[:, None]
            reg[on] = q["tcol"].astype(np.uint8)
    return img


# ---------------------------------------------------------------------------------------------------
# Detection tracking (csrc/ore_track.hip; association contract "track v1", include/ore_hip.h).  BoxTracker holds the state and runs the
# kernel, track_host is the numpy statement of the same contract: both give the same ids and the same state.
TRACK_MAX_TRACKS = 1024                                    # ORE_TRACK_MAX_TRACKS
TRACK_WIDE_MAX_TRACKS, TRACK_WIDE_MAX_ROWS = 16384, 8192   # ORE_TRACK_WIDE_MAX_TRACKS, ORE_TRACK_WIDE_MAX_ROWS (csrc/ore_track_wide.hip)
TRACK_WIDE_DEFAULTS = {"capacity": 4096, "max_rows": 2048, "iou_thresh": 0.6, "ttl": 8, "class_aware": True, "score_thresh": 0.0}
TRACK_DEFAULTS = {"capacity": 1024, "iou_thresh": 0.6, "ttl": 8, "class_aware": True, "score_thresh": 0.0}
_TRACK_HEADER = 32                                         # bytes: int32 m, capacity; int64 next_id, frames, dropped


def _track_params(who: str, capacity, iou_thresh, ttl, class_aware, score_thresh, max_tracks: int = TRACK_MAX_TRACKS) -> dict:
    """The parameters of a tracker, checked against the limits of ore_track_update_fwd (max_tracks = TRACK_WIDE_MAX_TRACKS: of
    ore_track_wide_update_fwd); the thresholds as the fp32 the kernel takes."""
    with np.errstate(over="ignore"):
        iou, sc = np.float32(iou_thresh), np.float32(score_thresh)
    if isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer)) or not 1 <= capacity <= max_tracks:
        raise OreError(f"{who}: capacity {capacity!r} (1 .. {max_tracks})")
    if isinstance(ttl, bool) or not isinstance(ttl, (int, np.integer)) or not 1 <= ttl <= 1 << 20:
        raise OreError(f"{who}: ttl {ttl!r} (1 .. {1 << 20})")
    if not (np.isfinite(iou) and iou >= 0):
        raise OreError(f"{who}: iou_thresh {iou_thresh!r} is finite and >= 0")
    if np.isnan(sc):
        raise OreError(f"{who}: score_thresh is NaN")
    return {"capacity": int(capacity), "iou_thresh": iou, "ttl": int(ttl), "class_aware": bool(class_aware), "score_thresh": sc}


def track_state_empty(capacity: int = 1024) -> dict:
    """The state of a tracker that has seen no frame, as track_host takes and returns it: the arrays cut at m = 0."""
    return {"boxes": np.zeros((0, 4), np.float32), "classes": np.zeros(0, np.int64), "ids": np.zeros(0, np.int64), "ttl": np.zeros(0, np.int32),
            "m": 0, "next_id": 0, "frames": 0, "dropped": 0}


def track_host(state, boxes, scores, classes=None, n=None, *, capacity: int = 1024, iou_thresh: float = 0.6, ttl: int = 8,
               class_aware: bool = True, score_thresh: float = 0.0, wide: bool = False):
    """One update of the association contract "track v1" (include/ore_hip.h) on the host, numpy fp32 one operation at a time: what
    ore_track_update_fwd computes, bit for bit.  wide=True: the same code with the limits of ore_track_wide_update_fwd (capacity up to
    16384, up to 8192 rows) -- what that computes, bit for bit.  state: a dict {boxes [m, 4] fp32, classes, ids [m] int64, ttl [m] int32, m, next_id,
    frames, dropped} (None: the empty state); boxes [rows, 4], scores [rows], classes [rows] or None (all 0), n = rows taken (None: all).
    Returns (ids [rows] int64 with -1 for rows that are not live, the new state); `state` is left as it was."""
    as_np = lambda t: t.detach().cpu().numpy() if torch.is_tensor(t) else (None if t is None else np.asarray(t))
    p = _track_params("track_host", capacity, iou_thresh, ttl, class_aware, score_thresh, TRACK_WIDE_MAX_TRACKS if wide else TRACK_MAX_TRACKS)
    max_rows = TRACK_WIDE_MAX_ROWS if wide else int(lib().ore_det_record_rows())
    st = track_state_empty() if state is None else state
    m = int(st["m"])
    tb = np.asarray(as_np(st["boxes"]), dtype=np.float32).reshape(-1, 4)[:m]
    tc, ti, tt = (np.asarray(as_np(st[k])).reshape(-1)[:m] for k in ("classes", "ids", "ttl"))
    b = np.ascontiguousarray(np.asarray(as_np(boxes), dtype=np.float32)).reshape(-1, 4)
    s = np.asarray(as_np(scores), dtype=np.float32).reshape(-1)
    rows = len(s)
    if rows > max_rows or len(b) != rows:
        raise OreError(f"track_host: {len(b)} boxes, {rows} scores (at most {max_rows} rows)")
    c = np.zeros(rows, dtype=np.int64) if classes is None else np.asarray(as_np(classes), dtype=np.int64).reshape(-1)
    n = rows if n is None else min(max(int(n), 0), rows)
    with np.errstate(all="ignore"):
        live = (np.arange(rows) < n) & np.isfinite(b).all(1) & np.isfinite(s) & (s >= p["score_thresh"])
        # IoU [m, rows], the contract's expression: a subtraction, a product, a sum, a difference and a quotient, each rounded to fp32
        area_t = (tb[:, 2] - tb[:, 0]) * (tb[:, 3] - tb[:, 1])
        area_d = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
        iw = np.minimum(tb[:, None, 2], b[None, :, 2]) - np.maximum(tb[:, None, 0], b[None, :, 0])
        ih = np.minimum(tb[:, None, 3], b[None, :, 3]) - np.maximum(tb[:, None, 1], b[None, :, 1])
        inter = np.where((iw > 0) & (ih > 0), iw * ih, np.float32(0))
        union = (area_t[:, None] + area_d[None, :]) - inter
        iou = np.where(inter > 0, inter / np.where(inter > 0, union, np.float32(1)), np.float32(0)).astype(np.float32)
        cand = live[None, :] & (iou > p["iou_thresh"])
    if p["class_aware"]:
        cand &= tc[:, None] == c[None, :]
    # greedy over (iou descending, slot ascending, row ascending): np.nonzero lists the pairs by (slot, row), a stable sort keeps that
    ts, ds = np.nonzero(cand)
    order = np.argsort(-iou[ts, ds].astype(np.float64), kind="stable")
    row_track = np.full(rows, -1, dtype=np.int64)
    track_row = np.full(m, -1, dtype=np.int64)
    for k in order:
        t, d = int(ts[k]), int(ds[k])
        if track_row[t] < 0 and row_track[d] < 0:
            track_row[t], row_track[d] = d, t
    ids = np.full(rows, -1, dtype=np.int64)
    next_id = int(st["next_id"])
    for d in np.nonzero(live)[0]:
        if row_track[d] >= 0:
            ids[d] = ti[row_track[d]]
        else:
            ids[d] = next_id
            next_id += 1
    keep = (track_row < 0) & (tt.astype(np.int64) - 1 > 0)
    nb = np.concatenate([b[live], tb[keep]]).astype(np.float32).reshape(-1, 4)
    nc = np.concatenate([c[live], tc[keep]]).astype(np.int64)
    ni = np.concatenate([ids[live], ti[keep]]).astype(np.int64)
    nt = np.concatenate([np.full(int(live.sum()), p["ttl"]), tt[keep].astype(np.int64) - 1]).astype(np.int32)
    total, cap = len(ni), p["capacity"]
    new = {"boxes": nb[:cap], "classes": nc[:cap], "ids": ni[:cap], "ttl": nt[:cap], "m": min(total, cap), "next_id": next_id,
           "frames": int(st["frames"]) + 1, "dropped": int(st["dropped"]) + max(total - cap, 0)}
    return ids, new


class BoxTracker:
    """Ids that persist from frame to frame (association contract "track v1", include/ore_hip.h):

        tracker = BoxTracker(device)                       # capacity=1024, iou_thresh=0.6, ttl=8, class_aware=True, score_thresh=0.0
        ids = tracker.update(boxes, scores, classes, n_dev)   # int64 [rows] on the device, -1 for rows that are not live; no sync
        tracker.update(instances)                          # a device Instances: also sets instances.track_ids
        tracker.stats()                                    # one sync: {"tracks", "started", "frames", "dropped"}

    On a device the state is one buffer and an update is one launch of ore_track_update_fwd on the current stream.  The tracker keeps
    the event behind its last update, and an update on another stream waits for it on the device: several streams may share one
    tracker, and the frames are associated in the order of the calls.  device "cpu" (or host tensors' tracker) runs track_host instead:
    the same ids."""

    # what WideBoxTracker replaces: the limits, the three entry points, the workspace
    MAX_TRACKS = TRACK_MAX_TRACKS
    _STATE_BYTES, _RESET, _UPDATE = "ore_track_state_bytes", "ore_track_reset", "ore_track_update_fwd"
    _host_kw: dict = {}

    def _row_limit(self) -> int:
        return int(lib().ore_det_record_rows())

    def _workspace(self):
        """(address or None, bytes) of the update's workspace."""
        return None, 0

    def __init__(self, device, *, capacity: int = 1024, iou_thresh: float = 0.6, ttl: int = 8, class_aware: bool = True,
                 score_thresh: float = 0.0):
        self.params = _track_params(type(self).__name__, capacity, iou_thresh, ttl, class_aware, score_thresh, self.MAX_TRACKS)
        self.capacity = self.params["capacity"]
        self.device = torch.device(device)
        self._host = None if self.device.type == "cuda" else track_state_empty()
        self._event, self._event_stream = None, None
        if self._host is None:
            if self.device.index is None:
                self.device = torch.device("cuda", torch.cuda.current_device())
            nbytes = int(getattr(lib(), self._STATE_BYTES)(self.capacity))
            with torch.cuda.device(self.device):
                self._buf = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
                self._event = torch.cuda.Event()
            cap, o = self.capacity, _TRACK_HEADER
            self._hdr32, self._hdr64 = self._buf[:8].view(torch.int32), self._buf[8:32].view(torch.int64)
            self._boxes = self._buf[o:o + 16 * cap].view(torch.float32).view(cap, 4)
            self._classes = self._buf[o + 16 * cap:o + 24 * cap].view(torch.int64)
            self._ids = self._buf[o + 24 * cap:o + 32 * cap].view(torch.int64)
            self._ttl = self._buf[o + 32 * cap:o + 36 * cap].view(torch.int32)
        self.reset()

    def _ordered(self) -> int:
        """The current stream, made to follow the tracker's last update wherever that ran."""
        cur = _stream()
        if self._event_stream is not None and self._event_stream != cur:
            here = torch.cuda.current_stream(self.device)
            here.wait_event(self._event)
            self._buf.record_stream(here)
        return cur

    def _updated(self, cur: int) -> None:
        self._event.record(torch.cuda.current_stream(self.device))
        self._event_stream = cur

    def reset(self) -> None:
        """The empty state: no tracks, next_id 0, the counters 0.  Enqueued on the current stream (device) like an update."""
        if self._host is not None:
            self._host = track_state_empty()
            return
        with torch.cuda.device(self.device):
            cur = self._ordered()
            _chk(getattr(lib(), self._RESET)(_ptr(self._buf), self.capacity, cur), self._RESET)
            self._updated(cur)

    def update(self, boxes, scores=None, classes=None, n_dev=None, *, out=None):
        """The ids of one frame's rows, and the state moved on by that frame.  boxes [rows, 4] fp32, scores [rows] fp32, classes [rows]
        int64 or None; n_dev: an int32 device tensor holding the row count (read by the kernel), an int, or None: every row.  Or one
        Instances (pred_boxes, scores, optional pred_classes), whose track_ids is set as well.  out: an int64 [rows] tensor for the ids."""
        if scores is None and hasattr(boxes, "has") and hasattr(boxes, "pred_boxes"):
            inst = boxes
            if not inst.has("pred_boxes") or not inst.has("scores"):
                raise OreError("BoxTracker.update: the Instances needs pred_boxes and scores")
            b = inst.pred_boxes
            b = b.tensor if hasattr(b, "tensor") else torch.as_tensor(b)
            c = inst.pred_classes.long().contiguous() if inst.has("pred_classes") else None
            ids = self.update(b.float().contiguous().reshape(-1, 4), inst.scores.float().contiguous(), c, out=out)
            inst.track_ids = ids
            return ids
        if scores is None:
            raise OreError("BoxTracker.update takes boxes and scores, or one Instances")
        if self._host is not None:
            n = int(n_dev.reshape(-1)[0]) if torch.is_tensor(n_dev) else n_dev
            ids, self._host = track_host(self._host, boxes, scores, classes, n, **self.params, **self._host_kw)
            ids = torch.from_numpy(ids)
            if out is not None:
                out.copy_(ids)
                ids = out
            return ids
        dev = self.device
        rows = int(boxes.shape[0])
        if not all(torch.is_tensor(t) and t.device == dev for t in (boxes, scores) + (() if classes is None else (classes,))):
            raise OreError(f"BoxTracker.update: the rows are tensors on the tracker's device {dev}")
        if not (boxes.dtype == torch.float32 and scores.dtype == torch.float32 and (classes is None or classes.dtype == torch.int64) and
                boxes.dim() == 2 and boxes.shape[1] == 4 and scores.dim() == 1 and int(scores.shape[0]) == rows and
                (classes is None or (classes.dim() == 1 and int(classes.shape[0]) == rows)) and
                (rows == 0 or (boxes.stride(1) == 1 and boxes.stride(0) == 4)) and
                (rows <= 1 or (scores.stride(0) == 1 and (classes is None or classes.stride(0) == 1)))):
            raise OreError("BoxTracker.update: boxes [n, 4] fp32, scores [n] fp32, classes [n] int64, rows contiguous")
        if rows > self._row_limit():
            raise OreError(f"{type(self).__name__}.update: {rows} rows (at most {self._row_limit()})")
        n_host = rows
        if n_dev is not None and not torch.is_tensor(n_dev):
            n_host, n_dev = min(max(int(n_dev), 0), rows), None
        if n_dev is not None and not (n_dev.dtype == torch.int32 and n_dev.device == dev and n_dev.numel() >= 1):
            raise OreError("BoxTracker.update: n_dev is an int32 tensor on the tracker's device (the kernel reads its first element)")
        with torch.cuda.device(dev):
            if out is None:
                out = torch.empty(rows, dtype=torch.int64, device=dev)
            elif not (torch.is_tensor(out) and out.dtype == torch.int64 and out.device == dev and out.dim() == 1 and
                      int(out.shape[0]) == rows and (rows <= 1 or out.stride(0) == 1)):
                raise OreError("BoxTracker.update: out is a contiguous int64 tensor [n] on the tracker's device")
            p = self.params
            cur = self._ordered()
            ws, ws_bytes = self._workspace()
            _chk(getattr(lib(), self._UPDATE)(_ptr(self._buf), self.capacity, _ptr(boxes) if rows else None, _ptr(scores) if rows else None,
                                              _ptr(classes) if rows else None, _ptr(n_dev), n_host, rows, float(p["score_thresh"]),
                                              float(p["iou_thresh"]), p["ttl"], int(p["class_aware"]), _ptr(out) if rows else None, ws,
                                              ws_bytes, cur), self._UPDATE)
            self._updated(cur)
        return out

    def state(self) -> dict:
        """Views of the state: boxes [capacity, 4], classes, ids, ttl [capacity] (the first m are the list, the rest zeros) and m,
        next_id, frames, dropped as one-element tensors.  Device tensors: synchronise with the updates' stream before reading them."""
        if self._host is not None:
            return {k: (torch.from_numpy(np.array(v)) if isinstance(v, np.ndarray) else torch.tensor([v])) for k, v in self._host.items()}
        return {"boxes": self._boxes, "classes": self._classes, "ids": self._ids, "ttl": self._ttl, "m": self._hdr32[0:1],
                "next_id": self._hdr64[0:1], "frames": self._hdr64[1:2], "dropped": self._hdr64[2:3]}

    def state_host(self) -> dict:
        """The state as track_host's dict (numpy, the arrays cut at m); one explicit sync on a device."""
        if self._host is not None:
            return dict(self._host)
        self._event.synchronize()
        raw = self._buf.cpu().numpy()
        cap, o = self.capacity, _TRACK_HEADER
        m = int(raw[:4].view(np.int32)[0])
        nxt, frames, dropped = (int(v) for v in raw[8:32].view(np.int64))
        return {"boxes": raw[o:o + 16 * cap].view(np.float32).reshape(cap, 4)[:m].copy(), "classes": raw[o + 16 * cap:o + 24 * cap].view(np.int64)[:m].copy(),
                "ids": raw[o + 24 * cap:o + 32 * cap].view(np.int64)[:m].copy(), "ttl": raw[o + 32 * cap:o + 36 * cap].view(np.int32)[:m].copy(),
                "m": m, "next_id": nxt, "frames": frames, "dropped": dropped}

    def stats(self) -> dict:
        """{"tracks": the list's length, "started": ids issued so far (the particle count), "frames", "dropped"} as Python ints, after
        one explicit sync with the last update."""
        if self._host is not None:
            h = self._host
            return {"tracks": int(h["m"]), "started": int(h["next_id"]), "frames": int(h["frames"]), "dropped": int(h["dropped"])}
        self._event.synchronize()
        raw = self._buf[:_TRACK_HEADER].cpu().numpy()
        nxt, frames, dropped = (int(v) for v in raw[8:32].view(np.int64))
        return {"tracks": int(raw[:4].view(np.int32)[0]), "started": nxt, "frames": frames, "dropped": dropped}


class WideBoxTracker(BoxTracker):
    """BoxTracker for the rows of a tiled or TTA merge: up to 16384 tracks and 8192 rows per update (csrc/ore_track_wide.hip), the same
    contract "track v1", the same ids and the same state as BoxTracker wherever both take the input.

        tracker = WideBoxTracker(device)                   # capacity=4096, max_rows=2048, iou_thresh=0.6, ttl=8, ...
        ids = tracker.update(boxes, scores, classes, n_dev)   # two launches on the current stream, no sync

    max_rows is the most rows one update takes; it sizes the workspace (candidate bits of every track x row tile, the copy of the old
    list).  Everything else -- update, reset, state, state_host, stats, the Instances form, out=, n_dev, the ordering across streams
    -- is BoxTracker's.  device "cpu" runs track_host(wide=True)."""

    MAX_TRACKS = TRACK_WIDE_MAX_TRACKS
    _STATE_BYTES, _RESET, _UPDATE = "ore_track_wide_state_bytes", "ore_track_wide_reset", "ore_track_wide_update_fwd"
    _host_kw = {"wide": True}

    def __init__(self, device, *, capacity: int = 4096, max_rows: int = 2048, iou_thresh: float = 0.6, ttl: int = 8,
                 class_aware: bool = True, score_thresh: float = 0.0):
        if isinstance(max_rows, bool) or not isinstance(max_rows, (int, np.integer)) or not 0 <= max_rows <= TRACK_WIDE_MAX_ROWS:
            raise OreError(f"WideBoxTracker: max_rows {max_rows!r} (0 .. {TRACK_WIDE_MAX_ROWS})")
        self.max_rows = int(max_rows)
        self._ws = None
        super().__init__(device, capacity=capacity, iou_thresh=iou_thresh, ttl=ttl, class_aware=class_aware, score_thresh=score_thresh)
        if self._host is None:
            self._ws_bytes = int(lib().ore_track_wide_workspace_bytes(self.capacity, self.max_rows))
            with torch.cuda.device(self.device):
                self._ws = torch.empty(max(self._ws_bytes, 256), dtype=torch.uint8, device=self.device)

    def _row_limit(self) -> int:
        return self.max_rows

    def _workspace(self):
        return _ptr(self._ws), self._ws_bytes

    def _ordered(self) -> int:
        cur = super()._ordered()
        if self._ws is not None and self._event_stream is not None and self._event_stream != cur:
            self._ws.record_stream(torch.cuda.current_stream(self.device))
        return cur


# ---------------------------------------------------------------------------------------------------
# Heat maps of a detection pass (render contract "heatmap v1", include/ore_hip.h)
HEATMAP_MEAN = -1                                          # ORE_HEATMAP_MEAN
HEATMAP_MAX_LEVELS, HEATMAP_MAX_MAP_SIDE, HEATMAP_MAX_INPUT_SIDE, HEATMAP_MAX_STRIDE = 3, 4096, 8192, 128
HEATMAP_LUTS = ("jet", "gray")
_HEATMAP_TRANSFORMS = {None: 0, "none": 0, "sigmoid": 1}
_HEATMAP_NORMS = {"unit": 0, "max": 1}
_HEATMAP_ALPHA_MODES = {"constant": 0, "value": 1}
# the level buffers every pass -- an N-way pass included -- leaves as a batch of `B` images per level (the laterals are not among
# them: an N-way pass computes them for its one image only)
_HEATMAP_LEVEL_BUFFERS = ("p", "attn", "pos", "tower", "head")
_HEATMAP_WS: Dict[tuple, torch.Tensor] = {}
_HEATMAP_WS_MAX = 16


def heatmap_lut(name_or_table="jet", channel_order: str = "RGB") -> np.ndarray:
    """The colour table of a heat map: [256, 3] uint8 in `channel_order`.  "gray": (k, k, k).  "jet": with t = k / 255 the classic
    r = clamp(1.5 - |4t - 3|), g = clamp(1.5 - |4t - 2|), b = clamp(1.5 - |4t - 1|), each floor(255 c + 0.5) -- the package's own
    table (255 c + 0.5 = 383 - |4k - 765| is an integer, so the table is integer arithmetic), not matplotlib's bytes.  Any [256, 3]
    uint8 table, taken as RGB, is accepted.  channel_order "BGR" reverses the channels."""
    if channel_order not in ("RGB", "BGR"):
        raise OreError(f'heatmap_lut: channel_order is "RGB" or "BGR", not {channel_order!r}')
    if isinstance(name_or_table, str):
        k = np.arange(256, dtype=np.int64)
        if name_or_table == "gray":
            tab = np.stack([k, k, k], 1)
        elif name_or_table == "jet":
            tab = np.stack([np.clip(383 - np.abs(4 * k - c), 0, 255) for c in (765, 510, 255)], 1)
        else:
            raise OreError(f"heatmap_lut: the built-in tables are {', '.join(HEATMAP_LUTS)}; not {name_or_table!r}")
        tab = tab.astype(np.uint8)
    else:
        tab = name_or_table.detach().cpu().numpy() if torch.is_tensor(name_or_table) else np.asarray(name_or_table)
        if tab.dtype != np.uint8 or tab.shape != (256, 3):
            raise OreError(f"heatmap_lut: a table is [256, 3] uint8, got {tab.shape} {tab.dtype}")
    return np.ascontiguousarray(tab[:, ::-1] if channel_order == "BGR" else tab)


def _heatmap_style(alpha, alpha_mode) -> Tuple[int, int]:
    if isinstance(alpha, bool) or not isinstance(alpha, (int, np.integer)) or not 0 <= int(alpha) <= 255:
        raise OreError(f"heatmap: alpha is an integer 0 .. 255, not {alpha!r}")
    if alpha_mode not in _HEATMAP_ALPHA_MODES:
        raise OreError(f'heatmap: alpha_mode is "constant" or "value", not {alpha_mode!r}')
    return int(alpha), _HEATMAP_ALPHA_MODES[alpha_mode]


def _heatmap_geometry(levels_hw, strides, in_hw) -> None:
    if not 1 <= len(levels_hw) <= HEATMAP_MAX_LEVELS or len(strides) != len(levels_hw):
        raise OreError(f"heatmap: 1 .. {HEATMAP_MAX_LEVELS} levels, one stride each; got {len(levels_hw)} levels, {len(strides)} strides")
    for (h, w), s in zip(levels_hw, strides):
        if not (1 <= h <= HEATMAP_MAX_MAP_SIDE and 1 <= w <= HEATMAP_MAX_MAP_SIDE and 1 <= s <= HEATMAP_MAX_STRIDE):
            raise OreError(f"heatmap: level {h}x{w} at stride {s}: map sides 1 .. {HEATMAP_MAX_MAP_SIDE}, strides 1 .. {HEATMAP_MAX_STRIDE}")
    if in_hw is not None and not (1 <= in_hw[0] <= HEATMAP_MAX_INPUT_SIDE and 1 <= in_hw[1] <= HEATMAP_MAX_INPUT_SIDE):
        raise OreError(f"heatmap: model input {in_hw[0]}x{in_hw[1]}: sides 1 .. {HEATMAP_MAX_INPUT_SIDE}")


def heat_kind(kind: str) -> dict:
    """A heat-map kind as its parts: {"buffers": names, "channel": int or "mean", "transform", "norm"}.  "objectness": head3 .. head5
    channel 4 through the sigmoid, norm "unit"; "attention": attn3 .. attn5, channel mean, norm "max"; "<buffer>" or
    "<buffer>:<channel>": one level buffer (p, attn, pos, tower, head + 3 .. 5), its mean or that channel, norm "max"."""
    if kind == "objectness":
        return {"buffers": ("head3", "head4", "head5"), "channel": 4, "transform": "sigmoid", "norm": "unit"}
    if kind == "attention":
        return {"buffers": ("attn3", "attn4", "attn5"), "channel": "mean", "transform": None, "norm": "max"}
    m = re.fullmatch(r"(%s)([345])(?::(\d+))?" % "|".join(_HEATMAP_LEVEL_BUFFERS), kind) if isinstance(kind, str) else None
    if m is None:
        raise OreError(f'heat map kind {kind!r}: "objectness", "attention", or a level buffer "<name><3 .. 5>[:<channel>]" with a name of '
                       f"{', '.join(_HEATMAP_LEVEL_BUFFERS)}")
    if m[1] == "head" and m[3] is None:
        raise OreError(f'heat map kind {kind!r}: the head rows are [l, t, r, b, hm]; name a channel ("{kind}:4")')
    return {"buffers": (m[1] + m[2],), "channel": "mean" if m[3] is None else int(m[3]), "transform": None, "norm": "max"}


class HeatSource:
    """Where a heat map's scalars live: 1 .. 3 level buffers on one device, and what to take from them.

    buffers: per level a contiguous 2-D device tensor [batch * h * w, ld], fp32 or bf16 (all alike); levels: per level (h, w, stride);
    the `ch` channels of a row start at element coff (an int, or one per level).  channel: an index below ch, or "mean" (ch, ld and coff
    multiples of 4); transform None or "sigmoid"; norm "unit" or "max"; in_hw: the model-input size the maps were computed at; slot:
    the image of the batch.  Engine.heat_source builds one over the engine's own buffers: it then also holds the engine and the serial
    of the pass it views, and check() raises once the engine has begun a newer pass."""

    def __init__(self, buffers, levels, *, ch: int, coff=0, channel="mean", transform=None, norm: str = "max", in_hw, batch: int = 1,
                 slot: int = 0, kind: Optional[str] = None):
        levels = [(int(h), int(w), int(s)) for h, w, s in levels]
        self.hw, self.strides = [(h, w) for h, w, _ in levels], [s for _, _, s in levels]
        self.in_hw = (int(in_hw[0]), int(in_hw[1]))
        _heatmap_geometry(self.hw, self.strides, self.in_hw)
        buffers = list(buffers)
        if len(buffers) != len(levels):
            raise OreError(f"HeatSource: {len(buffers)} buffers for {len(levels)} levels")
        self.batch, self.slot, self.ch, self.kind = int(batch), int(slot), int(ch), kind
        if self.batch < 1 or not 0 <= self.slot < self.batch:
            raise OreError(f"HeatSource: batch slot {slot} of {batch}")
        self.coff = [int(c) for c in coff] if isinstance(coff, (list, tuple)) else [int(coff)] * len(levels)
        first = buffers[0]
        for t, (h, w) in zip(buffers, self.hw):
            if not (torch.is_tensor(t) and t.is_cuda and t.dim() == 2 and t.is_contiguous() and t.dtype in (torch.float32, torch.bfloat16)
                    and t.dtype == first.dtype and t.device == first.device and t.shape[0] == self.batch * h * w):
                raise OreError("HeatSource: a level buffer is a contiguous [batch * h * w, ld] fp32 or bf16 device tensor, all of one type and device")
        self.device, self.is_bf16 = first.device, first.dtype == torch.bfloat16
        self.ptrs, self.ld, self._keep = [t.data_ptr() for t in buffers], [int(t.shape[1]) for t in buffers], buffers
        self.engine, self.serial = None, None
        self._set_what(channel, transform, norm)

    def _set_what(self, channel, transform, norm) -> None:
        if transform not in _HEATMAP_TRANSFORMS or norm not in _HEATMAP_NORMS:
            raise OreError(f'HeatSource: transform None or "sigmoid", norm "unit" or "max"; not {transform!r}, {norm!r}')
        self.transform, self.norm = transform, norm
        if channel == "mean":
            if self.ch % 4 or any(v % 4 for v in self.ld + self.coff):
                raise OreError(f"HeatSource: the channel mean takes ch, ld and coff that are multiples of 4 (ch {self.ch}, ld {self.ld}, coff {self.coff})")
            self.channel = HEATMAP_MEAN
        elif isinstance(channel, (int, np.integer)) and not isinstance(channel, bool) and 0 <= int(channel) < self.ch:
            self.channel = int(channel)
        else:
            raise OreError(f'HeatSource: channel {channel!r}: "mean" or an index below {self.ch}')
        if any(c < 0 or c + self.ch > ld for c, ld in zip(self.coff, self.ld)):
            raise OreError(f"HeatSource: {self.ch} channels at {self.coff} do not fit ld {self.ld}")

    def check(self) -> None:
        """Raises when the engine behind this source has begun a newer pass: its buffers no longer hold what the source was taken of."""
        if self.engine is not None and self.engine.last_geometry()["serial"] != self.serial:
            raise OreError(f"heat source {self.kind!r} is stale: the engine has begun a newer pass (take heat_source() again after it)")


class HeatLevels:
    """The quantised level maps of a HeatSource (heatmap_levels): .maps = per level an [h, w] uint8 device tensor, .strides, .in_hw.
    The maps are views of a workspace the current stream owns: the next heatmap_levels on that stream overwrites them (stream order
    protects a draw that was enqueued before); .clone() what must outlive it."""

    def __init__(self, maps, strides, in_hw, source=None):
        self.maps, self.strides, self.in_hw, self.source = list(maps), [int(s) for s in strides], (int(in_hw[0]), int(in_hw[1])), source

    def __len__(self):
        return len(self.maps)

    def __getitem__(self, i):
        return self.maps[i]

    def __iter__(self):
        return iter(self.maps)


def heatmap_levels(source: HeatSource) -> HeatLevels:
    """Stages A + B of the render contract on the device (ore_heatmap_levels_fwd): the scalar of every location of every level of the
    source, quantised to uint8 -- the reference's predhm_l windows.  One launch (norm "unit") or two ("max") on the current stream, no
    host sync; the workspace is cached per stream."""
    if not isinstance(source, HeatSource):
        raise OreError("heatmap_levels takes a HeatSource (Engine.heat_source, or one built over your own level buffers)")
    source.check()
    n, dev = len(source.hw), source.device
    hw = _i32s(v for pair in source.hw for v in pair)
    with torch.cuda.device(dev):
        need = int(lib().ore_heatmap_workspace_bytes(n, hw))
        if need == 0:
            raise OreError(f"heatmap_levels: level sizes {source.hw} are out of range")
        key = (str(dev), _stream())                                  # per stream: two streams' maps must not share a workspace
        ws = _HEATMAP_WS.get(key)
        if ws is None or ws.numel() < need:
            if torch.cuda.is_current_stream_capturing():
                raise OreError("heatmap_levels: no workspace for this stream yet; run once outside the stream capture first")
            while ws is None and len(_HEATMAP_WS) >= _HEATMAP_WS_MAX:
                _HEATMAP_WS.pop(next(iter(_HEATMAP_WS)))
            ws = _HEATMAP_WS[key] = torch.empty(max(need, 1 << 18), dtype=torch.uint8, device=dev)
        p = source.ptrs + [None] * (3 - n)
        _chk(lib().ore_heatmap_levels_fwd(n, p[0], p[1], p[2], hw, _i32s(source.ld), _i32s(source.coff), source.ch, int(source.is_bf16),
                                          source.batch, source.slot, source.channel, _HEATMAP_TRANSFORMS[source.transform],
                                          _HEATMAP_NORMS[source.norm], _ptr(ws), ws.numel(), _stream()), "ore_heatmap_levels_fwd")
        maps = []
        for l, (h, w) in enumerate(source.hw):
            off = int(lib().ore_heatmap_level_offset(n, hw, l))
            maps.append(ws[off:off + h * w].view(h, w))
    return HeatLevels(maps, source.strides, source.in_hw, source)


def _heatmap_levels_arg(levels, in_hw):
    """heatmap_draw's / heatmap_host's `levels` as (maps, strides, in_hw): a HeatLevels, or a sequence of (map, stride)."""
    if isinstance(levels, HeatLevels):
        maps, strides, in_hw = levels.maps, levels.strides, levels.in_hw if in_hw is None else in_hw
    else:
        try:
            pairs = [(m, int(s)) for m, s in levels]
        except (TypeError, ValueError):
            raise OreError("heatmap: levels is a HeatSource, a HeatLevels or a sequence of (uint8 map [h, w], stride)") from None
        maps, strides = [m for m, _ in pairs], [s for _, s in pairs]
    if in_hw is None:
        raise OreError("heatmap: in_hw, the model-input size the maps were computed at, is needed with bare maps")
    if not all(getattr(m, "ndim", 0) == 2 for m in maps):
        raise OreError("heatmap: a level map is [h, w] uint8")
    in_hw = (int(in_hw[0]), int(in_hw[1]))
    _heatmap_geometry([(int(m.shape[0]), int(m.shape[1])) for m in maps], strides, in_hw)
    return maps, strides, in_hw


def heatmap_draw(frame_hwc_u8: torch.Tensor, levels, in_hw=None, *, out: Optional[torch.Tensor] = None, lut="jet", alpha: int = 128,
                 alpha_mode: str = "constant", channel_order: str = "RGB") -> torch.Tensor:
    """A heat map blended over a contiguous [h, w, 3] uint8 device frame (ore_heatmap_draw_fwd; stages C + D of "heatmap v1"), enqueued
    on the current stream, no host sync.  levels: a HeatSource (its maps are computed first: heatmap_levels), a HeatLevels, or a
    sequence of (uint8 device map [h_l, w_l], stride) with in_hw = the model-input size they belong to.  lut: "jet", "gray" or a
    [256, 3] uint8 RGB table; channel_order: the frame's.  alpha_mode "constant" blends every pixel with alpha, "value" with
    (alpha * v + 127) / 255.  out=None returns a fresh frame, out=frame draws in place.  A source whose engine has begun a newer
    pass raises."""
    f = frame_hwc_u8
    if not (torch.is_tensor(f) and f.is_cuda and f.dtype == torch.uint8 and f.dim() == 3 and f.shape[2] == 3 and f.is_contiguous()):
        raise OreError("heatmap_draw takes a contiguous [h, w, 3] uint8 device tensor")
    h, w = int(f.shape[0]), int(f.shape[1])
    if not (1 <= h <= OVERLAY_MAX_SIDE and 1 <= w <= OVERLAY_MAX_SIDE):
        raise OreError(f"heatmap_draw: frame {h}x{w}: sides 1 .. {OVERLAY_MAX_SIDE}")
    a, mode = _heatmap_style(alpha, alpha_mode)
    table = heatmap_lut(lut, channel_order)
    if isinstance(levels, HeatSource):
        levels = heatmap_levels(levels)
    elif isinstance(levels, HeatLevels) and levels.source is not None:
        levels.source.check()
    maps, strides, in_hw = _heatmap_levels_arg(levels, in_hw)
    dev = f.device
    for m in maps:
        if not (torch.is_tensor(m) and m.dtype == torch.uint8 and m.device == dev and m.is_contiguous()):
            raise OreError("heatmap_draw: a level map is a contiguous [h, w] uint8 tensor on the frame's device")
    if out is None:
        out = torch.empty_like(f)
    if not (out.is_cuda and out.dtype == torch.uint8 and out.shape == f.shape and out.is_contiguous() and out.device == dev):
        raise OreError("heatmap_draw: out is a contiguous uint8 device tensor of the frame's shape")
    with torch.cuda.device(dev):
        lut_d = _overlay_table_dev(dev, ("heatmap_lut", table.tobytes()), lambda: table)
        p = [_ptr(m) for m in maps] + [None] * (3 - len(maps))
        _chk(lib().ore_heatmap_draw_fwd(_ptr(f), _ptr(out), h, w, len(maps), p[0], p[1], p[2],
                                        _i32s(int(v) for m in maps for v in m.shape), _i32s(strides), in_hw[0], in_hw[1], _ptr(lut_d), a, mode,
                                        _stream()), "ore_heatmap_draw_fwd")
    return out


def sigmoid_host(x) -> np.ndarray:
    """ore_sigmoid of the kernels on the host, operation by operation (ore_sigmoid_host): fp32 in, fp32 out, the input's shape."""
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float32))
    y = np.empty_like(x)
    _chk(lib().ore_sigmoid_host(x.ctypes.data, y.ctypes.data, x.size), "ore_sigmoid_host")
    return y


def heatmap_levels_host(values, *, channel="mean", transform=None, norm: str = "max") -> List[np.ndarray]:
    """heatmap_levels on the host: values = per level an [h, w, ch] fp32 array (bf16 widened by the caller) -> per level [h, w] uint8.
    The channel mean keeps the kernel's order: four partial sums over c % 4 == j, ascending, (s0 + s1) + (s2 + s3), / ch."""
    if transform not in _HEATMAP_TRANSFORMS or norm not in _HEATMAP_NORMS:
        raise OreError(f'heatmap_levels_host: transform None or "sigmoid", norm "unit" or "max"; not {transform!r}, {norm!r}')
    scal = []
    with np.errstate(all="ignore"):
        for v in values:
            v = np.asarray(v, dtype=np.float32)
            if v.ndim != 3:
                raise OreError("heatmap_levels_host: a level is [h, w, ch] fp32")
            ch = v.shape[2]
            if channel == "mean":
                if ch % 4:
                    raise OreError(f"heatmap_levels_host: the channel mean takes a channel count that is a multiple of 4, not {ch}")
                s = np.zeros(v.shape[:2] + (4,), dtype=np.float32)
                for c in range(0, ch, 4):
                    s = s + v[:, :, c:c + 4]
                x = ((s[..., 0] + s[..., 1]) + (s[..., 2] + s[..., 3])) / np.float32(ch)
            elif isinstance(channel, (int, np.integer)) and not isinstance(channel, bool) and 0 <= int(channel) < ch:
                x = v[:, :, int(channel)]
            else:
                raise OreError(f'heatmap_levels_host: channel {channel!r}: "mean" or an index below {ch}')
            scal.append(sigmoid_host(x) if _HEATMAP_TRANSFORMS[transform] else np.ascontiguousarray(x))
        quant = lambda x: (np.fmin(np.fmax(x, np.float32(0)), np.float32(1)) * np.float32(255)).astype(np.int32).astype(np.uint8)
        if norm == "unit":
            return [quant(x) for x in scal]
        m = np.float32(max([np.float32(0)] + [np.fmax(x, np.float32(0)).max() for x in scal if x.size]))
        if not m > 0:
            return [np.zeros(x.shape, dtype=np.uint8) for x in scal]
        return [quant(x / m) for x in scal]


def _heatmap_taps(n_out: int, n_in: int, stride: int, length: int):
    """One axis of stage C, every output coordinate at once: (i0, i1, frac)."""
    t = np.arange(n_out, dtype=np.int64)
    u = np.clip(((2 * t + 1) * n_in * 256) // (2 * n_out * stride) - 128, 0, (length - 1) * 256)
    i0 = u >> 8
    return i0, np.minimum(i0 + 1, length - 1), u & 255


def heatmap_host(frame_hwc_u8, levels, in_hw=None, *, out=None, lut="jet", alpha: int = 128, alpha_mode: str = "constant",
                 channel_order: str = "RGB") -> np.ndarray:
    """heatmap_draw on the host: the vectorised numpy statement of stages C + D of "heatmap v1" (include/ore_hip.h), byte for byte
    what the kernel draws.  levels: a sequence of (uint8 map [h_l, w_l], stride) -- numpy arrays or CPU tensors -- with in_hw, or a
    HeatLevels (its maps are copied to the host).  Returns an [h, w, 3] uint8 array: a fresh one, or `out` (the frame itself: in place)."""
    as_np = lambda t: t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    frame = as_np(frame_hwc_u8)
    if frame.dtype != np.uint8 or frame.ndim != 3 or frame.shape[2] != 3:
        raise OreError(f"heatmap_host takes an [h, w, 3] uint8 frame, got {frame.shape} {frame.dtype}")
    h, w = frame.shape[:2]
    if not (1 <= h <= OVERLAY_MAX_SIDE and 1 <= w <= OVERLAY_MAX_SIDE):
        raise OreError(f"heatmap_host: frame {h}x{w}: sides 1 .. {OVERLAY_MAX_SIDE}")
    a, mode = _heatmap_style(alpha, alpha_mode)
    table = heatmap_lut(lut, channel_order).astype(np.int64)
    maps, strides, in_hw = _heatmap_levels_arg(levels, in_hw)
    maps = [as_np(m) for m in maps]
    if any(m.dtype != np.uint8 for m in maps):
        raise OreError("heatmap_host: a level map is [h, w] uint8")
    v = np.zeros((h, w), dtype=np.int64)
    for m, s in zip(maps, strides):
        q = m.astype(np.int64)
        y0, y1, fy = _heatmap_taps(h, in_hw[0], s, m.shape[0])
        x0, x1, fx = _heatmap_taps(w, in_hw[1], s, m.shape[1])
        top = q[y0][:, x0] * (256 - fx) + q[y0][:, x1] * fx
        bot = q[y1][:, x0] * (256 - fx) + q[y1][:, x1] * fx
        v = np.maximum(v, (top * (256 - fy)[:, None] + bot * fy[:, None] + 32768) >> 16)
    A = ((a * v + 127) // 255 if mode else np.full_like(v, a))[..., None]
    res = ((frame.astype(np.int64) * (255 - A) + table[v] * A + 127) // 255).astype(np.uint8)
    if out is None:
        return res
    img = out if out is frame_hwc_u8 or out is frame else as_np(out)
    img[...] = res
    return img


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


# The stride-2 gradient kernels address a tensor through 32-bit byte offsets and refuse one of 2 GiB or more (ORE_EINVAL).  The bindings
# therefore hand them the batch in groups of whole images whose tensors stay below this many bytes (a margin of 1 MiB for the rows a last
# step may name): one group -- one launch, as ever -- for everything but the support batch of a very large step.  A weight gradient adds the
# groups in order with beta = 1, so it stays deterministic; the order of that sum then depends on the grouping, i.e. on the shapes alone.
_S2_MAX_BYTES = (1 << 31) - (1 << 20)


def _s2_image_groups(B: int, *bytes_per_image: int) -> List[Tuple[int, int]]:
    nb = max(1, min(B, _S2_MAX_BYTES // max(bytes_per_image)))
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


class _Arr:
    def __init__(self, ptr, n, dt):
        tstr = {torch.float32: "<f4", torch.int64: "<i8", torch.int32: "<i4", torch.int16: "<i2"}[dt]
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": tstr, "data": (ptr, False), "version": 2}


def _from_ptr(ptr: int, n: int, dt, device) -> torch.Tensor:
    if dt == torch.bfloat16:                                  # not expressible in __cuda_array_interface__: view 16-bit integers
        return torch.as_tensor(_Arr(ptr, n, torch.int16), device=device).view(torch.bfloat16)
    return torch.as_tensor(_Arr(ptr, n, dt), device=device)
