"""The C ABI of libore_hip.so: paths, the ctypes structs, the header's prototypes, the loader and the per-launch helpers."""

from __future__ import annotations

import ctypes as C
import os
import re
import subprocess
from typing import Dict, List, Optional, Tuple

import torch

import orehip          # LIB_PATH lives on the package, where callers rebind it: read as orehip.LIB_PATH at call time


_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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
    return orehip.LIB_PATH


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
        path = orehip.LIB_PATH                                # callers point it elsewhere before the first lib()
        if not os.path.exists(path):
            raise OreError(f"{path} not found: build it with `make -C {CSRC}` (there is no CPU fallback)")
        L = C.CDLL(path)
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


class _Arr:
    def __init__(self, ptr, n, dt):
        tstr = {torch.float32: "<f4", torch.int64: "<i8", torch.int32: "<i4", torch.int16: "<i2"}[dt]
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": tstr, "data": (ptr, False), "version": 2}


def _from_ptr(ptr: int, n: int, dt, device) -> torch.Tensor:
    if dt == torch.bfloat16:                                  # not expressible in __cuda_array_interface__: view 16-bit integers
        return torch.as_tensor(_Arr(ptr, n, torch.int16), device=device).view(torch.bfloat16)
    return torch.as_tensor(_Arr(ptr, n, dt), device=device)
