"""CPU: the C-ABI library builds/loads, exports every function include/ore_hip.h declares with the header's prototype as its ctypes
signature, and every call of one in the repository's Python passes the declared number of arguments (no compute calls)."""
import ast
import ctypes
import glob
import os
import re
import subprocess
import tempfile

import pytest

from conftest import ROOT

# what each scalar type gcc prints stands for in ctypes; every pointer is a c_void_p
_PARAM = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t, "float": ctypes.c_float}
_RESULT = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "size_t": ctypes.c_size_t, "double": ctypes.c_double,
           "const char *": ctypes.c_char_p, "void": None}


def _lib():
    import orehip
    if not os.path.exists(orehip.LIB_PATH):
        orehip.build()
    return orehip.lib()


def _declared():
    """{name: (return type, [parameter types])} of every function ore_hip.h declares, as the C compiler reads the header (gcc
    -aux-info writes one normalised prototype per function, array parameters as pointers)."""
    with tempfile.TemporaryDirectory() as d:
        src, aux = os.path.join(d, "h.c"), os.path.join(d, "h.aux")
        with open(src, "w") as f:
            f.write('#include "ore_hip.h"\n')
        subprocess.check_call(["gcc", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-aux-info", aux, src])
        with open(aux) as f:
            lines = [l for l in f if "ore_hip.h:" in l]
    out = {}
    for l in lines:
        m = re.fullmatch(r"/\*.*?\*/ extern (.+?) ?\b(ore_\w+) \((.*)\);\s*", l)
        assert m, l
        out[m[2]] = (m[1], [] if m[3] == "void" else m[3].split(", "))
    return out


def test_header_symbols_exported():
    import orehip
    L = _lib()
    declared = _declared()
    assert len(declared) > 100, "no declarations parsed"
    assert sorted(orehip.SYMBOLS) == sorted(declared), set(orehip.SYMBOLS) ^ set(declared)
    for name, (ret, params) in declared.items():
        fn = getattr(L, name)
        want = [ctypes.c_void_p if "*" in p else _PARAM[p.replace("const ", "")] for p in params]
        assert list(fn.argtypes) == want, (name, fn.argtypes, params)
        assert fn.restype is _RESULT[ret], (name, fn.restype, ret)
    assert L.ore_version() >= 100


_SCOPES = (ast.Module, ast.FunctionDef, ast.AsyncFunctionDef, ast.Lambda, ast.ClassDef)


def _scope_nodes(scope):
    """The nodes of one scope, the bodies of nested functions and classes excluded."""
    for child in ast.iter_child_nodes(scope):
        if not isinstance(child, _SCOPES):
            yield child
            yield from _scope_nodes(child)


def _callees(e, declared):
    """The header functions an expression names: `<x>.ore_name`, or either branch of `a if c else b`."""
    if isinstance(e, ast.IfExp):
        return _callees(e.body, declared) | _callees(e.orelse, declared)
    return {e.attr} if isinstance(e, ast.Attribute) and e.attr in declared else set()


def _header_calls(tree, declared):
    """(name, call) for every call of a header function: `L.ore_name(...)`, `lib().ore_name(...)`, and `fn(...)` where the same scope
    assigns `fn = lib().ore_a if c else lib().ore_b` (once for each function it can be)."""
    for scope in ast.walk(tree):
        if not isinstance(scope, _SCOPES):
            continue
        nodes = list(_scope_nodes(scope))
        alias = {}
        for a in nodes:
            if isinstance(a, ast.Assign) and len(a.targets) == 1 and isinstance(a.targets[0], ast.Name):
                alias.setdefault(a.targets[0].id, set()).update(_callees(a.value, declared))
        for c in nodes:
            if isinstance(c, ast.Call):
                for name in alias.get(c.func.id, ()) if isinstance(c.func, ast.Name) else _callees(c.func, declared):
                    yield name, c


def test_header_calls_pass_declared_argument_count():
    """ctypes refuses too few arguments but passes extra ones on untyped, so the count of every call site is checked here -- for most
    of them the only evidence short of a GPU run.  Starred calls are left out."""
    arity = {name: len(params) for name, (_, params) in _declared().items()}
    files = glob.glob(os.path.join(ROOT, "*.py"))
    for d in ("faster-orefsdet_amd", "tests", "tools"):
        files += glob.glob(os.path.join(ROOT, d, "**", "*.py"), recursive=True)
    checked, bad = 0, []
    for path in sorted(files):
        with open(path) as f:
            tree = ast.parse(f.read(), path)
        for name, call in _header_calls(tree, arity):
            if any(isinstance(a, ast.Starred) for a in call.args):
                continue
            checked += 1
            if len(call.args) != arity[name]:
                bad.append(f"{os.path.relpath(path, ROOT)}:{call.lineno} {name}: {len(call.args)} arguments, {arity[name]} declared")
    assert checked > 150, checked
    assert not bad, bad


def test_unknown_header_type_is_an_error(tmp_path):
    """A prototype with a type the binding has no ctypes type for stops the load: no function is left untyped."""
    import orehip
    h = tmp_path / "h.h"
    h.write_text("int ore_f(int32_t n, double x);\n")
    with pytest.raises(orehip.OreError, match="double x"):
        orehip._prototypes(str(h))


def test_prototype_rejects_wrong_arguments():
    """Host-only function: too few arguments, or a float in an int32_t slot, fail in ctypes before the library is entered."""
    L = _lib()
    assert L.ore_packed_weight_floats(16, 16, 3, 3) == 16 * 9 * 16
    with pytest.raises(TypeError):
        L.ore_packed_weight_floats(*(16, 16, 3))          # starred: the call-shape check above would (rightly) flag it
    with pytest.raises(ctypes.ArgumentError):
        L.ore_packed_weight_floats(16, 16.0, 3, 3)


def test_pack_weight_host_only():
    import numpy as np
    import torch
    import orehip
    w = torch.arange(2 * 16 * 3 * 3, dtype=torch.float32).reshape(2, 16, 3, 3)
    p = orehip.pack_conv_weight(w).numpy().reshape(16, 9, 16)
    assert np.array_equal(p[1, 4], w[1, :, 1, 1].numpy())   # [n][tap][cin]
    assert (p[2:] == 0).all()


def test_struct_sizes_match_header():
    """ctypes mirrors of the descriptor structs must have the C layout (checked against a tiny C program)."""
    import orehip
    src = '#include <stdio.h>\n#include "ore_hip.h"\nint main(){printf("%zu %zu %zu", sizeof(ore_conv_desc), sizeof(ore_detect_desc), sizeof(ore_model_cfg));return 0;}'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        a, b, c = (int(x) for x in subprocess.check_output([os.path.join(d, "s")]).split())
    assert (a, b, c) == (ctypes.sizeof(orehip.ConvDesc), ctypes.sizeof(orehip.DetectDesc), ctypes.sizeof(orehip.ModelCfg))
