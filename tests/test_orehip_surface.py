"""CPU: the orehip package keeps its surface while the binding moves from one file into per-subsystem submodules.  Every name the
one-file binding defined (tests/golden/orehip_surface.txt, an ast walk of that file) is still an attribute of the package, is defined
in one file only, and where that file is a submodule is the submodule's own object; the names that callers rebind on the package are read through the package at call time; and the functions that tests replace on
the package have no caller inside the binding.  Nothing here loads the library or touches a GPU."""
import ast
import glob
import os
import sys

import pytest

from conftest import PKG, ROOT

import orehip

ORE_DIR = os.path.join(PKG, "orehip")
REBOUND = ("LIB_PATH", "ROI_BWD_DETERMINISTIC", "ROI_BWD_MODE", "_S2_MAX_BYTES")          # assigned on the package by tests and tools
PATCHED = ("conv2d_wgrad", "dw3x3_wgrad", "centernet_targets")                            # replaced on the package by tests
CACHES = ("_WS", "_WGWS", "_PACK_TABLES", "_RESIZE_TABLES", "_RESIZE_WS", "_SUPPORT_BUF", "_OVERLAY_TABLES", "_OVERLAY_WS", "_HEATMAP_WS")


def _tree(path):
    with open(path) as f:
        return ast.parse(f.read(), path)


def _top_names(tree):
    """The names a module defines at its top level: def, class, and the targets of = and of annotated assignments."""
    out = []
    for n in tree.body:
        if isinstance(n, (ast.FunctionDef, ast.ClassDef)):
            out.append(n.name)
        elif isinstance(n, ast.Assign):
            out += [e.id for t in n.targets for e in ast.walk(t) if isinstance(e, ast.Name)]
        elif isinstance(n, ast.AnnAssign):
            out.append(n.target.id)
    return out


def _files(binding_only=False):
    """{module name: path} of the package's files; binding_only leaves the autograd layers out."""
    files = {os.path.basename(p)[:-3]: p for p in sorted(glob.glob(os.path.join(ORE_DIR, "*.py")))}
    return {m: p for m, p in files.items() if not (binding_only and m.startswith("autograd"))}


@pytest.fixture(scope="module")
def surface():
    with open(os.path.join(ROOT, "tests", "golden", "orehip_surface.txt")) as f:
        names = f.read().split()
    assert len(names) == 248 and len(set(names)) == 248 and sum(n.startswith("_") for n in names) == 79
    return names


def test_every_name_is_still_on_the_package(surface):
    missing = [n for n in surface if not hasattr(orehip, n)]
    assert not missing, missing
    for n in CACHES:
        assert n in surface and type(getattr(orehip, n)) is dict, n


def test_package_names_are_the_submodules_objects(surface):
    """A re-export that copied or wrapped would split a cache in two, or hide a replaced function from its callers."""
    homes = {}                                                   # name -> the files that define it: one each, or there are two copies
    for mod, path in _files(binding_only=True).items():
        for n in set(_top_names(_tree(path))) & set(surface):
            homes.setdefault(n, []).append(mod)
    assert all(len(homes[n]) == 1 for n in surface), {n: m for n, m in homes.items() if len(m) != 1}
    assert all(homes[n] == ["__init__"] for n in REBOUND)
    # the names whose move is the hazard have moved: the caches read by identity, the functions replaced on the package, and the
    # readers of the rebound names (only _WS, the forward convs' workspace, is still with them in __init__.py)
    moved = set(CACHES) - {"_WS"} | set(PATCHED) | {"lib", "build", "roi_align_bwd", "_s2_image_groups"}
    assert not [n for n in moved if homes[n] == ["__init__"]], sorted(n for n in moved if homes[n] == ["__init__"])
    checked, own_rebinds = 0, set()
    for mod, path in _files(binding_only=True).items():
        if mod == "__init__":
            continue
        tree = _tree(path)
        # a name its own module rebinds (`global` in a function) has no one object: the package keeps the value at import
        rebinds = {g for n in ast.walk(tree) if isinstance(n, ast.Global) for g in n.names}
        own_rebinds |= rebinds
        sub = sys.modules["orehip." + mod]
        for n in _top_names(tree):
            if n in surface and n not in rebinds:
                assert getattr(orehip, n) is getattr(sub, n), (mod, n)
                checked += 1
    assert own_rebinds == {"_lib", "_OVERLAY_ATLAS"}, own_rebinds              # lib() and overlay_atlas(): built once, on first use
    in_submodules = [n for n in surface if homes[n] != ["__init__"]]
    assert checked == len(in_submodules) - len(own_rebinds), (checked, len(in_submodules))
    assert checked >= len(surface) - len(REBOUND) - len(own_rebinds) - 37, checked       # 37: the ops and engine names still in __init__.py


def test_defined_names_cover_the_list(surface):
    defined = set()
    for path in _files(binding_only=True).values():
        defined.update(_top_names(_tree(path)))
    assert not set(surface) - defined, sorted(set(surface) - defined)


def test_reexports_are_explicit():
    for n in ast.walk(_tree(os.path.join(ORE_DIR, "__init__.py"))):
        assert not (isinstance(n, ast.ImportFrom) and any(a.name == "*" for a in n.names)), "import * drops the underscore names"


def test_s2_max_bytes_is_read_at_call_time(monkeypatch):
    assert orehip._s2_image_groups(5, 400) == [(0, 5)]
    monkeypatch.setattr(orehip, "_S2_MAX_BYTES", 1000)
    assert orehip._s2_image_groups(5, 400) == [(0, 2), (2, 4), (4, 5)]


def test_lib_path_is_read_at_call_time(monkeypatch, tmp_path):
    nowhere = str(tmp_path / "no_such_libore_hip.so")
    monkeypatch.setattr(sys.modules[orehip.lib.__module__], "_lib", None)       # as before the first lib(); put back after the test
    monkeypatch.setattr(orehip, "LIB_PATH", nowhere)
    with pytest.raises(orehip.OreError) as e:
        orehip.lib()
    assert nowhere in str(e.value)


def test_rebound_names_live_on_the_package_alone():
    """roi_align_bwd reads both ROI_BWD names as attributes of orehip, and no file beside __init__.py holds any of the four as a bare
    name: not assigned (a second copy), not read (a value frozen at import)."""
    home = sys.modules[orehip.roi_align_bwd.__module__]
    assert home is not orehip
    fn = next(n for n in _tree(home.__file__).body if isinstance(n, ast.FunctionDef) and n.name == "roi_align_bwd")
    reads = {n.attr for n in ast.walk(fn) if isinstance(n, ast.Attribute) and isinstance(n.ctx, ast.Load)
             and isinstance(n.value, ast.Name) and n.value.id == "orehip"}
    assert {"ROI_BWD_DETERMINISTIC", "ROI_BWD_MODE"} <= reads, reads
    top = _top_names(_tree(os.path.join(ORE_DIR, "__init__.py")))
    assert all(top.count(n) == 1 for n in REBOUND), top
    for mod, path in _files().items():
        if mod == "__init__":
            continue
        for n in ast.walk(_tree(path)):
            assert not (isinstance(n, ast.Name) and n.id in REBOUND), (mod, n.id, n.lineno)
            assert not (isinstance(n, ast.Attribute) and n.attr in REBOUND and not isinstance(n.ctx, ast.Load)), (mod, n.attr, n.lineno)
            assert not (isinstance(n, ast.Global) and set(n.names) & set(REBOUND)), (mod, n.lineno)


def test_patched_functions_have_no_caller_inside_the_binding():
    """tests wrap orehip.conv2d_wgrad / dw3x3_wgrad / centernet_targets and expect every call to pass the wrapper: the autograd layers
    call through orehip.<name>, and the binding itself must not call them by their bare names."""
    for mod, path in _files(binding_only=True).items():
        for n in ast.walk(_tree(path)):
            assert not (isinstance(n, ast.Call) and isinstance(n.func, ast.Name) and n.func.id in PATCHED), (mod, n.func.id, n.lineno)
