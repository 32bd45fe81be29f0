"""Every launch form of the conv data gradient (ore_conv2d_fwd over dZ with the data-gradient weight layout) against float64.

Each trained conv / linear layer gets dX from ore_conv2d_fwd on dZ [B,H,W,Cout16] with the weights packed [Cin16][flipped tap][Cout16]
(and, for the 3x3 layers the Winograd covers, their Winograd form).  The plan picks one of about a dozen launchers; the test hook
orehip.conv_last_launch() names the one that ran and its split-K S.  tests/dgrad_ref.py computes dX in float64 and holds every
element to 2 d u (A + E) and every 16-row x 16-channel block to an rms of C_S u sqrt(d), with d from the launcher and S (its
docstring derives both; tests/test_dgrad_host.py shows they pass an fp32 emulation and fail the faults they are there to catch).
The operands carry per-channel scales from 1e-3 to 1e3, so the channels of dX span about 1e6 in magnitude.

Launchers and how this module reaches them:
  automatic plan (the shape matrix and edge classes; test_reached_cells pins the exact set): fp32 k_conv3x3_wino, k_conv3x3_wino_nu,
    k_conv3x3_patch<4>, k_conv_kd, k_conv_gs, k_conv_kw, k_conv_igemm; bf16 k_conv3x3_patch<4>, k_conv_kw, k_conv_igemm.  The
    production replay lands on the launcher each recorded call ran (forward calls add k_conv_gd); its stride-2 and input-affine calls
    and every returned column sum are held to the forward contract of tests/fwdconv_ref.py;
  forced through ore_conv_set_plan_override at a data-gradient shape (test_forced_launcher), the hook confirming each:
    k_conv3x3_patch<8>, k_conv3x3_patch_db, k_conv3x3_ws<2,64>, k_conv3x3_ws<2,128>, k_conv_gd, k_conv_rf, and k_conv3x3_patch<4>,
    k_conv_kw, k_conv_gs, k_conv_igemm at other shapes; explicit split-K 2, 3, 7, 17 on k_conv_igemm (test_explicit_splitk).

ORE_DGRAD_LOG=<file>: append the worst hard-bound and rms ratios per (mode, launcher) to that file."""
import contextlib
import ctypes as C
import os

import pytest
import torch

import dgrad_ref as DR
import fwdconv_ref as FR

pytestmark = pytest.mark.gpu

NAN = float("nan")
_RATIOS = {}        # (mode, launcher) -> [worst hard, worst rms, checks]
_CELLS = set()      # (mode, launcher) reached by the automatic plan in the matrix / edge classes


@pytest.fixture(scope="module")
def oh():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import orehip
    orehip.lib()
    return orehip


class _Plans(list):
    bm = 0          # rows of a block tile in the last plan (the row tiles of the column sums)


@contextlib.contextmanager
def _planned(oh):
    """Each ore_conv2d_fwd call made inside the block first asks ore_conv_plan about the same descriptor; the answers, in order."""
    L = oh.lib()
    real, plans = L.ore_conv2d_fwd, _Plans()

    def fwd(d, stream):
        pl = oh.ConvPlan()
        assert L.ore_conv_plan(d, 0, None, None, 0, C.byref(pl)) == 0, L.ore_last_error()
        plans.append((oh.CONV_LAUNCHERS[pl.launcher], pl.splitk))
        plans.bm = pl.bm
        return real(d, stream)

    L.ore_conv2d_fwd = fwd
    try:
        yield plans
    finally:
        L.ore_conv2d_fwd = real


@pytest.fixture(scope="module", autouse=True)
def ratio_report(oh):
    yield
    lines = [f"{m:5s} {l:26s} max hard {h:.3e}  max rms {r:.3e}  ({n} checks)" for (m, l), (h, r, n) in sorted(_RATIOS.items())]
    print("\n" + "\n".join(lines))
    log = os.environ.get("ORE_DGRAD_LOG")
    if log and lines:
        with open(log, "a") as f:
            f.write("\n".join(lines) + "\n")


@pytest.fixture(params=["fp32", "bf16"])
def mode(oh, request):
    prev = oh.set_conv_precision(request.param)
    yield request.param
    oh.set_conv_precision(prev)


def _subset(B, H, W, k, work):
    """(images, rows) of the output the float64 reference computes: everything unless the launch is large; then all rows of the
    first and last image plus a strided sample of the others (k = 3), or a strided sample of the rows (1x1, every row stands alone)."""
    if work < 4e9:
        return None, None
    if k == 1:
        M = B * H * W
        idx = torch.cat([torch.arange(0, 4096), torch.arange(4096, M - 4096, max(1, (M - 8192) // 8192) * 16 + 1), torch.arange(M - 4096, M)])
        return None, idx[idx < M].unique()
    if B > 2:
        imgs = sorted({0, B - 1} | set(range(1, B - 1, max(1, B // 6))))
        return imgs, None
    return None, None


def _record(mode, launcher, r):
    h0, r0, n0 = _RATIOS.get((mode, launcher), (0.0, 0.0, 0))
    _RATIOS[(mode, launcher)] = (max(h0, r["hard"]), max(r0, r["rms"]), n0 + 1)


def _launch_dgrad(oh, dz, w, k, *, wino=True, splitk=0, workspace=None, out=None):
    """The data-gradient call exactly as orehip/autograd.py's _conv_backward makes it (packed(w, dgrad=True), packed_wino(w, True))."""
    Cin = w.shape[1]
    pw = oh.pack_conv_weight_dev(w.cuda().contiguous(), dgrad=True)
    ww = None
    if wino and k == 3 and oh.winograd_covers(Cin, dz.shape[-1]):
        ww = oh.winograd_weight(pw, Cin, dz.shape[-1])
    got = oh.conv2d(dz.cuda(), pw, Cin, k, 1, k // 2, w_wino=ww, splitk=splitk, workspace=workspace, out=out)
    return got, oh.conv_last_launch()


def _check(oh, mode, dz, w, k, got, launch, what, *, images=None, rows=None):
    name, S = launch
    bf16 = mode == "bf16"
    B, H, W, cl = dz.shape
    dev = "cuda" if B * H * W * cl * w.shape[1] * k * k > 2e7 else "cpu"
    wino = name.startswith("k_conv3x3_wino")
    ref, mag = DR.dgrad_ref(dz, w, bf16=bf16, device=dev, images=images, rows=rows, wino=wino)
    d = DR.depth(k * k * cl, S, wino_cin=cl if wino else None)
    g = got.reshape(B, H, W, -1)
    if images is not None:
        g = g[images]
    g = g.reshape(-1, g.shape[-1])
    if rows is not None:
        g = g[rows.to(g.device)]
    r = DR.dgrad_check(g, ref, mag, d)
    _record(mode, name, r)
    assert r["hard"] <= 1 and r["rms"] <= 1, (what, launch, r)
    return r


# ---- layout ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cout", [2, 5, 16, 96, 112, 128])
@pytest.mark.parametrize("k", [1, 3])
def test_dgrad_pack_layout(oh, Cout, k):
    """pack_conv_weight_dev(w, dgrad=True) and the dgrad jobs of pack_conv_weights_multi equal the restatement bit for bit."""
    g = torch.Generator().manual_seed(Cout + k)
    jobs = []
    for Cin in (16, 80, 128):
        w = torch.randn(Cout, Cin, k, k, generator=g)
        want = DR.pack_dgrad(w)
        got = oh.pack_conv_weight_dev(w.cuda(), dgrad=True)
        assert torch.equal(got.cpu(), want), (Cout, Cin, k)
        out = torch.full_like(got, NAN)
        jobs.append((w.cuda().contiguous(), True, out, want))
    oh.pack_conv_weights_multi([(w, d, o) for w, d, o, _ in jobs])
    for _, _, o, want in jobs:
        assert torch.equal(o.cpu(), want)


# ---- shape matrix: one class per trained layer, batch 1 and 16, automatic plan --------------------------------------------------
@pytest.mark.parametrize("lab,B,H,W,Cout,Cin,k", DR.matrix() + [("edge",) + e for e in DR.EDGES])
def test_dgrad_matrix(oh, mode, lab, B, H, W, Cout, Cin, k):
    dz, w = DR.scaled_operands(B, H, W, Cout, Cin, k, seed=B * H * W + 7 * Cin + Cout + k, device="cuda")
    got, launch = _launch_dgrad(oh, dz, w, k)
    _CELLS.add((mode, launch[0]))
    images, rows = _subset(B, H, W, k, B * H * W * DR.c16(Cout) * Cin * k * k)
    _check(oh, mode, dz, w, k, got, launch, (lab, B, H, W, Cout, Cin, k), images=images, rows=rows)
    got2, launch2 = _launch_dgrad(oh, dz, w, k)
    assert launch2 == launch and torch.equal(got, got2), "two identical launches differ"


def test_reached_cells():
    """The exact set of (mode, launcher) cells the matrix and edge classes reach on the automatic plan (runs after them)."""
    want = EXPECTED_CELLS
    if not _CELLS:
        pytest.fail("the matrix did not run before this test")
    print("\ncells reached:", sorted(_CELLS))
    assert _CELLS == want, (sorted(_CELLS - want), sorted(want - _CELLS))


EXPECTED_CELLS = {("fp32", "k_conv3x3_wino"), ("fp32", "k_conv3x3_wino_nu"), ("fp32", "k_conv3x3_patch<4>"), ("fp32", "k_conv_kd"),
                  ("fp32", "k_conv_gs"), ("fp32", "k_conv_kw"), ("fp32", "k_conv_igemm"),
                  ("bf16", "k_conv3x3_patch<4>"), ("bf16", "k_conv_kw"), ("bf16", "k_conv_igemm")}


# ---- forced launchers ---------------------------------------------------------------------------------------------------------
# (launcher, overrides, (B, H, W, Cout, Cin, k) of the layer, modes)
FORCED = [
    ("k_conv3x3_patch<4>", [(-14, 0), (-2, 0), (-1, 4)], (2, 20, 20, 96, 128, 3), ("fp32", "bf16")),
    ("k_conv3x3_patch<8>", [(-14, 0), (-2, 0), (-1, 8)], (2, 20, 20, 96, 128, 3), ("fp32",)),
    ("k_conv3x3_patch_db", [(-14, 0), (-2, 0), (-1, 16)], (2, 20, 20, 96, 64, 3), ("fp32",)),
    ("k_conv3x3_ws<2,64>", [(-14, 0), (-2, 0), (-1, 102)], (2, 20, 20, 64, 64, 3), ("fp32", "bf16")),
    ("k_conv3x3_ws<2,128>", [(-14, 0), (-2, 0), (-1, 102)], (2, 20, 20, 128, 128, 3), ("fp32",)),
    ("k_conv_kw", [(-2, 2), (-10, 0), (-12, 0), (-14, 0)], (3, 13, 11, 112, 112, 3), ("fp32", "bf16")),
    ("k_conv_kw", [(-2, 2), (-10, 0), (-12, 0), (-14, 0)], (1, 20, 20, 512, 720, 1), ("fp32", "bf16")),
    ("k_conv_gs", [(-14, 0), (-4, 64, 64)], (1, 40, 40, 384, 544, 1), ("fp32",)),
    ("k_conv_gd", [(-12, 0), (-15, 64, 128, 4)], (1, 80, 80, 128, 256, 1), ("fp32", "bf16")),
    ("k_conv_rf", [(-14, 0), (-12, 0), (-10, 2)], (1, 16, 20, 128, 128, 3), ("fp32",)),
    ("k_conv_igemm", [(-14, 0), (-2, 0), (-1, 0)], (2, 15, 17, 128, 128, 3), ("fp32", "bf16")),
    ("k_conv_igemm", [(-14, 0), (-2, 0), (-1, 0)], (1, 1, 300, 4, 128, 1), ("fp32", "bf16")),
]


@pytest.mark.parametrize("i,mode_", [(i, m) for i, f in enumerate(FORCED) for m in f[3]])
def test_forced_launcher(oh, i, mode_):
    """Each launcher the automatic plan does not pick for a data-gradient call, forced at a data-gradient shape in every mode it has a
    build for; the hook confirms it ran."""
    name, overrides, (B, H, W, Cout, Cin, k), _ = FORCED[i]
    prev = oh.set_conv_precision(mode_)
    try:
        with oh.conv_overrides(*FORCED[i][1]):
            _forced(oh, i, mode_)
    finally:
        oh.set_conv_precision(prev)


def _forced(oh, i, mode):
    name, overrides, (B, H, W, Cout, Cin, k), _ = FORCED[i]
    dz, w = DR.scaled_operands(B, H, W, Cout, Cin, k, seed=50 + i, device="cuda")
    with _planned(oh) as plans:
        got, launch = _launch_dgrad(oh, dz, w, k, wino=False)
    assert launch[0] == name, (FORCED[i], launch)
    assert plans == [launch], (FORCED[i], plans, launch)
    _check(oh, mode, dz, w, k, got, launch, FORCED[i])
    got2, launch2 = _launch_dgrad(oh, dz, w, k, wino=False)
    assert launch2 == launch and torch.equal(got, got2), "two identical launches differ"


# ---- split-K ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [2, 3, 7, 17])
@pytest.mark.parametrize("shape", [(1, 12, 10, 7616, 64, 1), (1, 12, 10, 384, 544, 1), (2, 9, 7, 112, 112, 3)])
def test_explicit_splitk(oh, mode, S, shape):
    """An explicit split-K runs k_conv_igemm with S slabs of ceil(steps / S) steps (the plan evens them out: S' = ceil(steps /
    ceil(steps / S))).  Over 7616 channels of dZ (119 steps of 4 chunks) every requested S is exact; d is taken from the S that ran."""
    B, H, W, Cout, Cin, k = shape
    dz, w = DR.scaled_operands(B, H, W, Cout, Cin, k, seed=S + k, device="cuda")
    got, launch = _launch_dgrad(oh, dz, w, k, splitk=S)
    assert launch[0] == "k_conv_igemm" and 1 < launch[1] <= S, launch
    if Cout == 7616:
        assert launch[1] == S, launch
    _check(oh, mode, dz, w, k, got, launch, ("splitk", S, shape))
    got2, _ = _launch_dgrad(oh, dz, w, k, splitk=S)
    assert torch.equal(got, got2), "two identical split-K launches differ"


def test_explicit_splitk_small_workspace_is_refused(oh):
    B, H, W, Cout, Cin, k = 1, 12, 10, 384, 544, 1
    dz, w = DR.scaled_operands(B, H, W, Cout, Cin, k, seed=3, device="cuda")
    out = torch.full((B, H, W, Cin), NAN, device="cuda")
    ws = torch.zeros(4096 + 100, device="cuda")
    with pytest.raises(oh.OreError) as e:
        _launch_dgrad(oh, dz, w, k, splitk=7, workspace=ws, out=out)
    assert "(-12)" in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert bool(out.isnan().all()), "a refused launch wrote its output"


def test_automatic_split_falls_back_with_a_small_workspace(oh, mode):
    """The automatic k_conv_igemm plan splits K on a small, deep launch (>= 48 steps, < 256 blocks: a 3x3 over 384 dZ channels on
    an 8x8 map); with a workspace too small for the split it runs S = 1."""
    with oh.conv_overrides((-14, 0), (-2, 0), (-1, 0)):
        _automatic_split(oh, mode)


def _automatic_split(oh, mode):
    B, H, W, Cout, Cin, k = 1, 8, 8, 384, 112, 3
    dz, w = DR.scaled_operands(B, H, W, Cout, Cin, k, seed=4, device="cuda")
    got, launch = _launch_dgrad(oh, dz, w, k)
    assert launch[0] == "k_conv_igemm" and launch[1] > 1, launch
    _check(oh, mode, dz, w, k, got, launch, "automatic split")
    got1, launch1 = _launch_dgrad(oh, dz, w, k, workspace=torch.zeros(4096 + 16, device="cuda"))
    assert launch1 == ("k_conv_igemm", 1), launch1
    _check(oh, mode, dz, w, k, got1, launch1, "automatic split, small workspace")


# ---- backward chains against float64 autograd --------------------------------------------------------------------------------
def _chain_ref(x, w, dy, y, scale, relu):
    """float64 dX of conv(x, w) * scale (+ shift) (+ ReLU), with the ReLU mask taken from the product's own forward output y."""
    dz = dy.double()
    if relu:
        dz = dz * (y.double() > 0)
    if scale is not None:
        dz = dz * scale.double()
    return dz


@pytest.mark.parametrize("form", ["bn_relu", "bias", "bias_relu", "cout5", "topdown_add"])
def test_convfn_backward_chain(oh, mode, form):
    from orehip import autograd as A
    g = torch.Generator(device="cuda").manual_seed(["bn_relu", "bias", "bias_relu", "cout5", "topdown_add"].index(form))
    B, H, W, Cin, Cout, k = (2, 20, 20, 128, 128, 3) if form != "topdown_add" else (2, 21, 19, 128, 128, 1)
    if form == "cout5":
        Cout = 5
    x = (torch.randn(B, H, W, Cin, generator=g, device="cuda")).requires_grad_(True)
    _, w = DR.scaled_operands(1, 1, 1, Cout, Cin, k, seed=7, device="cuda")
    w = w.requires_grad_(True)
    scale = shift = bias = add = None
    relu = form in ("bn_relu", "bias_relu", "cout5")
    if form == "bn_relu":
        scale, shift = torch.rand(Cout, generator=g, device="cuda") + 0.5, torch.randn(Cout, generator=g, device="cuda")
    else:
        bias = torch.randn(Cout, generator=g, device="cuda").requires_grad_(True)
    if form == "topdown_add":
        add = torch.randn(B, (H + 1) // 2, (W + 1) // 2, Cout, generator=g, device="cuda").requires_grad_(True)
    y = A.conv(x, w, bias, scale, shift, relu, add)
    dy = torch.randn(y.shape, generator=g, device="cuda") * 10.0 ** (torch.rand(Cout, generator=g, device="cuda") * 6 - 3)
    gx, = torch.autograd.grad(y, [x], dy, retain_graph=add is not None)
    launch = oh.conv_last_launch()
    dz = torch.zeros(B, H, W, DR.c16(Cout), device="cuda")
    dz[..., :Cout] = _chain_ref(x, w, dy, y.detach(), scale, relu).float()        # fp32 dZ the product hands its dgrad call
    _check(oh, mode, dz, w.detach(), k, gx, launch, form)
    if add is not None:
        gadd, = torch.autograd.grad(y, [add], dy)
        want = dy.double().reshape(B, H, W, Cout)
        want = torch.nn.functional.pad(want, (0, 0, 0, W % 2, 0, H % 2))
        want = want.reshape(B, (H + 1) // 2, 2, (W + 1) // 2, 2, Cout).sum((2, 4))
        assert torch.allclose(gadd.double(), want, rtol=1e-6, atol=1e-6 * float(want.abs().max()))


@pytest.mark.parametrize("Cout", [2, 4])
def test_linear_backward_chain(oh, mode, Cout):
    from orehip import autograd as A
    g = torch.Generator(device="cuda").manual_seed(Cout)
    x = torch.randn(2048, 128, generator=g, device="cuda").requires_grad_(True)
    _, w = DR.scaled_operands(1, 1, 1, Cout, 128, 1, seed=Cout, device="cuda")
    wl = w.reshape(Cout, 128).requires_grad_(True)
    bias = torch.randn(Cout, generator=g, device="cuda").requires_grad_(True)
    y = A.linear(x, wl, bias)
    dy = torch.randn(y.shape, generator=g, device="cuda")
    gx, = torch.autograd.grad(y, [x], dy)
    launch = oh.conv_last_launch()
    dz = torch.zeros(1, 1, 2048, 16, device="cuda")
    dz[0, 0, :, :Cout] = dy
    _check(oh, mode, dz, w, 1, gx, launch, ("linear", Cout))


def test_relu_affine_bwd_bitwise(oh):
    """dZ = where(y > 0, dy * scale, 0) over channel slices with NaN around them and exact zeros in y."""
    g = torch.Generator(device="cuda").manual_seed(9)
    rows, Cc, dld, yld, dc, yc = 777, 96, 160, 224, 32, 64
    dy = torch.full((rows, dld), NAN, device="cuda")
    y = torch.full((rows, yld), NAN, device="cuda")
    dy[:, dc:dc + Cc] = torch.randn(rows, Cc, generator=g, device="cuda")
    yv = torch.randn(rows, Cc, generator=g, device="cuda")
    yv[yv.abs() < 0.3] = 0.0
    y[:, yc:yc + Cc] = yv
    scale = torch.rand(Cc, generator=g, device="cuda") + 0.5
    got = oh.relu_affine_bwd(dy, y, scale, dy_coff=dc, y_coff=yc, Cc=Cc)
    want = torch.where(yv > 0, dy[:, dc:dc + Cc] * scale, torch.zeros_like(yv))
    assert torch.equal(got, want)


# ---- production replay ----------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _spying(oh, calls, phase):
    """Inside the block every fp32 orehip.conv2d call is recorded in calls: signature -> [count, {the launchers it ran on}]."""
    real = oh.conv2d

    def spy(x, w_packed, Cout, k, stride=1, pad=None, **kw2):
        res = real(x, w_packed, Cout, k, stride, pad, **kw2)
        if x.dtype != torch.float32:
            return res
        B, H, W, ld = x.shape
        out = kw2.get("out")
        add = kw2.get("add")
        sig = (phase[0], B, H, W, ld, kw2.get("in_coff", 0), kw2.get("Cin") or ld - kw2.get("in_coff", 0), Cout, k, stride,
               k // 2 if pad is None else pad, out.shape[-1] if out is not None else Cout, kw2.get("out_coff", 0),
               kw2.get("scale") is not None, kw2.get("shift") is not None, int(kw2.get("relu_cout", 0)), kw2.get("in_mul") is not None,
               add.shape[-1] if add is not None else 0, kw2.get("w_wino") is not None, int(kw2.get("splitk", 0)),
               bool(kw2.get("want_colsum", False)), kw2.get("in_add") is not None, bool(kw2.get("in_relu", False)))
        e = calls.setdefault(sig, [0, set()])
        e[0] += 1
        e[1].add(oh.conv_last_launch())
        return res

    oh.conv2d = spy
    try:
        yield
    finally:
        oh.conv2d = real


def _spy_step(oh, batch):
    """Every distinct orehip.conv2d call of one eager training step: forward-pass calls marked "fwd", backward-pass calls "dgrad";
    each with the launcher it ran."""
    from conftest import GOLDEN, PKG
    import numpy as np
    from detectron2.modeling import build_model
    from detectron2.structures import Boxes, Instances
    from fewx.config import get_cfg
    from fewx.modeling.fsod.train_forward import train_forward
    from fewx.solver.build import get_bucket
    from oracle import ref_model as R
    from oracle import ref_train as T
    g = dict(np.load(os.path.join(GOLDEN, "train_iter_ref_full.npz")))
    shots = 24 if batch > 1 else int(g["shots"])
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(PKG, "configs", "fsod", "finetune_vovnet.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", "cuda", "INPUT.FS.SUPPORT_SHOT", shots])
    cfg.freeze()
    torch.manual_seed(0)
    m = build_model(cfg)
    m.load_state_dict(R.synth_roi_state(R.synth_state_dict(0), 0), strict=False)
    m.train()
    get_bucket(m, cfg)
    items, kw = [], {}
    if batch == 1:
        hw = tuple(int(v) for v in g["hw"])
        img, gt, sup, sbox = T.synth_train_inputs(int(g["input_seed"]), hw, n_gt=int(g["n_gt"]), shots=shots, support_hw=int(g["support_hw"]))
        items.append((img, gt, sup, sbox, hw))
        kw["roi_override"] = {"boxes": torch.from_numpy(g["roi_boxes"]), "labels": torch.from_numpy(g["roi_labels"]), "gt": torch.from_numpy(g["roi_gt"])}
    else:
        for b in range(batch):
            img, gt, sup, sbox = T.synth_train_inputs(40 + b, (640, 640), n_gt=15 + b % 6, shots=shots, support_hw=240)
            items.append((img, gt, sup, sbox, (640, 640)))
    data = []
    for img, gt, sup, sbox, hw in items:
        inst = Instances(hw)
        inst.gt_boxes, inst.gt_classes = Boxes(gt), torch.zeros(len(gt), dtype=torch.int64)
        data.append({"image": img, "instances": inst, "support_images": sup, "support_bboxes": sbox.numpy()})
    calls, phase = {}, ["fwd"]
    with _spying(oh, calls, phase):
        losses = train_forward(m, data, **kw)
        torch.cuda.synchronize()
        phase[0] = "dgrad"
        sum(losses.values()).backward()
        torch.cuda.synchronize()
    del m
    return calls


def _fwd_ref_images(images, xv, wl, stride, pad, bf16, scale, shift, relu_cout, mul, iadd, in_relu, add, wino, dev):
    """fwdconv_ref.fwd_ref of these images (None: all), one image at a time, as rows [n, Cout]."""
    B, H, W, Cin = xv.shape
    to = lambda t: None if t is None else t.to(dev)
    wl, scale, shift = to(wl), to(scale), to(shift)
    refs, mags = [], []
    for b in (range(B) if images is None else images):
        r, m = FR.fwd_ref(to(xv[b]).reshape(-1, Cin), wl, [(H, W)], 1, stride=stride, pad=pad, bf16=bf16, scale=scale, shift=shift,
                          relu_cout=relu_cout, in_mul=to(mul[b:b + 1]) if mul is not None else None,
                          in_add=to(iadd[b:b + 1]) if iadd is not None else None, in_relu=in_relu,
                          add=to(add[b:b + 1, ..., :wl.shape[0]]) if add is not None else None, wino=wino)
        refs.append(r)
        mags.append(m)
    return torch.cat(refs, 0), torch.cat(mags, 0)


def _replay(oh, mode, calls, batch):
    bf16 = mode == "bf16"
    reached, skipped, n, nfwd, ncs = set(), 0, 0, 0, 0
    dclasses = set()
    for i, (sig, (count, launches)) in enumerate(sorted(calls.items())):
        (ph, B, H, W, ld, in_coff, Cin, Cout, k, stride, pad, out_ld, out_coff, has_sc, has_sh, relu_cout, in_mul, add_ld, has_wino,
         splitk, colsum, has_in_add, in_relu) = sig
        if len(launches) != 1:
            skipped += 1
            continue
        fwd_only = stride != 1 or pad != k // 2 or in_mul   # forward-only forms: the float64 contract of tests/fwdconv_ref.py
        nfwd += fwd_only
        exact = in_mul and bf16                             # (operands whose affine is exact in fp32: fwdconv_ref's docstring)
        Ho, Wo = FR.out_hw(H, W, k, stride, pad)
        launch = next(iter(launches))
        if ph == "dgrad":
            dclasses.add((Cin, Cout, k))
        gen = torch.Generator(device="cuda").manual_seed(1000 + i)
        sx = 10.0 ** (torch.rand(Cin, generator=gen, device="cuda") * 6 - 3)
        x = torch.full((B, H, W, ld), NAN, device="cuda")
        xv = torch.randn(B, H, W, Cin, generator=gen, device="cuda") * sx
        if exact:
            sx = 2.0 ** (torch.rand(Cin, generator=gen, device="cuda") * 9 - 5)
            xv = ((torch.randn(B, H, W, Cin, generator=gen, device="cuda") * sx * 64).round() / 64).clamp(-63, 63)
        x[..., in_coff:in_coff + Cin] = xv
        mul = iadd = None
        if in_mul:
            sign = torch.where(torch.rand(B, Cin, generator=gen, device="cuda") < 0.3, -1.0, 1.0)
            mul = sign * (2.0 ** torch.randint(-2, 3, (B, Cin), generator=gen, device="cuda").float() if exact
                          else torch.rand(B, Cin, generator=gen, device="cuda") + 0.5)
            if has_in_add:
                iadd = torch.randn(B, Cin, generator=gen, device="cuda") * sx * mul.abs()
                iadd = ((iadd * 64).round() / 64).clamp(-63, 63) if exact else iadd
            assert not exact or FR.affine_is_exact(xv.reshape(-1, Cin), mul, iadd, B, [(H, W)]), sig
        sw = 10.0 ** (torch.rand(Cout, generator=gen, device="cuda") * 6 - 3)
        wl = torch.randn(Cout, Cin, k, k, generator=gen, device="cuda") * sw.view(-1, 1, 1, 1) / (Cin * k * k) ** 0.5
        pw = oh.pack_conv_weight_dev(wl)
        ww = oh.winograd_weight(pw, Cout, Cin) if has_wino else None
        scale = torch.rand(Cout, generator=gen, device="cuda") + 0.5 if has_sc else None
        shift = torch.randn(Cout, generator=gen, device="cuda") * float(sw.mean()) if has_sh else None
        add = None
        if add_ld:
            add = torch.randn(B, (Ho + 1) // 2, (Wo + 1) // 2, add_ld, generator=gen, device="cuda") * float(sw.mean())
        out = torch.full((B, Ho, Wo, out_ld), NAN, device="cuda")
        with _planned(oh) as plans:
            res = oh.conv2d(x, pw, Cout, k, stride, pad, in_coff=in_coff, Cin=Cin, scale=scale, shift=shift, relu_cout=relu_cout, add=add,
                            out=out, out_coff=out_coff, splitk=splitk, w_wino=ww, want_colsum=colsum, in_mul=mul, in_add=iadd,
                            in_relu=in_relu)
        got_l = oh.conv_last_launch()
        assert got_l == launch, (sig, launch, got_l)
        assert plans == [got_l], (sig, plans, got_l)
        out = res[0] if colsum else res
        assert bool(out[..., :out_coff].isnan().all()) and bool(out[..., out_coff + Cout:].isnan().all()), ("wrote outside its slice", sig)
        images, rows = _subset(B, Ho, Wo, k, B * Ho * Wo * Cin * Cout * k * k)
        wt = wl.transpose(0, 1).flip(2, 3).contiguous()          # the conv x -> out as a data-gradient-oriented weight
        name, S = got_l
        wino = name.startswith("k_conv3x3_wino")
        dev = "cuda" if B * Ho * Wo * Cin * Cout * k * k > 2e7 else "cpu"
        fwd_args = (xv, wl, stride, pad, bf16, scale, shift, relu_cout, mul, iadd, in_relu, add, wino, dev)
        if fwd_only:
            rows = None
            ref, mag = _fwd_ref_images(images, *fwd_args)
            d = FR.fwd_depth(k * k * Cin, S, affine=bool(in_mul), bf16=bf16)
        else:
            ref, mag = DR.dgrad_ref(xv, wt, bf16=bf16, device=dev, images=images, rows=rows, scale=scale, shift=shift, add=add,
                                    relu=relu_cout, wino=wino)
            d = DR.depth(k * k * Cin, S, wino_cin=Cin if wino else None)
        if colsum:                                            # the returned column sums against the float64 sum over ALL pixels
            cs = res[1]
            assert cs.shape == (-(-B * Ho * Wo // plans.bm), DR.c16(Cout)), (sig, cs.shape, plans.bm)
            full = (ref, mag) if images is None and rows is None else _fwd_ref_images(None, *fwd_args)
            r_cs = FR.colsum_check(cs, full[0], full[1], d, plans.bm, Cout)
            assert r_cs <= 1, (sig, got_l, "column sums", r_cs)
            ncs += 1
        g = out[..., out_coff:out_coff + Cout]
        if images is not None:
            g = g[images]
        g = g.reshape(-1, Cout)
        if rows is not None:
            g = g[rows.to(g.device)]
        r = DR.dgrad_check(g, ref, mag, d)
        _record(mode, name, r)
        assert r["hard"] <= 1 and r["rms"] <= 1, (sig, got_l, r)
        reached.add((ph, name))
        n += 1
    print(f"\n{mode} bs{batch}: {len(calls)} distinct conv2d calls ({sum(c for c, _ in calls.values())} launches), {n} replayed "
          f"({nfwd} stride 2 / input affine through fwdconv_ref, {ncs} with column sums), {skipped} skipped (ran on more than one "
          f"launcher); launchers {sorted(reached)}")
    _replay.counts = {"replayed": n, "fwd_only": nfwd, "colsum": ncs, "skipped": skipped}
    return dclasses


@pytest.mark.parametrize("batch", [1, 16])
def test_production_replay(oh, mode, batch):
    calls = _spy_step(oh, batch)
    assert any(s[0] == "dgrad" for s in calls) and any(s[0] == "fwd" for s in calls)
    dclasses = _replay(oh, mode, calls, batch)
    # every data-gradient call of the step is a class of the shape matrix: (Cin_launch = Cout16, Cout_launch = Cin, k) of a layer
    model = {(DR.c16(co), ci, k) for (co, ci, k) in DR.LAYERS}
    print(f"dgrad classes {sorted(dclasses)}")
    assert dclasses <= model, sorted(dclasses - model)
    assert model <= dclasses, sorted(model - dclasses)


def test_replay_of_the_forward_forms_a_training_step_lacks(oh, mode):
    """The replay on the forward forms of the inference engine that no training step of this configuration calls: the eSE concat conv
    with fused column sums (1x1, one image and two), the consumer of an eSE gate (in_mul alone), a GroupNorm fold (in_mul, in_add,
    in_relu) and a 3x3 stride-2 layer with a slice output.  Recorded through the same spy, so every branch of _replay runs in both
    modes whatever the step contains."""
    z = lambda *s: torch.zeros(*s, device="cuda")
    calls = {}
    with _spying(oh, calls, ["fwd"]):
        for B, H, W, Cin, Cout in ((1, 20, 19, 352, 256), (2, 9, 11, 64, 48)):
            pw = oh.pack_conv_weight_dev(z(Cout, Cin, 1, 1))
            oh.conv2d(z(B, H, W, Cin), pw, Cout, 1, scale=z(Cout), shift=z(Cout), relu_cout=Cout, want_colsum=True)
        pw = oh.pack_conv_weight_dev(z(96, 64, 3, 3))
        oh.conv2d(z(2, 13, 10, 96), pw, 96, 3, in_coff=16, Cin=64, scale=z(96), shift=z(96), relu_cout=96, in_mul=z(2, 64))
        oh.conv2d(z(2, 13, 10, 64), pw, 96, 3, shift=z(96), relu_cout=50, in_mul=z(2, 64), in_add=z(2, 64), in_relu=True)
        pw = oh.pack_conv_weight_dev(z(128, 64, 3, 3))
        oh.conv2d(z(2, 14, 17, 64), pw, 128, 3, 2, scale=z(128), shift=z(128), relu_cout=128, out=z(2, 7, 9, 160), out_coff=32)
    assert len(calls) == 5
    _replay(oh, mode, calls, 0)
    assert _replay.counts == {"replayed": 5, "fwd_only": 3, "colsum": 2, "skipped": 0}, _replay.counts
