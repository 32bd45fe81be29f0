"""GPU parity tests: every HIP kernel, called through the C-ABI (orehip -> libore_hip.so), against the CPU
oracle on the same seeded inputs and against the reference-run golden fixtures.

Tolerances: fp32 feature maps within 1e-4 rel (max|a-b| / max|b|), as BASELINE.json's north_star states;
indices / keep lists / decoded boxes and scores bit-exact versus oracle/ref_decode.c on identical inputs."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import chan_err
from conftest import rel_err as _max_norm_err
from oracle import decode as odec
from oracle import ref_model as R

pytestmark = pytest.mark.gpu
TOL = 1e-4
# per-channel rms bound (conftest.chan_err) for tensors at the END of the dense chain (28 layers deep, behind the correlation's
# depthwise products): a channel's own rms is the yardstick there, not the tensor's maximum; measured 0.4-1.1e-4 (ORE_CHAN_LOG)
CHAN_TOL_DEEP = 3e-4


def rel_err(a, b):
    """The measure every feature-map comparison of this file uses.  The max-norm figure max|a - b| / max|b| (north_star's "1e-4 rel") alone
    lets a channel -- or a pyramid level -- whose magnitude is 1 % of the tensor's maximum be 1 % wrong,
    so for every array with a channel axis (NCHW maps, [rows, channels] matrices, [B, C] gates) the PER-CHANNEL rms error joins it:
    returned is max(max-norm error, chan_err / 3), i.e. `rel_err(...) < TOL` also asserts chan_err < 3 * TOL = CHAN_TOL_DEEP for each
    channel against its own rms (measured 2e-7 ... 1.4e-4 over this file's call sites)."""
    a, b = np.asarray(a), np.asarray(b)
    v = _max_norm_err(a, b)
    if a.ndim in (2, 4) and a.shape == b.shape and a.shape[1] >= 1 and a.size > a.shape[1]:
        v = max(v, chan_err(a, b) / 3.0)
    return v


@pytest.fixture(scope="module")
def ore():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import orehip
    orehip.lib()  # fails loudly if libore_hip.so is missing
    return orehip


@pytest.fixture(scope="module")
def sd():
    return R.synth_state_dict(0)


def dev(t):
    return t.contiguous().cuda()


def nhwc(x_nchw):
    return x_nchw.permute(0, 2, 3, 1).contiguous().cuda()


def nchw(x_nhwc):
    return x_nhwc.permute(0, 3, 1, 2).cpu()


def bn_fold(sd, name):
    sc = sd[name + "/norm.weight"] * (sd[name + "/norm.running_var"] + 1e-5).rsqrt()
    return sc, sd[name + "/norm.bias"] - sd[name + "/norm.running_mean"] * sc


def conv_bn(ore, x, sd, name, k, stride, **kw):
    w = sd[name + "/conv.weight"]
    sc, sh = bn_fold(sd, name)
    return ore.conv2d(x, ore.pack_conv_weight(w).cuda(), w.shape[0], k, stride, scale=dev(sc), shift=dev(sh),
                      relu_cout=w.shape[0], **kw)


# ------------------------------------------------------------------------------------------ convs
def test_conv_golden_blocks(ore, sd, golden):
    p = "backbone.bottom_up.stem."
    g = golden("conv_stem2")
    y = conv_bn(ore, nhwc(torch.from_numpy(g["x"])), sd, p + "stem_2", 3, 1)
    assert rel_err(nchw(y).numpy(), g["y"]) < TOL
    assert chan_err(nchw(y).numpy(), g["y"]) < TOL
    g = golden("conv_stem3_odd")
    y = conv_bn(ore, nhwc(torch.from_numpy(g["x"])), sd, p + "stem_3", 3, 2)
    assert y.shape[1:3] == g["y"].shape[2:]
    assert rel_err(nchw(y).numpy(), g["y"]) < TOL
    assert chan_err(nchw(y).numpy(), g["y"]) < TOL


@pytest.mark.parametrize("B,H,W,Cin,Cout,k,stride,splitk", [
    (1, 20, 20, 384, 112, 3, 1, 0),    # OSA5 layer 0 shape (auto split-K)
    (1, 20, 20, 384, 112, 3, 1, 1),    # same, no split
    (1, 20, 20, 384, 112, 3, 1, 7),    # forced odd split
    (2, 17, 23, 352, 256, 1, 1, 0),    # 1x1 concat, odd spatial, 2 column blocks
    (1, 40, 40, 96, 96, 3, 1, 0),
    (1, 9, 7, 16, 5, 3, 1, 0),         # tiny, Cout=5 (head) -> padded to 16
    (1, 80, 80, 128, 128, 3, 1, 0),
    (3, 33, 31, 64, 80, 3, 2, 0),      # stride 2, odd size, N=80
    (1, 160, 160, 64, 64, 3, 1, 0),    # BM=128 path
])
def test_conv_random_vs_oracle(ore, B, H, W, Cin, Cout, k, stride, splitk):
    g = torch.Generator().manual_seed(B * 1000 + H + Cin + Cout)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
    sc = torch.rand(Cout, generator=g) + 0.5
    sh = torch.randn(Cout, generator=g) * 0.1
    ref = F.relu(F.conv2d(x, w, None, stride, k // 2) * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))
    y = ore.conv2d(nhwc(x), ore.pack_conv_weight(w).cuda(), Cout, k, stride, scale=dev(sc), shift=dev(sh),
                   relu_cout=Cout, splitk=splitk)
    assert rel_err(nchw(y).numpy(), ref.numpy()) < TOL


def test_conv_slices_inmul_add_partial_relu(ore):
    """Channel-slice in/out (OSA concat buffer), input affine+ReLU (GN fold), nearest-2x add (FPN), partial ReLU."""
    g = torch.Generator().manual_seed(7)
    B, H, W = 2, 11, 14
    buf = torch.randn(B, 96, H, W, generator=g)           # read channels 32..79 (48), write into 16..47 of out buffer
    w = torch.randn(32, 48, 3, 3, generator=g) * 0.05
    mul = torch.rand(B, 48, generator=g) + 0.5
    add_in = torch.randn(B, 48, generator=g) * 0.2
    top = torch.randn(B, 32, (H + 1) // 2, (W + 1) // 2, generator=g)
    bias = torch.randn(32, generator=g)
    xin = F.relu(buf[:, 32:80] * mul[:, :, None, None] + add_in[:, :, None, None])
    ref = F.conv2d(xin, w, bias, 1, 1) + F.interpolate(top, scale_factor=2.0, mode="nearest")[:, :, :H, :W]
    ref[:, :20] = F.relu(ref[:, :20])
    out = torch.full((B, H, W, 64), -7.0).cuda()
    ore.conv2d(nhwc(buf), ore.pack_conv_weight(w).cuda(), 32, 3, 1, in_coff=32, Cin=48, shift=dev(bias), relu_cout=20,
               in_mul=dev(mul), in_add=dev(add_in), in_relu=True, add=nhwc(top), out=out, out_coff=16)
    o = nchw(out)
    assert rel_err(o[:, 16:48].numpy(), ref.numpy()) < TOL
    assert (o[:, :16] == -7.0).all() and (o[:, 48:] == -7.0).all()  # neighbours of the slice untouched


@pytest.fixture
def wino_forced(ore):
    """Winograd F(2x2,3x3) kernel (csrc/ore_conv_wino.hip) wherever it applies -- the automatic plan only takes it from 1500 / 3000 rows."""
    with ore.conv_overrides((-7, 2)):
        yield


@pytest.mark.parametrize("B,H,W,Cin,Cout", [
    (1, 32, 32, 64, 64),      # stem_2 / stage-2 64 -> 64 shape class, whole batches
    (1, 20, 24, 128, 64),     # stage-2 layer 0 class (two K wave groups, 32 channels per block), partial column batch
    (2, 13, 11, 64, 128),     # odd sizes: tiles hanging over the right and bottom edge, two images, two channel blocks
    (1, 10, 40, 128, 128),    # FPN output / head tower class
    (1, 3, 5, 64, 64),        # smaller than one batch
    (1, 24, 40, 80, 80),      # nu-split build (k_conv3x3_wino_nu): stage-3 class, 48 channels per block, second block 32 real
    (2, 13, 19, 112, 80),     # stage-3 layer 0 class: 32 channels per block, third block half empty; odd sizes, two images
    (1, 20, 20, 96, 96),      # stage-4 class, three full channel blocks
    (1, 9, 33, 112, 112),     # stage-5 class
    (1, 12, 16, 96, 256),     # dgrad of stage-4 layer 0: eight channel blocks
    (1, 7, 9, 80, 16),        # a single channel group
])
def test_conv_winograd_kernel_vs_oracle(ore, wino_forced, B, H, W, Cin, Cout):
    """k_conv3x3_wino against F.conv2d at the fp32 tolerance, with FrozenBN scale / shift + ReLU, and bit-reproducible."""
    g = torch.Generator().manual_seed(B * 100 + H + W + Cin + Cout)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5
    sc = torch.rand(Cout, generator=g) + 0.5
    sh = torch.randn(Cout, generator=g) * 0.1
    ref = F.relu(F.conv2d(x, w, None, 1, 1) * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))
    wp = ore.pack_conv_weight(w).cuda()
    U = ore.winograd_weight(wp, Cout, Cin)
    y = ore.conv2d(nhwc(x), wp, Cout, 3, 1, scale=dev(sc), shift=dev(sh), relu_cout=Cout, w_wino=U)
    direct = ore.conv2d(nhwc(x), wp, Cout, 3, 1, scale=dev(sc), shift=dev(sh), relu_cout=Cout)
    assert not torch.equal(y, direct), "the Winograd kernel did not run (results identical to the direct kernel bit for bit)"
    assert rel_err(nchw(y).numpy(), ref.numpy()) < TOL
    assert rel_err(nchw(y).numpy(), nchw(direct).numpy()) < 2e-5
    y2 = ore.conv2d(nhwc(x), wp, Cout, 3, 1, scale=dev(sc), shift=dev(sh), relu_cout=Cout, w_wino=U)
    assert torch.equal(y, y2)


def test_conv_winograd_weight_transform(ore):
    """U = G g G^T per (Cout, Cin) pair, stored in MFMA-fragment order [16 pos][Cout16 / 16][Cin / 16][(c % 16) / 4][n % 16][c % 4]."""
    g = torch.Generator().manual_seed(5)
    w = torch.randn(48, 64, 3, 3, generator=g)
    U = ore.winograd_weight(ore.pack_conv_weight(w).cuda(), 48, 64).cpu()
    U = U.view(16, 3, 4, 4, 16, 4).permute(0, 1, 4, 2, 3, 5).reshape(4, 4, 48, 64)
    G = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=torch.float64)
    want = torch.einsum("xa,ncab,yb->xync", G, w.double(), G)
    assert float((U.double() - want).abs().max()) < 1e-6


def test_conv_winograd_slices_levels_bias(ore, wino_forced):
    """What the engine asks of it: channel-slice input and output inside wider buffers (the OSA concat buffer), bias without scale, no
    ReLU, three pyramid levels in one launch (the head tower), and the automatic plan taking it at 6400 rows."""
    g = torch.Generator().manual_seed(12)
    buf = torch.randn(1, 192, 20, 24, generator=g)                                 # read channels 64..127
    w = torch.randn(64, 64, 3, 3, generator=g) * 0.04
    sh = torch.randn(64, generator=g) * 0.1
    out = torch.full((1, 20, 24, 160), 7.0).cuda()
    wp = ore.pack_conv_weight(w).cuda()
    U = ore.winograd_weight(wp, 64, 64)
    ore.conv2d(nhwc(buf), wp, 64, 3, 1, in_coff=64, Cin=64, shift=dev(sh), relu_cout=0, out=out, out_coff=32, w_wino=U)
    ref = F.conv2d(buf[:, 64:128], w, sh, 1, 1)
    assert rel_err(nchw(out[..., 32:96].contiguous()).numpy(), ref.numpy()) < TOL
    assert float(out[..., :32].min()) == 7.0 and float(out[..., 96:].max()) == 7.0   # the neighbours of the slice are untouched
    HW = [(12, 16), (6, 8), (3, 4)]
    xs = [torch.randn(1, 128, h, w_, generator=g) for h, w_ in HW]
    w2 = torch.randn(128, 128, 3, 3, generator=g) * 0.03
    b2 = torch.randn(128, generator=g) * 0.1
    rows = torch.cat([nhwc(t).reshape(-1, 128) for t in xs], 0).contiguous()
    wp2 = ore.pack_conv_weight(w2).cuda()
    U2 = ore.winograd_weight(wp2, 128, 128)
    y = ore.conv2d_levels(rows, HW, 1, wp2, 128, 3, shift=dev(b2), w_wino=U2).cpu()
    r0 = 0
    for (h, w_), t in zip(HW, xs):
        ref_l = F.conv2d(t, w2, b2, 1, 1)[0].permute(1, 2, 0).reshape(-1, 128)
        assert rel_err(y[r0:r0 + h * w_].numpy(), ref_l.numpy()) < TOL
        r0 += h * w_
    # nu-split build: slice of the stage-3 concat buffer in, slice out
    buf3 = torch.randn(1, 352, 12, 20, generator=g)
    w3 = torch.randn(80, 80, 3, 3, generator=g) * 0.04
    sh3 = torch.randn(80, generator=g) * 0.1
    out3 = torch.full((1, 12, 20, 352), 7.0).cuda()
    wp3 = ore.pack_conv_weight(w3).cuda()
    ore.conv2d(nhwc(buf3), wp3, 80, 3, 1, in_coff=112, Cin=80, shift=dev(sh3), relu_cout=80, out=out3, out_coff=192,
               w_wino=ore.winograd_weight(wp3, 80, 80))
    ref3 = F.relu(F.conv2d(buf3[:, 112:192], w3, sh3, 1, 1))
    assert rel_err(nchw(out3[..., 192:272].contiguous()).numpy(), ref3.numpy()) < TOL
    assert float(out3[..., :192].min()) == 7.0 and float(out3[..., 272:].max()) == 7.0
    assert ore.winograd_covers(80, 80) and ore.winograd_covers(384, 112) and not ore.winograd_covers(96, 256) and not ore.winograd_covers(40, 80)
    ore.lib().ore_conv_set_plan_override(-7, 1, 0, 0, 0)                              # automatic: M = 6400 qualifies
    x3 = torch.randn(1, 64, 80, 80, generator=g)
    y3 = ore.conv2d(nhwc(x3), wp, 64, 3, 1, shift=dev(sh), w_wino=U)
    d3 = ore.conv2d(nhwc(x3), wp, 64, 3, 1, shift=dev(sh))
    assert not torch.equal(y3, d3) and rel_err(nchw(y3).numpy(), F.conv2d(x3, w, sh, 1, 1).numpy()) < TOL


@pytest.mark.parametrize("HW,B", [([(80, 80), (40, 40), (20, 20)], 1), ([(12, 20), (6, 10), (3, 5)], 2), ([(5, 7), (3, 4), (2, 2)], 1)])
def test_conv_winograd_per_level_weights(ore, HW, B):
    """Three layers of one shape over three pyramid levels in ONE launch (the FPN output convs): level l multiplies its own Winograd
    weights and adds its own bias; every block of the kernel serves one level."""
    g = torch.Generator().manual_seed(HW[0][0] + B)
    Cc = 128
    xs = [torch.randn(B, Cc, h, w_, generator=g) for h, w_ in HW]
    ws = [torch.randn(Cc, Cc, 3, 3, generator=g) * 0.03 for _ in HW]
    bs = [torch.randn(Cc, generator=g) * 0.1 for _ in HW]
    rows = torch.cat([nhwc(t).reshape(-1, Cc) for t in xs], 0).contiguous()
    wps = [ore.pack_conv_weight(w).cuda() for w in ws]
    U = torch.stack([ore.winograd_weight(wp, Cc, Cc) for wp in wps]).contiguous()
    out = torch.full((rows.shape[0], 2 * Cc), 7.0).cuda()
    ore.conv2d_levels(rows, HW, B, wps[0], Cc, 3, shift=dev(torch.stack(bs).contiguous()), ep_stride=Cc, w_wino=U, w_wino_level_stride=U.shape[1],
                      out=out, out_coff=Cc)
    assert float(out[:, :Cc].min()) == 7.0 and float(out[:, :Cc].max()) == 7.0
    y = out[:, Cc:].cpu()
    r0 = 0
    for (h, w_), t, w, b in zip(HW, xs, ws, bs):
        ref_l = F.conv2d(t, w, b, 1, 1).permute(0, 2, 3, 1).reshape(-1, Cc)
        assert rel_err(y[r0:r0 + B * h * w_].numpy(), ref_l.numpy()) < TOL
        r0 += B * h * w_
    with pytest.raises(ore.OreError):                                                # 1x1 layers have no per-level form
        ore.conv2d_levels(rows, HW, B, ore.pack_conv_weight(torch.randn(Cc, Cc, 1, 1)).cuda(), Cc, 1, w_wino=U, w_wino_level_stride=U.shape[1])


@pytest.fixture
def kw_forced(ore):
    """Force the wave-private K-split LDS-DMA kernel (k_conv_kw, csrc/ore_conv_kw.hip) wherever it applies, then restore the plan."""
    with ore.conv_overrides((-2, 2), (-10, 0), (-12, 0), (-14, 0)):   # (the register-fed / lean-DMA kernels would take their shapes first)
        yield


@pytest.mark.parametrize("B,H,W,Cin,Cout,k,stride", [
    (1, 20, 20, 384, 112, 3, 1),    # stage-5 layer 0: deep K, cross-block split-K
    (1, 20, 20, 112, 112, 3, 1),    # stage-5 layers 1/2
    (1, 20, 20, 720, 512, 1, 1),    # stage-5 concat
    (1, 40, 40, 256, 96, 3, 1),     # stage-4 layer 0
    (1, 40, 40, 544, 384, 1, 1),    # stage-4 concat
    (1, 80, 80, 112, 80, 3, 1),     # stage-3 layer 0 (BN = 80)
    (1, 80, 80, 352, 256, 1, 1),    # stage-3 concat
    (1, 40, 40, 128, 128, 3, 1),    # FPN output 4
    (2, 17, 23, 352, 256, 1, 1),    # odd spatial size, 2 images, rows not a multiple of the tile
    (1, 9, 7, 16, 5, 3, 1),         # tiny: one chunk per tap, Cout = 5 (padded to 16), most waves idle
    (3, 33, 31, 64, 80, 3, 2),      # stride 2, odd size
    (1, 1, 320, 8192, 128, 1, 1),   # the second-stage GEMM (320 ROIs x 8192 -> 128)
    (1, 13, 11, 48, 48, 3, 1),      # Cin = 48: three chunks per tap, wraps inside one 4-chunk advance
])
def test_conv_kw_kernel_vs_oracle(ore, kw_forced, B, H, W, Cin, Cout, k, stride):
    g = torch.Generator().manual_seed(B * 1000 + H + Cin + Cout + k)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
    sc = torch.rand(Cout, generator=g) + 0.5
    sh = torch.randn(Cout, generator=g) * 0.1
    ref = F.relu(F.conv2d(x, w, None, stride, k // 2) * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))
    y = ore.conv2d(nhwc(x), ore.pack_conv_weight(w).cuda(), Cout, k, stride, scale=dev(sc), shift=dev(sh), relu_cout=Cout)
    assert rel_err(nchw(y).numpy(), ref.numpy()) < TOL
    y2 = ore.conv2d(nhwc(x), ore.pack_conv_weight(w).cuda(), Cout, k, stride, scale=dev(sc), shift=dev(sh), relu_cout=Cout)
    assert torch.equal(y, y2)                       # split-K slabs are summed in slice order: bit-reproducible


GD_BUILDS = [(64, 128, 4), (64, 64, 4), (64, 112, 4), (128, 64, 4), (128, 128, 4), (32, 128, 4), (128, 112, 4), (208, 64, 4), (224, 64, 4), (112, 64, 4), (96, 128, 4),
             (64, 128, 2), (128, 128, 2), (208, 64, 2), (128, 112, 2),
             (128, 128, 14), (112, 128, 14), (128, 112, 14), (64, 128, 14), (128, 64, 14), (64, 64, 14), (128, 128, 12), (112, 128, 12), (80, 64, 4), (80, 128, 4), (48, 64, 4), (32, 64, 4)]   # 10 + ns: the eight-wave builds


@pytest.fixture
def gd_forced(ore):
    """Force builds of the shared-stage descriptor kernel (k_conv_gd, csrc/ore_conv_gd.hip); restore the plan afterwards."""
    with ore.conv_overrides():
        yield


@pytest.mark.parametrize("bm,bn,ns", GD_BUILDS)
@pytest.mark.parametrize("B,H,W,Cin,Cout,k,stride", [
    (1, 40, 48, 352, 256, 1, 1),    # a stage-3 concat shape, smaller map
    (1, 33, 47, 320, 112, 1, 1),    # the stage-2 concat's widths, odd size: rows not a multiple of the tile, Cout = 112
    (1, 66, 50, 64, 128, 3, 2),     # stem_3: 3x3 stride 2, even size
    (2, 17, 23, 64, 128, 3, 2),     # stride 2, odd size, two images
    (1, 9, 11, 96, 40, 3, 1),       # tiny: most of every tile is padding, Cout = 40
])
def test_conv_gd_every_build(ore, gd_forced, bm, bn, ns, B, H, W, Cin, Cout, k, stride):
    """k_conv_gd (shared-stage LDS-DMA through buffer descriptors) against F.conv2d at 1e-4, every instantiated (tile, ring depth) build:
    1x1 and 3x3 / stride 2, border taps and partial tiles as the descriptor's zeros, K not a multiple of the unroll, bit-reproducible,
    fused per-tile column sums."""
    g = torch.Generator().manual_seed(B * 1000 + H + Cin + Cout + k + bm + ns)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
    sc = torch.rand(Cout, generator=g) + 0.5
    sh = torch.randn(Cout, generator=g) * 0.1
    ref = F.relu(F.conv2d(x, w, None, stride, k // 2) * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))
    wp = ore.pack_conv_weight(w).cuda()
    ore.lib().ore_conv_set_plan_override(-15, bm, bn, ns, 0)
    y, cs = ore.conv2d(nhwc(x), wp, Cout, k, stride, scale=dev(sc), shift=dev(sh), relu_cout=Cout, want_colsum=True)
    assert rel_err(nchw(y).numpy(), ref.numpy()) < TOL
    assert chan_err(nchw(y).numpy(), ref.numpy()) < TOL
    assert rel_err(cs.sum(0)[:Cout].cpu().numpy(), ref.sum((0, 2, 3)).numpy()) < 1e-5
    y2 = ore.conv2d(nhwc(x), wp, Cout, k, stride, scale=dev(sc), shift=dev(sh), relu_cout=Cout)
    assert torch.equal(y, y2)
    # channel slices: a slice of a wider input, a slice of a wider output
    buf = torch.randn(B, H, W, 16 + Cin, generator=g)
    xs = buf[..., 16:].permute(0, 3, 1, 2).contiguous()
    refs = F.conv2d(xs, w, sh, stride, k // 2)
    out = torch.full((B, refs.shape[2], refs.shape[3], 32 + (Cout + 15) // 16 * 16), 3.0).cuda()
    ore.conv2d(buf.cuda(), wp, Cout, k, stride, in_coff=16, Cin=Cin, shift=dev(sh), out=out, out_coff=32)
    o = out.cpu()
    assert rel_err(o[..., 32:32 + Cout].permute(0, 3, 1, 2).numpy(), refs.numpy()) < TOL and (o[..., :32] == 3.0).all()


@pytest.mark.parametrize("bm,bn,ns", [(64, 64, 14), (32, 64, 4), (80, 64, 4), (64, 128, 4)])
def test_conv_gd_levels_flat(ore, gd_forced, bm, bn, ns):
    """A 1x1 stride-1 layer over several pyramid levels is one flat GEMM over the level-major rows for k_conv_gd too (conv3 after the
    correlation: 256 -> 128 over p3..p5): forced builds against F.conv2d per level, and the automatic plan at the 640^2 row counts
    (6400 + 1600 + 400) bit-identical to the forced build it names."""
    g = torch.Generator().manual_seed(bm + ns)
    HW = [(21, 19), (11, 10), (6, 5)]
    B, Cin, Cout = 2, 256, 128
    w = torch.randn(Cout, Cin, 1, 1, generator=g) / Cin ** 0.5
    b = torch.randn(Cout, generator=g) * 0.1
    xs = [torch.randn(B, Cin, h, ww, generator=g) for h, ww in HW]
    rows = torch.cat([nhwc(x).reshape(-1, Cin) for x in xs], 0).contiguous()
    wp = ore.pack_conv_weight(w).cuda()
    with ore.conv_overrides((-12, 0), (-15, bm, bn, ns)):          # k_conv_kd would take these rows first
        y = ore.conv2d_levels(rows.cuda(), HW, B, wp, Cout, 1, shift=dev(b), relu_cout=Cout).cpu()
    o = 0
    for x, (h, ww) in zip(xs, HW):
        ref = F.relu(F.conv2d(x, w, b))
        got = y[o:o + B * h * ww].reshape(B, h, ww, Cout).permute(0, 3, 1, 2)
        assert rel_err(got.numpy(), ref.numpy()) < TOL
        o += B * h * ww


@pytest.mark.parametrize("bm,bn,ns", [(64, 64, 14), (64, 64, 4), (32, 128, 4)])
def test_conv_gd_topdown_add(ore, gd_forced, bm, bn, ns):
    """k_conv_gd's epilogue adds the nearest-upsampled coarser level (the FPN lateral): odd sizes, two images."""
    g = torch.Generator().manual_seed(ns + bm)
    B, H, W, Cin, Cout = 2, 13, 18, 64, 48
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 1, 1, generator=g) / 8
    b = torch.randn(Cout, generator=g) * 0.1
    top = torch.randn(B, Cout, (H + 1) // 2, (W + 1) // 2, generator=g)
    ref = F.conv2d(x, w, b) + F.interpolate(top, scale_factor=2, mode="nearest")[:, :, :H, :W]
    with ore.conv_overrides((-12, 0), (-15, bm, bn, ns)):
        y = ore.conv2d(nhwc(x), ore.pack_conv_weight(w).cuda(), Cout, 1, 1, shift=dev(b), add=nhwc(top))
    assert rel_err(nchw(y).numpy(), ref.numpy()) < TOL


def test_conv_gd_plan_takes_conv3_and_lat3(ore):
    """The automatic plan at the 640^2 shapes: conv3 over three levels (8400 rows) and the stage-3 lateral (6400 rows), 256 -> 128, run on
    k_conv_gd -- the results equal the forced builds the plan names bit for bit, and differ in rounding from k_conv_kd's."""
    g = torch.Generator().manual_seed(5)
    w = torch.randn(128, 256, 1, 1, generator=g) / 16
    wp = ore.pack_conv_weight(w).cuda()
    for HW, build in (([(80, 80), (40, 40), (20, 20)], (32, 64, 4)), ([(80, 80)], (64, 64, 14))):
        rows = torch.randn(sum(h * ww for h, ww in HW), 256, generator=g).cuda()
        top = torch.randn(1, 40, 40, 128, generator=g).cuda()          # the lateral adds the upsampled coarser level (FPN top-down)
        run = (lambda: ore.conv2d_levels(rows, HW, 1, wp, 128, 1)) if len(HW) > 1 else (lambda: ore.conv2d(rows.view(1, 80, 80, 256), wp, 128, 1, add=top).view(-1, 128))
        y_plan = run().clone()
        with ore.conv_overrides((-12, 0), (-15, *build)):
            y_forced = run().clone()
        with ore.conv_overrides((-12, 0), (-14, 0)):
            y_other = run().clone()                                    # gd and kd off: the round-3 kernel
        assert torch.equal(y_plan, y_forced)
        ref = rows.cpu() @ w.view(128, 256).t()
        if len(HW) == 1:
            ref = ref + top.cpu()[0].repeat_interleave(2, 0).repeat_interleave(2, 1).reshape(-1, 128)
        assert rel_err(y_plan.cpu().numpy(), ref.numpy()) < TOL and rel_err(y_other.cpu().numpy(), ref.numpy()) < TOL


@pytest.fixture
def kd_forced(ore):
    """Force the lean LDS-DMA kernel (k_conv_kd, csrc/ore_conv_kd.hip) wherever it applies, then restore the plan."""
    with ore.conv_overrides((-12, 2)):
        yield


KD_BUILDS = [(16, 16, 4, 4), (16, 16, 4, 8), (16, 16, 8, 4), (16, 16, 16, 2), (16, 32, 4, 4), (16, 32, 8, 2), (32, 32, 4, 4), (32, 32, 8, 2),
             (16, 48, 4, 4), (16, 48, 8, 2), (16, 64, 4, 2), (16, 80, 4, 2), (32, 64, 4, 2), (32, 80, 4, 2), (64, 64, 4, 2), (32, 48, 4, 2),
             (32, 16, 4, 4)]


@pytest.mark.parametrize("B,H,W,Cin,Cout,k,stride", [
    (1, 20, 20, 112, 112, 3, 1),    # stage-5 layers 1 / 2
    (1, 20, 20, 384, 112, 3, 1),    # stage-5 layer 0
    (1, 20, 20, 720, 512, 1, 1),    # stage-5 concat
    (1, 40, 40, 96, 96, 3, 1),      # stage-4 layers 1 / 2
    (1, 40, 40, 256, 96, 3, 1),     # stage-4 layer 0
    (1, 40, 40, 544, 384, 1, 1),    # stage-4 concat
    (1, 80, 80, 256, 128, 1, 1),    # FPN lateral 3
    (1, 1, 320, 8192, 128, 1, 1),   # the second-stage GEMM
    (2, 13, 11, 96, 40, 3, 1),      # two images, odd size, rows not a multiple of 16, Cout = 40
    (1, 9, 7, 112, 5, 3, 1),        # Cout = 5: one channel quad + one lane of the next
    (3, 17, 15, 128, 64, 3, 2),     # stride 2, odd size, three images
    (1, 7, 5, 16, 16, 3, 1),        # one chunk per tap
])
def test_conv_kd_kernel_vs_oracle(ore, kd_forced, B, H, W, Cin, Cout, k, stride):
    """k_conv_kd against F.conv2d at 1e-4: border taps, partial tiles and chunks beyond K arrive as the buffer descriptor's zeros
    through LDS-DMA; bit-reproducible; another summation order than k_conv_kw's (2e-5 of it)."""
    g = torch.Generator().manual_seed(B * 1000 + H + Cin + Cout + k)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
    sc = torch.rand(Cout, generator=g) + 0.5
    sh = torch.randn(Cout, generator=g) * 0.1
    ref = F.relu(F.conv2d(x, w, None, stride, k // 2) * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))
    wp = ore.pack_conv_weight(w).cuda()
    y = ore.conv2d(nhwc(x), wp, Cout, k, stride, scale=dev(sc), shift=dev(sh), relu_cout=Cout)
    assert rel_err(nchw(y).numpy(), ref.numpy()) < TOL
    assert chan_err(nchw(y).numpy(), ref.numpy()) < TOL
    assert torch.equal(y, ore.conv2d(nhwc(x), wp, Cout, k, stride, scale=dev(sc), shift=dev(sh), relu_cout=Cout))
    with ore.conv_overrides((-12, 0), (-10, 0)):
        y_kw = ore.conv2d(nhwc(x), wp, Cout, k, stride, scale=dev(sc), shift=dev(sh), relu_cout=Cout)
    assert rel_err(y.cpu().numpy(), y_kw.cpu().numpy()) < 2e-5


@pytest.mark.parametrize("bm,bn,nw,sb", KD_BUILDS)
@pytest.mark.parametrize("H,W,Cin,Cout,k", [(20, 20, 112, 112, 3), (7, 9, 96, 80, 3), (1, 96, 2048, 128, 1)])
def test_conv_kd_every_build(ore, kd_forced, bm, bn, nw, sb, H, W, Cin, Cout, k):
    """Every instantiated (tile, waves, steps per batch) build of k_conv_kd: one batch, many batches (double-buffer reuse), waves whose
    range lies wholly beyond K, tiles wider than Cout."""
    L = ore.lib()
    if bn > (Cout + 15) // 16 * 16 and (bm, (Cout + 15) // 16 * 16, nw, sb) not in KD_BUILDS:
        pytest.skip("the launcher narrows the tile to Cout; that narrower build is not instantiated")
    g = torch.Generator().manual_seed(H + Cin + nw + sb + bm)
    x = torch.randn(1, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
    sh = torch.randn(Cout, generator=g) * 0.1
    ref = F.conv2d(x, w, sh, 1, k // 2)
    L.ore_conv_set_plan_override(-13, bm, bn, nw, sb)
    y = ore.conv2d(nhwc(x), ore.pack_conv_weight(w).cuda(), Cout, k, 1, shift=dev(sh))
    assert rel_err(nchw(y).numpy(), ref.numpy()) < TOL


def test_conv_kd_slices_add_colsum(ore, kd_forced):
    """Channel-slice input / output inside wider buffers, the FPN top-down addend (nearest-2x) and the fused per-tile column sums."""
    g = torch.Generator().manual_seed(5)
    B, H, W, Cin, Cout = 1, 10, 12, 128, 128
    buf = torch.randn(B, H, W, 32 + Cin + 16, generator=g)
    x = buf[..., 32:32 + Cin].permute(0, 3, 1, 2).contiguous()
    w = torch.randn(Cout, Cin, 1, 1, generator=g) / Cin ** 0.5
    bias = torch.randn(Cout, generator=g) * 0.1
    top = torch.randn(B, Cout, H // 2, W // 2, generator=g)
    ref = F.conv2d(x, w, bias) + F.interpolate(top, scale_factor=2.0, mode="nearest")
    out = torch.full((B, H, W, 16 + Cout + 16), 7.0).cuda()
    ore.conv2d(buf.cuda(), ore.pack_conv_weight(w).cuda(), Cout, 1, 1, in_coff=32, Cin=Cin, shift=dev(bias), add=nhwc(top), out=out, out_coff=16)
    o = out.cpu()
    assert rel_err(o[..., 16:16 + Cout].permute(0, 3, 1, 2).numpy(), ref.numpy()) < TOL
    assert (o[..., :16] == 7.0).all() and (o[..., 16 + Cout:] == 7.0).all()
    for bm, bn, sb in ((16, 16, 4), (32, 32, 4), (32, 64, 2), (64, 64, 2)):
        ore.lib().ore_conv_set_plan_override(-13, bm, bn, 4, sb)
        w3 = torch.randn(80, 96, 3, 3, generator=g) / (96 * 9) ** 0.5
        x3 = torch.randn(1, 96, 9, 8, generator=g)
        sc, sh = torch.rand(80, generator=g) + 0.5, torch.randn(80, generator=g) * 0.1
        ref3 = F.relu(F.conv2d(x3, w3, None, 1, 1) * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))
        y3, cs = ore.conv2d(nhwc(x3), ore.pack_conv_weight(w3).cuda(), 80, 3, 1, scale=dev(sc), shift=dev(sh), relu_cout=80, want_colsum=True)
        assert rel_err(nchw(y3).numpy(), ref3.numpy()) < TOL
        assert rel_err(cs.sum(0)[:80].cpu().numpy(), ref3.sum((0, 2, 3)).numpy()) < 1e-5


@pytest.fixture
def rf_forced(ore):
    """Force the register-fed small-M kernel (k_conv_rf, csrc/ore_conv_rf.hip) wherever it applies, then restore the plan."""
    with ore.conv_overrides((-10, 2), (-12, 0)):
        yield


RF_BUILDS = [(1, 4, 8), (1, 4, 12), (1, 4, 16), (1, 8, 12), (1, 8, 16), (1, 8, 20), (1, 16, 12), (2, 4, 12), (2, 4, 16), (2, 8, 12)]


@pytest.mark.parametrize("B,H,W,Cin,Cout,k,stride", [
    (1, 20, 20, 112, 112, 3, 1),    # stage-5 layers 1 / 2: 63 chunks, 7 per tap
    (1, 20, 20, 384, 112, 3, 1),    # stage-5 layer 0: 216 chunks -> 16 waves
    (1, 20, 20, 512, 128, 1, 1),    # FPN lateral 5
    (1, 40, 40, 96, 96, 3, 1),      # stage-4 layers 1 / 2: 6 chunks per tap
    (1, 40, 40, 256, 96, 3, 1),     # stage-4 layer 0: 144 chunks -> 8 waves
    (1, 40, 40, 384, 128, 1, 1),    # FPN lateral 4
    (1, 1, 320, 8192, 128, 1, 1),   # the second-stage GEMM: 512 chunks, several batches per wave
    (2, 13, 11, 96, 40, 3, 1),      # two images, odd size, rows not a multiple of 16, Cout = 40 (padded to 48, last quad partly live)
    (1, 9, 7, 112, 5, 3, 1),        # Cout = 5: one channel quad + one lane of the next
    (3, 17, 15, 128, 64, 3, 2),     # stride 2, odd size, three images
    (1, 5, 5, 720, 512, 1, 1),      # many output channels (forced: the plan leaves these to k_conv_kw)
])
def test_conv_rf_kernel_vs_oracle(ore, rf_forced, B, H, W, Cin, Cout, k, stride):
    """k_conv_rf against F.conv2d at 1e-4 on the shapes it serves (and the awkward ones: partial tiles, partial channel quads, border
    taps through the buffer descriptor's range check, stride 2, empty tail chunks of the last wave), bit-reproducible."""
    g = torch.Generator().manual_seed(B * 1000 + H + Cin + Cout + k)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
    sc = torch.rand(Cout, generator=g) + 0.5
    sh = torch.randn(Cout, generator=g) * 0.1
    ref = F.relu(F.conv2d(x, w, None, stride, k // 2) * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))
    wp = ore.pack_conv_weight(w).cuda()
    y = ore.conv2d(nhwc(x), wp, Cout, k, stride, scale=dev(sc), shift=dev(sh), relu_cout=Cout)
    assert rel_err(nchw(y).numpy(), ref.numpy()) < TOL
    assert chan_err(nchw(y).numpy(), ref.numpy()) < TOL
    assert torch.equal(y, ore.conv2d(nhwc(x), wp, Cout, k, stride, scale=dev(sc), shift=dev(sh), relu_cout=Cout))
    with ore.conv_overrides((-10, 0), (-12, 0)):                                      # and it really was another kernel than k_conv_kw's sum order
        y_kw = ore.conv2d(nhwc(x), wp, Cout, k, stride, scale=dev(sc), shift=dev(sh), relu_cout=Cout)
    assert rel_err(y.cpu().numpy(), y_kw.cpu().numpy()) < 2e-5


@pytest.mark.parametrize("gb,nw,maxs", RF_BUILDS)
@pytest.mark.parametrize("H,W,Cin,Cout,k", [(20, 20, 112, 112, 3), (7, 9, 96, 48, 3), (1, 96, 2048, 128, 1)])
def test_conv_rf_every_build(ore, rf_forced, gb, nw, maxs, H, W, Cin, Cout, k):
    """Every instantiated (tile width, waves, steps per batch) build of k_conv_rf on a 3x3 layer with 7 and with 6 chunks per tap and on
    a deep 1x1 layer: one batch, several batches, waves whose range lies wholly beyond K."""
    L = ore.lib()
    g = torch.Generator().manual_seed(H + Cin + nw + maxs)
    x = torch.randn(1, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
    sh = torch.randn(Cout, generator=g) * 0.1
    ref = F.conv2d(x, w, sh, 1, k // 2)
    L.ore_conv_set_plan_override(-11, gb, nw, maxs, 0)
    y = ore.conv2d(nhwc(x), ore.pack_conv_weight(w).cuda(), Cout, k, 1, shift=dev(sh))
    assert rel_err(nchw(y).numpy(), ref.numpy()) < TOL


def test_conv_rf_slices_add_colsum(ore, rf_forced):
    """Channel-slice input / output inside wider buffers, the FPN top-down addend (nearest-2x) and the fused per-tile column sums."""
    g = torch.Generator().manual_seed(5)
    B, H, W, Cin, Cout = 1, 10, 12, 128, 128
    buf = torch.randn(B, H, W, 32 + Cin + 16, generator=g)
    x = buf[..., 32:32 + Cin].permute(0, 3, 1, 2).contiguous()
    w = torch.randn(Cout, Cin, 1, 1, generator=g) / Cin ** 0.5
    bias = torch.randn(Cout, generator=g) * 0.1
    top = torch.randn(B, Cout, H // 2, W // 2, generator=g)
    ref = F.conv2d(x, w, bias) + F.interpolate(top, scale_factor=2.0, mode="nearest")
    out = torch.full((B, H, W, 16 + Cout + 16), 7.0).cuda()
    ore.conv2d(buf.cuda(), ore.pack_conv_weight(w).cuda(), Cout, 1, 1, in_coff=32, Cin=Cin, shift=dev(bias), add=nhwc(top), out=out, out_coff=16)
    o = out.cpu()
    assert rel_err(o[..., 16:16 + Cout].permute(0, 3, 1, 2).numpy(), ref.numpy()) < TOL
    assert (o[..., :16] == 7.0).all() and (o[..., 16 + Cout:] == 7.0).all()              # nothing outside the slice is written
    ore.lib().ore_conv_set_plan_override(-11, 1, 4, 8, 0)                                 # forced build: column sums allowed
    w3 = torch.randn(48, 96, 3, 3, generator=g) / (96 * 9) ** 0.5
    x3 = torch.randn(1, 96, 9, 8, generator=g)
    sc, sh = torch.rand(48, generator=g) + 0.5, torch.randn(48, generator=g) * 0.1
    ref3 = F.relu(F.conv2d(x3, w3, None, 1, 1) * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))
    y3, cs = ore.conv2d(nhwc(x3), ore.pack_conv_weight(w3).cuda(), 48, 3, 1, scale=dev(sc), shift=dev(sh), relu_cout=48, want_colsum=True)
    assert rel_err(nchw(y3).numpy(), ref3.numpy()) < TOL
    assert rel_err(cs.sum(0)[:48].cpu().numpy(), ref3.sum((0, 2, 3)).numpy()) < 1e-5


@pytest.mark.parametrize("nw,tile", [(8, (16, 16)), (8, (16, 32)), (8, (16, 48)), (16, (16, 16)), (16, (16, 32))])
@pytest.mark.parametrize("H,W,Cin,Cout,k,S", [(20, 20, 112, 112, 3, 1), (1, 96, 2048, 128, 1, 1), (13, 11, 48, 48, 3, 1), (20, 20, 384, 112, 3, 2)])
def test_conv_kw_wave_counts(ore, kw_forced, nw, tile, H, W, Cin, Cout, k, S):
    """k_conv_kw with the K dimension split over 8 / 16 waves of one block (template NW; the production plan uses 8 waves for the
    second-stage GEMM): every instantiated (tile, NW) pair, few and many chunks per tap, with and without a cross-block split, against
    F.conv2d at 1e-4, bit-reproducible."""
    g = torch.Generator().manual_seed(H + Cin + nw)
    x = torch.randn(1, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
    sh = torch.randn(Cout, generator=g) * 0.1
    ref = F.relu(F.conv2d(x, w, sh, 1, k // 2))
    with ore.conv_overrides((-6, nw), (-3, tile[0], tile[1], 2, S)):     # (on top of kw_forced; every override is reset afterwards)
        y = ore.conv2d(nhwc(x), ore.pack_conv_weight(w).cuda(), Cout, k, 1, shift=dev(sh), relu_cout=Cout)
        y2 = ore.conv2d(nhwc(x), ore.pack_conv_weight(w).cuda(), Cout, k, 1, shift=dev(sh), relu_cout=Cout)
    assert rel_err(nchw(y).numpy(), ref.numpy()) < TOL
    assert torch.equal(y, y2)


def test_conv_kw_slices_add_colsum_levels(ore, kw_forced):
    """k_conv_kw with everything the engine asks of it: channel-slice input and output inside wider buffers (OSA concat), the FPN
    nearest-2x top-down add, partial ReLU, fused per-tile column sums (eSE average pool), several pyramid levels in one launch with
    per-level epilogue parameters."""
    g = torch.Generator().manual_seed(11)
    B, H, W = 1, 20, 24
    buf = torch.randn(B, 160, H, W, generator=g)                                  # read channels 32..143 (112)
    w = torch.randn(80, 112, 3, 3, generator=g) * 0.03
    top = torch.randn(B, 80, (H + 1) // 2, (W + 1) // 2, generator=g)
    bias = torch.randn(80, generator=g)
    ref = F.conv2d(buf[:, 32:144], w, bias, 1, 1) + F.interpolate(top, scale_factor=2.0, mode="nearest")[:, :, :H, :W]
    ref[:, :50] = F.relu(ref[:, :50])
    out = torch.full((B, H, W, 128), -7.0).cuda()
    ore.conv2d(nhwc(buf), ore.pack_conv_weight(w).cuda(), 80, 3, 1, in_coff=32, Cin=112, shift=dev(bias), relu_cout=50, add=nhwc(top),
               out=out, out_coff=16)
    o = nchw(out)
    assert rel_err(o[:, 16:96].numpy(), ref.numpy()) < TOL
    assert (o[:, :16] == -7.0).all() and (o[:, 96:] == -7.0).all()
    # fused column sums: sum over the tile partials == column sums of the output
    x = torch.relu(torch.randn(1, 544, 40, 40, generator=g))
    wc = torch.randn(384, 544, 1, 1, generator=g) / 544 ** 0.5
    sc, sh = torch.rand(384, generator=g) + 0.5, torch.randn(384, generator=g) * 0.1
    y, parts = ore.conv2d(nhwc(x), ore.pack_conv_weight(wc).cuda(), 384, 1, 1, scale=dev(sc), shift=dev(sh), relu_cout=384, want_colsum=True)
    refc = F.relu(F.conv2d(x, wc) * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))
    assert rel_err(nchw(y).numpy(), refc.numpy()) < TOL
    assert rel_err(parts.sum(0)[:384].cpu().numpy(), refc.sum((0, 2, 3)).numpy()) < TOL
    # three pyramid levels in one launch, per-level scale / shift (the head's tower / conv3 form)
    HW = [(20, 24), (10, 12), (5, 6)]
    xs = [torch.randn(1, 128, h, w_, generator=g) for h, w_ in HW]
    wl = torch.randn(128, 128, 3, 3, generator=g) * 0.03
    scl, shl = torch.rand(3, 128, generator=g) + 0.5, torch.randn(3, 128, generator=g) * 0.1
    rows = torch.cat([nhwc(t).reshape(-1, 128) for t in xs], 0)
    yl = ore.conv2d_levels(rows, HW, 1, ore.pack_conv_weight(wl).cuda(), 128, 3, scale=dev(scl), shift=dev(shl), ep_stride=128)
    r0 = 0
    for l, (h, w_) in enumerate(HW):
        refl = F.conv2d(xs[l], wl, None, 1, 1) * scl[l].view(1, -1, 1, 1) + shl[l].view(1, -1, 1, 1)
        got = yl[r0:r0 + h * w_].reshape(1, h, w_, 128).permute(0, 3, 1, 2).cpu()
        assert rel_err(got.numpy(), refl.numpy()) < TOL, l
        r0 += h * w_


def test_conv_rejects_bad_shapes(ore):
    x = torch.zeros(1, 4, 4, 24).cuda()
    with pytest.raises(ore.OreError):
        ore.conv2d(x, torch.zeros(16 * 24).cuda(), 16, 1)  # Cin % 16 != 0


# ------------------------------------------------------------------------------------------ stem / pool / eSE
@pytest.mark.parametrize("u8", [True, False])
def test_stem1_fused_preprocess(ore, sd, golden, u8):
    g = golden("preprocess_75x100")
    img = torch.from_numpy(g["image"])
    name = "backbone.bottom_up.stem.stem_1"
    ref = R.conv_bn_relu(torch.from_numpy(g["x"]), sd, name, 2, 1)  # golden x = reference ImageList output
    sc, sh = bn_fold(sd, name)
    xin = dev(img if u8 else img.float())[None]
    y = ore.stem1(xin, 96, 128, R.PIXEL_MEAN, R.PIXEL_STD, dev(sd[name + "/conv.weight"]), dev(sc), dev(sh))
    assert rel_err(nchw(y).numpy(), ref.numpy()) < TOL


@pytest.mark.parametrize("H,W,C", [(21, 21, 112), (160, 160, 112), (5, 8, 256), (2, 3, 16), (40, 40, 384)])
def test_maxpool_ceil(ore, H, W, C):
    x = torch.relu(torch.randn(2, C, H, W, generator=torch.Generator().manual_seed(H)))
    gate = torch.rand(2, C, generator=torch.Generator().manual_seed(W))
    ref = F.max_pool2d(x * gate[:, :, None, None], 3, 2, ceil_mode=True)
    y = ore.maxpool3x3s2(nhwc(x), dev(gate))
    assert tuple(y.shape[1:3]) == tuple(ref.shape[2:])
    assert torch.equal(nchw(y), ref)  # exact: positive scaling commutes with max


@pytest.mark.parametrize("H,W,C,rows", [(160, 160, 112, 0), (80, 80, 256, 128), (40, 40, 384, 128), (21, 13, 48, 16)])
def test_ese_gate_pool_one_launch(ore, H, W, C, rows):
    """ore_ese_gate_pool_fwd (gate + gate-scaled consumer weight + max-pool of x * gate in one launch, the bs = 1 engine's form) against
    the separate entry points: same gate bits, same scaled weight, pooled output exactly max-pool(x) * gate."""
    g = torch.Generator().manual_seed(H + C)
    x = torch.relu(torch.randn(1, C, H, W, generator=g))
    fw = torch.randn(C, C, 1, 1, generator=g) / C ** 0.5
    fb = torch.randn(C, generator=g)
    P = 37
    xr = nhwc(x).reshape(-1, C)
    part = torch.stack([c.sum(0) for c in xr.chunk(P, 0)])                              # any split of the rows into partial sums
    P = part.shape[0]
    wp = (torch.randn(rows, C, generator=g).cuda() if rows else None)
    gate, pooled, ws = ore.ese_gate_pool(part.contiguous(), dev(fw), dev(fb), nhwc(x), wp)
    ref = F.relu6(F.conv2d(F.adaptive_avg_pool2d(x, 1), fw, fb) + 3.0) / 6.0
    assert rel_err(gate.cpu().numpy().reshape(-1), ref.numpy().reshape(-1)) < TOL
    if rows:
        g2, ws2 = ore.ese_gate_scaled_weight(part.contiguous(), H * W, dev(fw), dev(fb), wp)
        assert torch.equal(g2, gate) and torch.equal(ws2, ws)
    else:
        assert ws is None and torch.equal(ore.ese_gate_from_colsum(part.contiguous(), H * W, dev(fw), dev(fb)), gate)
    assert torch.equal(pooled, ore.maxpool3x3s2(nhwc(x), gate))
    xb = nhwc(x).to(torch.bfloat16)
    gb, pb, wsb = ore.ese_gate_pool(part.contiguous(), dev(fw), dev(fb), xb, wp if rows and C % 32 == 0 else None)
    assert torch.equal(gb, gate) and pb.dtype == torch.bfloat16
    want = (F.max_pool2d(xb.float().permute(0, 3, 1, 2), 3, 2, ceil_mode=True) * gate.view(1, -1, 1, 1)).to(torch.bfloat16)
    assert torch.equal(pb.permute(0, 3, 1, 2), want)
    if wsb is not None:
        assert wsb.dtype == torch.bfloat16 and torch.equal(wsb, ws.to(torch.bfloat16))


@pytest.mark.parametrize("HW,C", [((160, 160), 112), ((20, 20), 512), ((3, 5), 256), ((80, 80), 256)])
def test_ese_gate(ore, HW, C):
    g = torch.Generator().manual_seed(C)
    x = torch.relu(torch.randn(2, C, *HW, generator=g))
    fw = torch.randn(C, C, 1, 1, generator=g) / C ** 0.5
    fb = torch.randn(C, generator=g)
    ref = F.relu6(F.conv2d(F.adaptive_avg_pool2d(x, 1), fw, fb) + 3.0) / 6.0
    gate = ore.ese_gate(nhwc(x), dev(fw), dev(fb))
    assert rel_err(gate.cpu().numpy(), ref[:, :, 0, 0].numpy()) < 1e-5
    y = ore.scale_channels(nhwc(x), gate)
    assert rel_err(nchw(y).numpy(), (x * ref).numpy()) < 1e-5


@pytest.mark.parametrize("name,k", [("osa_stage3_odd", 3), ("osa_stage5", 5)])
def test_osa_stage_golden(ore, sd, golden, name, k):
    """maxpool(ceil) -> 3 convs writing slices of ONE concat buffer -> 1x1 concat -> eSE, vs the reference run."""
    g = golden(name)
    x = torch.from_numpy(g["x"])
    p = f"backbone.bottom_up.stage{k}.OSA{k}_1."
    cin = x.shape[1]
    sc = sd[f"{p}layers.0.OSA{k}_1_0/conv.weight"].shape[0]
    pooled = ore.maxpool3x3s2(nhwc(x))
    B, H, W, _ = pooled.shape
    cat = torch.zeros(B, H, W, cin + 3 * sc).cuda()
    cat[..., :cin] = pooled
    src, dst = 0, cin
    for i in range(3):
        conv_bn(ore, cat, sd, f"{p}layers.{i}.OSA{k}_1_{i}", 3, 1, in_coff=src, Cin=cin if i == 0 else sc, out=cat, out_coff=dst)
        src, dst = dst, dst + sc
    y = conv_bn(ore, cat, sd, f"{p}concat.OSA{k}_1_concat", 1, 1)
    gate = ore.ese_gate(y, dev(sd[p + "ese.fc.weight"]), dev(sd[p + "ese.fc.bias"]))
    y = ore.scale_channels(y, gate)
    assert rel_err(nchw(y).numpy(), g["y"]) < TOL
    assert chan_err(nchw(y).numpy(), g["y"]) < TOL


# ------------------------------------------------------------------------------------------ correlation / head
def test_correlation_golden(ore, sd, golden):
    g = golden("correlation")
    w3 = ore.pack_conv_weight(sd["conv3.weight"]).cuda()
    for k in ("p3", "p4", "p5"):
        q = torch.from_numpy(g["q_" + k])
        proto = dev(torch.from_numpy(g["s_" + k])[0])
        k11, k13, k31 = ore.support_kernels(proto)
        r11, r13, r31 = R.support_kernels(torch.from_numpy(g["s_" + k]))
        assert rel_err(k11.cpu().numpy(), r11.numpy()) < 1e-5
        assert rel_err(k13.cpu().numpy(), r13.numpy()) < 1e-5
        assert rel_err(k31.cpu().numpy(), r31.numpy().T if r31.shape[0] != k31.shape[0] else r31.numpy()) < 1e-5
        B, C, H, W = q.shape
        pcat = torch.zeros(B, H, W, 2 * C).cuda()
        pcat[..., C:] = nhwc(q)
        ore.correlation(pcat, k11, k13, k31, out=pcat, q_coff=C, out_coff=0, Cc=C)
        y = ore.conv2d(pcat, w3, C, 1, shift=dev(sd["conv3.bias"]), relu_cout=C)
        assert rel_err(nchw(y).numpy(), g["out_" + k]) < TOL, k
        assert chan_err(nchw(y).numpy(), g["out_" + k]) < TOL, k


def head_level(ore, sd, x_nhwc, l):
    h = "proposal_generator.centernet_head."
    C = x_nhwc.shape[-1]
    t = ore.conv2d(x_nhwc, ore.pack_conv_weight(sd[h + "bbox_tower.0.weight"]).cuda(), C, 3, shift=dev(sd[h + "bbox_tower.0.bias"]))
    mul, add = ore.groupnorm_affine(t, 32, dev(sd[h + "bbox_tower.1.weight"]), dev(sd[h + "bbox_tower.1.bias"]))
    s = float(sd[h + f"scales.{l}.scale"])
    w5 = torch.cat([sd[h + "bbox_pred.weight"], sd[h + "agn_hm.weight"]], 0)
    scale = torch.tensor([s, s, s, s, 1.0])
    shift = torch.cat([sd[h + "bbox_pred.bias"] * s, sd[h + "agn_hm.bias"]])
    out = torch.zeros(*x_nhwc.shape[:3], 8).cuda()
    ore.conv2d(t, ore.pack_conv_weight(w5).cuda(), 5, 3, scale=dev(scale), shift=dev(shift), relu_cout=4, in_mul=mul,
               in_add=add, in_relu=True, out=out)
    return out


def test_centernet_head_golden(ore, sd, golden):
    g = golden("cn_head")
    for l in range(3):
        out = head_level(ore, sd, nhwc(torch.from_numpy(g[f"x{l}"])), l)
        o = nchw(out)
        assert rel_err(o[:, :4].numpy(), g[f"reg{l}"]) < TOL
        assert rel_err(o[:, 4:5].numpy(), g[f"hm{l}"]) < TOL


# ------------------------------------------------------------------------------------------ detection tail
def run_detect(ore, hms, regs, pre_topk, nms_thr, post_topk, thr=1e-5):
    heads = []
    for hm, reg in zip(hms, regs):
        h = torch.zeros(hm.shape[0], hm.shape[1], 8)
        h[..., :4] = torch.from_numpy(reg)
        h[..., 4] = torch.from_numpy(hm)
        heads.append(h.cuda())
    o = ore.detect(heads, (8, 16, 32)[: len(hms)], thr, pre_topk, nms_thr, post_topk)
    n_pre, n_keep = (int(v) for v in o["counts"][:2].cpu())
    return {"pre_boxes": o["pre_boxes"][:n_pre].cpu().numpy(), "pre_scores": o["pre_scores"][:n_pre].cpu().numpy(),
            "pre_loc": o["pre_loc"][:n_pre].cpu().numpy(), "pre_level": o["pre_level"][:n_pre].cpu().numpy(),
            "keep": o["keep_idx"][:n_keep].cpu().numpy(), "boxes": o["out_boxes"][:n_keep].cpu().numpy(),
            "scores": o["out_scores"][:n_keep].cpu().numpy()}


def assert_detect_equal(a, b):
    for k in ("pre_boxes", "pre_scores", "pre_loc", "pre_level", "keep", "boxes", "scores"):
        assert a[k].shape == b[k].shape, (k, a[k].shape, b[k].shape)
        assert np.array_equal(a[k], b[k]), k  # bit-exact, floats included


@pytest.mark.parametrize("tag", ["sparse", "dense"])
@pytest.mark.parametrize("cfg", [(1000, 0.6, 256), (4000, 0.9, 2000), (1000, 0.6, 100000), (50, 0.3, 10)])
def test_detect_bit_exact_vs_oracle(ore, golden, tag, cfg):
    g = golden(f"cn_infer_640_{tag}")
    hms, regs = [g[f"hm{l}"] for l in range(3)], [g[f"reg{l}"] for l in range(3)]
    pre_topk, nms_thr, post_topk = cfg
    ref = odec.decode_nms(hms, regs, (8, 16, 32), 1e-5, pre_topk, nms_thr, post_topk)
    got = run_detect(ore, hms, regs, pre_topk, nms_thr, post_topk)
    assert_detect_equal(got, ref)


@pytest.mark.parametrize("tag", ["sparse", "dense"])
def test_detect_vs_reference_run(ore, golden, tag):
    g = golden(f"cn_infer_640_{tag}")
    got = run_detect(ore, [g[f"hm{l}"] for l in range(3)], [g[f"reg{l}"] for l in range(3)], 1000, 0.6, 256)
    assert got["boxes"].shape == g["boxes"].shape
    np.testing.assert_allclose(got["scores"], g["scores"], rtol=2e-6)
    np.testing.assert_allclose(got["boxes"], g["boxes"], rtol=2e-6, atol=1e-5)


@pytest.mark.parametrize("tag,pre_topk,nms_thr,post_topk", [("sparse", 1000, 0.6, 256), ("dense", 1000, 0.6, 256), ("train", 4000, 0.9, 2000)])
def test_detect_indices_vs_reference_run(ore, golden, tag, pre_topk, nms_thr, post_topk):
    """north_star: bit-exact box indices / NMS keep masks vs the reference CPU path.  tests/golden/cn_infer_640_*_idx.npz hold the
    int64 index tensors of the EXECUTED reference (oracle/refrun/gen_golden.py::gen_cn_indices): per-level selected flat
    locations, the rows left by the post-NMS filter in the canonical pre order; eval thresholds on two maps, the training
    thresholds (4000 / 0.9 / 2000) on a third.  The HIP path must reproduce them with np.array_equal (keep lists up to the order
    inside a run of exactly tied scores, which the reference's topk(sorted=False) leaves undefined -- same_keep_list)."""
    from test_oracle_golden import same_keep_list
    gi = golden(f"cn_infer_640_{tag}_idx")
    g = gi if tag == "train" else golden(f"cn_infer_640_{tag}")
    got = run_detect(ore, [g[f"hm{l}"] for l in range(3)], [g[f"reg{l}"] for l in range(3)], pre_topk, nms_thr, post_topk)
    base = np.cumsum([0] + [g[f"hm{l}"].size for l in range(3)])
    for l in range(3):
        mine = got["pre_loc"][got["pre_level"] == l].astype(np.int64) - base[l]
        assert np.array_equal(mine, gi[f"sel{l}"]), l
    same_keep_list(got["keep"].astype(np.int64), gi["post_keep"], got["pre_scores"])
    full = ore.nms(torch.from_numpy(got["pre_boxes"]).cuda(), torch.from_numpy(got["pre_scores"]).cuda(), nms_thr)
    same_keep_list(full.cpu().numpy().astype(np.int64), gi["nms_keep"], got["pre_scores"])


def test_detect_ties_and_edge_cases(ore):
    rng = np.random.default_rng(3)
    # heavy score ties (quantised logits) + identical boxes: exercises tie-breaking in top-k, sort and post-top-k
    hms = [np.round(rng.normal(0, 2, (s, s)) * 2) / 2 for s in (24, 12, 6)]
    regs = [np.round(np.abs(rng.normal(2, 1, (s, s, 4))) * 2) / 2 for s in (24, 12, 6)]
    hms = [h.astype(np.float32) for h in hms]
    regs = [r.astype(np.float32) for r in regs]
    for cfg in ((100, 0.5, 20), (1000, 0.7, 50), (7, 0.6, 3)):
        ref = odec.decode_nms(hms, regs, (8, 16, 32), 1e-5, *cfg)
        assert_detect_equal(run_detect(ore, hms, regs, *cfg), ref)
    # nothing passes the threshold
    none = [np.full((4, 4), -30.0, np.float32)]
    ref = odec.decode_nms(none, [np.ones((4, 4, 4), np.float32)], (8,), 1e-5, 10, 0.6, 5)
    got = run_detect(ore, none, [np.ones((4, 4, 4), np.float32)], 10, 0.6, 5)
    assert len(got["keep"]) == 0 and len(ref["keep"]) == 0 and len(got["pre_scores"]) == 0
    # single location
    one = [np.full((1, 1), 3.0, np.float32)]
    assert_detect_equal(run_detect(ore, one, [np.ones((1, 1, 4), np.float32)], 10, 0.6, 5),
                        odec.decode_nms(one, [np.ones((1, 1, 4), np.float32)], (8,), 1e-5, 10, 0.6, 5))


def test_nms_standalone(ore):
    rng = np.random.default_rng(0)
    for n in (0, 1, 2, 63, 64, 65, 300, 2400):
        b = rng.uniform(0, 200, (n, 2)).astype(np.float32)
        wh = rng.uniform(5, 60, (n, 2)).astype(np.float32)
        boxes = np.concatenate([b, b + wh], 1)
        scores = np.round(rng.uniform(0, 1, n), 2).astype(np.float32)  # ties
        for thr in (0.3, 0.6, 0.9):
            keep = ore.nms(torch.from_numpy(boxes).cuda(), torch.from_numpy(scores).cuda(), thr).cpu().numpy()
            assert np.array_equal(keep, odec.nms(boxes, scores, thr)), (n, thr)


# ------------------------------------------------------------------------------------------ engine
@pytest.fixture(scope="module")
def engine(ore, sd):
    e = ore.Engine(max_batch=2, max_h=640, max_w=640)
    e.load_state_dict(sd)
    e.set_support(R.synth_support(0))
    e.finalize()
    yield e
    e.close()


def test_engine_backbone_golden(engine, golden):
    g = golden("backbone_fpn_96x128")
    # the fixture input is already normalised; the engine fuses (x - mean)/std into stem_1, so add the mean back
    x = torch.from_numpy(g["x"]) + torch.tensor(R.PIXEL_MEAN).view(1, 3, 1, 1)
    out = engine.backbone(x.contiguous().cuda())
    for k in ("p3", "p4", "p5"):
        assert tuple(out[k].shape) == g[k].shape
        assert rel_err(out[k].cpu().numpy(), g[k]) < TOL, k
        assert chan_err(out[k].cpu().numpy(), g[k]) < TOL, k


@pytest.mark.parametrize("use_graph", [False, True])
def test_engine_eval_640_vs_oracle(engine, sd, use_graph):
    """BASELINE config[1] shape: 640x640 synthetic image, 25-shot cached support, bs=1."""
    img = R.synth_image(0)
    ref = R.eval_dense(img, sd, R.synth_support(0))
    for _ in range(2 if use_graph else 1):  # second call replays the captured graph
        engine.eval_forward(img.cuda(), use_graph=use_graph)
    torch.cuda.synchronize()
    for l, k in enumerate(("p3", "p4", "p5")):
        s = 640 >> (l + 3)
        assert rel_err(engine.buffer(k, (1, s, s)).cpu().numpy(), ref["features"][k].numpy()) < TOL, k
        assert rel_err(engine.buffer(f"pos{l + 3}", (1, s, s)).cpu().numpy(), ref["pos_features"][l].numpy()) < TOL
        assert chan_err(engine.buffer(k, (1, s, s)).cpu().numpy(), ref["features"][k].numpy()) < TOL, k
        assert chan_err(engine.buffer(f"pos{l + 3}", (1, s, s)).cpu().numpy(), ref["pos_features"][l].numpy()) < CHAN_TOL_DEEP
        hd = engine.buffer(f"head{l + 3}", (1, s, s)).cpu()
        assert rel_err(hd[:, :4].numpy(), ref["reg"][l].numpy()) < TOL
        assert rel_err(hd[:, 4:5].numpy(), ref["hm"][l].numpy()) < TOL
    # detection tail: bit-exact against the oracle fed with the SAME (GPU-produced) head outputs
    hms, regs = [], []
    for l in range(3):
        s = 640 >> (l + 3)
        hd = engine.buffer(f"head{l + 3}").cpu().numpy().reshape(s, s, 5)
        hms.append(np.ascontiguousarray(hd[..., 4]))
        regs.append(np.ascontiguousarray(hd[..., :4]))
    want = odec.decode_nms(hms, regs, (8, 16, 32), 1e-5, 1000, 0.6, 256)
    boxes, scores, keep = engine.proposals()
    assert np.array_equal(keep.cpu().numpy(), want["keep"])
    assert np.array_equal(boxes.cpu().numpy(), want["boxes"])
    assert np.array_equal(scores.cpu().numpy(), want["scores"])
    assert len(want["keep"]) > 0


def test_engine_on_reference_demo_images(ore, sd, golden):
    """BASELINE configs[0]'s inputs (ref:directory/0000{0,1}.png resized to 320x320 as the reference's predictor does; the R-50-C4
    model of that config is out of scope per SURVEY 2, so the VoVNet path stands in): the whole first stage on real ore images
    against the oracle at 1e-4, the detection tail bit-exact on the engine's own head outputs."""
    g = golden("demo_images_320")
    e = ore.Engine(max_batch=1, max_h=320, max_w=320)
    e.load_state_dict(sd)
    e.set_support(R.synth_support(0))
    e.finalize()
    for i in range(2):
        img = torch.from_numpy(g["images"][i])
        assert img.dtype == torch.uint8 and tuple(img.shape) == (3, 320, 320)
        ref = R.eval_dense(img, sd, R.synth_support(0))
        e.eval_forward(img.cuda(), use_graph=bool(i))
        e.eval_forward(img.cuda(), use_graph=bool(i))
        torch.cuda.synchronize()
        hms, regs = [], []
        for l, k in enumerate(("p3", "p4", "p5")):
            s = 320 >> (l + 3)
            assert rel_err(e.buffer(k, (1, s, s)).cpu().numpy(), ref["features"][k].numpy()) < TOL, k
            hd = e.buffer(f"head{l + 3}", (1, s, s)).cpu()
            assert rel_err(hd[:, :4].numpy(), ref["reg"][l].numpy()) < TOL
            assert rel_err(hd[:, 4:5].numpy(), ref["hm"][l].numpy()) < TOL
            assert chan_err(e.buffer(k, (1, s, s)).cpu().numpy(), ref["features"][k].numpy()) < TOL, k
            raw = e.buffer(f"head{l + 3}").cpu().numpy().reshape(s, s, 5)
            hms.append(np.ascontiguousarray(raw[..., 4]))
            regs.append(np.ascontiguousarray(raw[..., :4]))
        want = odec.decode_nms(hms, regs, (8, 16, 32), 1e-5, 1000, 0.6, 256)
        boxes, scores, keep = e.proposals()
        assert np.array_equal(keep.cpu().numpy(), want["keep"]) and np.array_equal(boxes.cpu().numpy(), want["boxes"])
        assert np.array_equal(scores.cpu().numpy(), want["scores"])
    e.close()


def test_engine_eval_non_divisible_size(engine, sd):
    img = R.synth_image(1, 300, 420)  # padded to 320x448 inside stem_1
    ref = R.eval_dense(img, sd, R.synth_support(0))
    engine.eval_forward(img.cuda(), use_graph=False)
    torch.cuda.synchronize()
    for l, k in enumerate(("p3", "p4", "p5")):
        hh, ww = 320 >> (l + 3), 448 >> (l + 3)
        assert rel_err(engine.buffer(k, (1, hh, ww)).cpu().numpy(), ref["features"][k].numpy()) < TOL
        hd = engine.buffer(f"head{l + 3}", (1, hh, ww)).cpu()
        assert rel_err(hd[:, 4:5].numpy(), ref["hm"][l].numpy()) < TOL


@pytest.mark.parametrize("hw", [(480, 640), (544, 736), (600, 800)])
def test_engine_eval_other_sizes_vs_oracle(ore, sd, hw):
    """Sizes whose layer shapes select other kernels / tile mappings than 640x640 (stage 2 on the double-buffered patch kernel with
    partial tiles in W, tile grids that are not multiples of 8 under the XCD mapping, a non-/32 input that stem_1 pads): the whole first
    stage against the oracle at 1e-4, the detection tail bit-exact on the engine's own head outputs."""
    H, W = hw
    Hp, Wp = (H + 31) // 32 * 32, (W + 31) // 32 * 32
    img = R.synth_image(5 + H, H, W)
    ref = R.eval_dense(img, sd, R.synth_support(0))
    e = ore.Engine(max_batch=1, max_h=Hp, max_w=Wp)
    e.load_state_dict(sd)
    e.set_support(R.synth_support(0))
    e.finalize()
    try:
        for use_graph in (False, True):
            e.eval_forward(img.cuda(), use_graph=use_graph)
            torch.cuda.synchronize()
            hms, regs = [], []
            for l, k in enumerate(("p3", "p4", "p5")):
                hh, ww = Hp >> (l + 3), Wp >> (l + 3)
                assert rel_err(e.buffer(k, (1, hh, ww)).cpu().numpy(), ref["features"][k].numpy()) < TOL, (k, use_graph)
                hd = e.buffer(f"head{l + 3}", (1, hh, ww)).cpu()
                assert rel_err(hd[:, :4].numpy(), ref["reg"][l].numpy()) < TOL and rel_err(hd[:, 4:5].numpy(), ref["hm"][l].numpy()) < TOL
                raw = e.buffer(f"head{l + 3}").cpu().numpy().reshape(hh, ww, 5)
                hms.append(np.ascontiguousarray(raw[..., 4]))
                regs.append(np.ascontiguousarray(raw[..., :4]))
            want = odec.decode_nms(hms, regs, (8, 16, 32), 1e-5, 1000, 0.6, 256)
            boxes, scores, keep = e.proposals()
            assert np.array_equal(keep.cpu().numpy(), want["keep"]) and np.array_equal(boxes.cpu().numpy(), want["boxes"])
    finally:
        e.close()


# ------------------------------------------------------------------------------------------ module surface (fewx registry)
@pytest.fixture(scope="module")
def model(ore, sd):
    import os
    from conftest import PKG
    from fewx.config import get_cfg
    from detectron2.modeling import build_model
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(PKG, "configs", "fsod", "finetune_vovnet.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", "cuda", "INPUT.MAX_SIZE_TEST", 640])
    cfg.freeze()
    m = build_model(cfg)
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith("roi_heads.") for k in missing), (missing, unexpected)
    sup = R.synth_support(0)
    m.set_support_dict({**{k: {0: v} for k, v in sup.items()}, "rcnn_8": {0: torch.zeros(24, 128, 8, 8)}, "rcnn_4": {0: torch.zeros(24, 128, 4, 4)}})
    return m.eval()


def test_module_backbone_forward_golden(model, golden):
    """build_fcos_vovnet_fpn_backbone(...).forward through the layer-by-layer HIP modules (reference call protocol)."""
    g = golden("backbone_fpn_96x128")
    with torch.no_grad():
        out = model.backbone(torch.from_numpy(g["x"]).cuda())
    for k in ("p3", "p4", "p5"):
        assert tuple(out[k].shape) == g[k].shape
        assert rel_err(out[k].cpu().numpy(), g[k]) < TOL, k
        assert chan_err(out[k].cpu().numpy(), g[k]) < TOL, k


def test_module_sm_block_golden(model, golden):
    for lvl in (3, 5):
        g = golden(f"sm_block_p{lvl}")
        with torch.no_grad():
            y = getattr(model, f"vip_p{lvl}")(torch.from_numpy(g["x"]).cuda())
        assert rel_err(y[:1].cpu().numpy(), g["y0"]) < TOL
        assert rel_err(y.permute(0, 3, 2, 1).mean(0, True).cpu().numpy(), g["proto"]) < TOL


def test_module_head_and_proposal_generator(model, golden):
    g = golden("cn_head")
    with torch.no_grad():
        _, regs, hms = model.proposal_generator.centernet_head([torch.from_numpy(g[f"x{l}"]).cuda() for l in range(3)])
    for l in range(3):
        assert rel_err(regs[l].cpu().numpy(), g[f"reg{l}"]) < TOL
        assert rel_err(hms[l].cpu().numpy(), g[f"hm{l}"]) < TOL


def test_detector_inference_proposals_vs_oracle(model, sd):
    img = R.synth_image(5, 320, 320)
    props = model.inference_proposals([{"image": img}])[0]
    e = model._engine
    hms, regs = [], []
    for l in range(3):
        s = 320 >> (l + 3)
        hd = e.buffer(f"head{l + 3}").cpu().numpy().reshape(s, s, 5)
        hms.append(np.ascontiguousarray(hd[..., 4]))
        regs.append(np.ascontiguousarray(hd[..., :4]))
    ref = R.eval_dense(img, sd, R.synth_support(0))
    for l in range(3):
        assert rel_err(hms[l], ref["hm"][l][0, 0].numpy()) < TOL
    want = odec.decode_nms(hms, regs, (8, 16, 32), 1e-5, 1000, 0.6, 256)
    assert np.array_equal(props.proposal_boxes.tensor.cpu().numpy(), want["boxes"])
    assert np.array_equal(props.objectness_logits.cpu().numpy(), want["scores"])
    assert props.pred_classes.dtype == torch.int64 and int(props.pred_classes.abs().sum()) == 0


# ------------------------------------------------------------------------------------------ second stage
def _roi_inputs(seed=1, n=300):
    g = torch.Generator().manual_seed(seed)
    feats = [torch.randn(1, 128, s, s, generator=g) for s in (40, 20, 10)]          # a 320x320 image
    ctr = torch.rand(n, 2, generator=g) * 320
    wh = torch.exp(torch.rand(n, 2, generator=g) * 4.5 + 1.0)                         # 2.7 .. 245 px: hits all three levels
    props = torch.cat([ctr - wh / 2, ctr + wh / 2], 1)
    props[:5] = torch.tensor([[-20.0, -30.0, 50.0, 40.0], [300.0, 300.0, 400.0, 380.0], [10.0, 10.0, 10.01, 10.01],
                              [0.0, 0.0, 320.0, 320.0], [100.0, 100.0, 101.0, 300.0]])  # out of image, tiny, whole image, thin
    props[5:9] = torch.tensor([[-100.0, -100.0, 400.0, 420.0], [-60.0, 0.0, 420.0, 460.0], [10.0, -200.0, 500.0, 330.0],
                               [0.0, 0.0, 448.0, 448.0]])                              # sqrt(area) >= 448 -> p5
    sup = torch.randn(24, 128, 8, 8, generator=g) * 0.1
    return feats, props, sup


def test_roi_align_vs_oracle(ore):
    feats, props, _ = _roi_inputs()
    lv = R.assign_levels(props)
    assert set(lv.tolist()) == {0, 1, 2}
    ref = R.roi_pool_levels(feats, props, 8)                                          # [R,C,8,8]
    x = ore.roi_align([nhwc(f) for f in feats], props.cuda(), (8, 16, 32), 8)
    got = x.view(len(props), 64, 128).permute(0, 2, 1).reshape(len(props), 128, 8, 8).cpu()
    assert rel_err(got.numpy(), ref.numpy()) < 1e-5


def test_roi_stage_vs_oracle(ore):
    feats, props, sup = _roi_inputs(2)
    sd = R.synth_roi_state(R.synth_state_dict(0))
    ref = R.roi_head_eval(feats, props, sup, sd, (320, 320), 0.0, 0.9, 100)
    x = ore.roi_align([nhwc(f) for f in feats], props.cuda(), (8, 16, 32), 8)
    Wp, bp = ore.compose_roi_head(sd, sup)
    h = ore.conv2d(x.view(1, 1, *x.shape), Wp.cuda(), 128, 1, shift=bp.cuda(), relu_cout=128).view(len(props), 128)
    assert rel_err(h.cpu().numpy(), ref["h"].numpy()) < TOL                           # composed linear chain == layer sequence
    p = "roi_heads.box_predictor.0."
    det = ore.roi_predict(h, dev(sd[p + "cls_score.weight"]), dev(sd[p + "cls_score.bias"]), dev(sd[p + "bbox_pred.weight"]),
                          dev(sd[p + "bbox_pred.bias"]), props.cuda(), (10.0, 10.0, 5.0, 5.0), (320, 320), 0.0, 0.9, 100)
    k = int(det["count"].item())
    # bit-exact against the C twin fed with the SAME fc1 output
    want = odec.roi_predict(h.cpu().numpy(), sd[p + "cls_score.weight"].numpy(), sd[p + "cls_score.bias"].numpy(),
                            sd[p + "bbox_pred.weight"].numpy(), sd[p + "bbox_pred.bias"].numpy(), props.numpy(), (10.0, 10.0, 5.0, 5.0),
                            (320, 320), 0.0, 0.9, 100)
    assert k == len(want["scores"]) == 100
    assert np.array_equal(det["boxes"][:k].cpu().numpy(), want["boxes"])
    assert np.array_equal(det["scores"][:k].cpu().numpy(), want["scores"])
    assert np.array_equal(det["src"][:k].cpu().numpy(), want["src"])
    # and close to the all-oracle result (its h differs by float rounding)
    np.testing.assert_allclose(det["scores"][:k].cpu().numpy(), ref["scores"], rtol=1e-3, atol=1e-5)


def test_roi_stage_vs_reference_run(ore, golden):
    """f1 pinned by the EXECUTED reference (tests/golden/roi_stage_eval.npz: CustomCascadeROIHeads._forward_box/_run_stage,
    CustomFastRCNNOutputLayers.predict_probs, FastRCNNOutputLayers.predict_boxes, fast_rcnn_inference): pooled features, fc1
    output, final detections.  MULT_PROPOSAL_SCORE is not applied (the shadowed `_forward_box`)."""
    g = golden("roi_stage_eval")
    sd = R.synth_roi_state(R.synth_state_dict(0), 0)
    feats = [torch.from_numpy(g[k]) for k in ("p3", "p4", "p5")]
    props, sup = torch.from_numpy(g["proposals"]), torch.from_numpy(g["sup8"])
    hw = tuple(int(v) for v in g["image_hw"])
    x = ore.roi_align([nhwc(f) for f in feats], props.cuda(), (8, 16, 32), 8)
    got = x.view(len(props), 64, 128).permute(0, 2, 1).reshape(len(props), 128, 8, 8).cpu()
    assert rel_err(got[g["sub"]].numpy(), g["box_features_sub"]) < 1e-5
    Wp, bp = ore.compose_roi_head(sd, sup)
    h = ore.conv2d(x.view(1, 1, *x.shape), Wp.cuda(), 128, 1, shift=bp.cuda(), relu_cout=128).view(len(props), 128)
    assert rel_err(h.cpu().numpy(), g["h"]) < TOL
    p = "roi_heads.box_predictor.0."
    det = ore.roi_predict(h, dev(sd[p + "cls_score.weight"]), dev(sd[p + "cls_score.bias"]), dev(sd[p + "bbox_pred.weight"]),
                          dev(sd[p + "bbox_pred.bias"]), props.cuda(), (10.0, 10.0, 5.0, 5.0), hw, 0.0, 0.9, 100)
    k = int(det["count"].item())
    assert k == len(g["scores"])
    np.testing.assert_allclose(det["scores"][:k].cpu().numpy(), g["scores"], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(det["boxes"][:k].cpu().numpy(), g["pred_boxes"], rtol=1e-4, atol=2e-2)


def test_roi_heads_module_vs_reference_run(model, golden):
    """The same fixture through the product's registered module, called with the reference's protocol
    `roi_heads(images, features, [rcnn_8, rcnn_4], proposals, targets)` (fsod_roi_heads.py:368-402)."""
    from detectron2.structures import Boxes, ImageList, Instances
    g = golden("roi_stage_eval")
    sd = R.synth_roi_state(R.synth_state_dict(0), 0)
    model.load_state_dict({k: v for k, v in sd.items() if k.startswith("roi_heads.")}, strict=False)
    model.eval()
    hw = tuple(int(v) for v in g["image_hw"])
    prop = Instances(hw)
    prop.proposal_boxes = Boxes(torch.from_numpy(g["proposals"]).cuda())
    prop.objectness_logits = torch.from_numpy(g["proposal_scores"]).cuda()
    feats = {k: torch.from_numpy(g[k]).cuda() for k in ("p3", "p4", "p5")}
    res, _ = model.roi_heads(ImageList(torch.empty(0), [hw]), feats, [torch.from_numpy(g["sup8"]).cuda(), torch.from_numpy(g["sup4"]).cuda()],
                             [prop], None)
    r = res[0]
    assert len(r) == len(g["scores"]) and r.image_size == hw
    np.testing.assert_allclose(r.scores.cpu().numpy(), g["scores"], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(r.pred_boxes.tensor.cpu().numpy(), g["pred_boxes"], rtol=1e-4, atol=2e-2)
    assert r.pred_classes.dtype == torch.int64 and int(r.pred_classes.abs().sum()) == 0


def test_detector_end_to_end(model, sd):
    """model(batched_inputs) -> [{"instances": Instances(pred_boxes, scores, pred_classes)}], the reference call protocol."""
    sd2 = R.synth_roi_state(sd)
    sd2["roi_heads.box_head.0.fc1.weight"] = sd2["roi_heads.box_head.0.fc1.weight"] * 0.01   # keep logits/deltas un-saturated
    model.load_state_dict({k: v for k, v in sd2.items() if k.startswith("roi_heads.")}, strict=False)
    g = torch.Generator().manual_seed(9)
    sup = R.synth_support(0)
    rc8 = torch.randn(24, 128, 8, 8, generator=g) * 0.1
    model.set_support_dict({**{k: {0: v} for k, v in sup.items()}, "rcnn_8": {0: rc8}, "rcnn_4": {0: torch.zeros(24, 128, 4, 4)}})
    img = R.synth_image(5, 320, 320)
    out = model([{"image": img, "height": 640, "width": 640}])          # output resolution 2x the input
    inst = out[0]["instances"]
    assert inst.image_size == (640, 640) and len(inst) <= 100 and len(inst) > 0
    # oracle: same second stage on the GPU-produced proposals and FPN features
    e = model._engine
    props = model.inference_proposals([{"image": img}])[0].proposal_boxes.tensor.cpu()
    feats = [e.buffer(f"p{l}", (1, 320 >> l, 320 >> l)).cpu().contiguous() for l in (3, 4, 5)]
    ref = R.roi_head_eval(feats, props, rc8, {k: v.cpu() for k, v in model.state_dict().items()}, (320, 320), 0.0, 0.9, 100)
    n = min(len(inst), len(ref["scores"]))
    assert abs(len(inst) - len(ref["scores"])) <= 2, (len(inst), len(ref["scores"]))   # empty boxes may be dropped by detector_postprocess
    got_scores = inst.scores.cpu().numpy()
    assert 0.05 < float(np.median(ref["scores"])) < 0.999, "synthetic second-stage scores should not be saturated"
    np.testing.assert_allclose(np.sort(got_scores)[::-1][:n], np.sort(ref["scores"])[::-1][:n], rtol=1e-3, atol=1e-5)
    np.testing.assert_allclose(inst.pred_boxes.tensor.cpu().numpy()[:n] / 2.0, ref["boxes"][:n], rtol=1e-3, atol=0.05)
    assert inst.pred_classes.dtype == torch.int64
    b = inst.pred_boxes.tensor
    assert float(b.min()) >= 0 and float(b[:, 2].max()) <= 640 and float(b[:, 3].max()) <= 640
    # the in-graph second stage (engine, 512-row GEMM) and the module-level forward (per-op calls, n-row GEMM -> another split-K
    # plan) are the same kernels up to float summation order
    assert getattr(e, "has_roi", False)
    e.eval_forward(img.cuda(), use_graph=True)
    eb, es, _ = e.detections()
    from detectron2.structures import ImageList
    proposals = model.inference_proposals([{"image": img}])
    feats_d = {f"p{l}": e.buffer(f"p{l}", (1, 320 >> l, 320 >> l)) for l in (3, 4, 5)}
    res, _ = model.roi_heads(ImageList(torch.empty(0), [(320, 320)]), feats_d, [rc8.cuda(), None], proposals, None)
    assert len(es) == len(res[0].scores)
    np.testing.assert_allclose(res[0].scores.cpu().numpy(), es.cpu().numpy(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(res[0].pred_boxes.tensor.cpu().numpy(), eb.cpu().numpy(), rtol=1e-4, atol=1e-2)


def test_engine_detect_call_equals_python_postprocess(model, sd):
    """ore_engine_detect_fwd (both stages + detector_postprocess as the last kernel of the graph, count through pinned memory)
    returns exactly what d2z:modeling/postprocessing.py computes from the engine's raw detections: anisotropic output size, device and
    host images, uint8 and float32."""
    from detectron2.modeling.postprocessing import detector_postprocess
    from detectron2.structures import Boxes, Instances
    sd2 = R.synth_roi_state(sd)
    sd2["roi_heads.box_head.0.fc1.weight"] = sd2["roi_heads.box_head.0.fc1.weight"] * 0.01
    model.load_state_dict({k: v for k, v in sd2.items() if k.startswith("roi_heads.")}, strict=False)
    g = torch.Generator().manual_seed(9)
    sup = R.synth_support(0)
    rc8 = torch.randn(24, 128, 8, 8, generator=g) * 0.1
    model.set_support_dict({**{k: {0: v} for k, v in sup.items()}, "rcnn_8": {0: rc8}, "rcnn_4": {0: torch.zeros(24, 128, 4, 4)}})
    img = R.synth_image(6, 320, 352)
    for image, (oh, ow) in ((img, (480, 800)), (img.cuda(), (320, 352)), (img.float(), (200, 111)), (img.cuda(), (480, 800))):
        out = model([{"image": image, "height": oh, "width": ow}])[0]["instances"]
        e = model._engine
        b, s_, _ = e.detections()                                        # raw second-stage output of the same forward
        raw = Instances((320, 352))
        raw.pred_boxes, raw.scores = Boxes(b.clone()), s_.clone()
        raw.pred_classes = torch.zeros(len(s_), dtype=torch.int64, device=s_.device)
        want = detector_postprocess(raw, oh, ow)
        assert out.image_size == (oh, ow) and len(out) == len(want) and len(out) > 0
        assert torch.equal(out.pred_boxes.tensor, want.pred_boxes.tensor) and torch.equal(out.scores, want.scores)
        assert out.pred_boxes.tensor.is_cuda and out.pred_classes.dtype == torch.int64


def test_detector_inference_many_equals_one_at_a_time(model, sd):
    """CenterNet2Detector.inference_many: single-image requests of two sizes, folded per size into batched engine passes, return
    the detections of the reference protocol (one image per forward) in request order."""
    sd2 = R.synth_roi_state(sd)
    sd2["roi_heads.box_head.0.fc1.weight"] = sd2["roi_heads.box_head.0.fc1.weight"] * 0.01
    model.load_state_dict({k: v for k, v in sd2.items() if k.startswith("roi_heads.")}, strict=False)
    g = torch.Generator().manual_seed(9)
    rc8 = torch.randn(24, 128, 8, 8, generator=g) * 0.1
    model.set_support_dict({**{k: {0: v} for k, v in R.synth_support(0).items()}, "rcnn_8": {0: rc8}, "rcnn_4": {0: torch.zeros(24, 128, 4, 4)}})
    reqs = [{"image": R.synth_image(20 + i, *hw)} for i, hw in enumerate([(320, 320), (256, 384), (320, 320), (320, 320), (256, 384)])]
    many = model.inference_many(reqs, max_fold=3)
    assert len(many) == len(reqs)
    for r, got in zip(reqs, many):
        one = model([r])[0]["instances"]
        gi = got["instances"]
        assert gi.image_size == one.image_size and len(gi) == len(one) and len(one) > 0
        np.testing.assert_allclose(gi.scores.cpu().numpy(), one.scores.cpu().numpy(), rtol=1e-4, atol=1e-6)
        # the folded pass reduces the eSE pools in another order (1e-7 on the gates): detections whose scores agree to 1e-4 may swap
        # places in the score-sorted list, so the boxes are matched as a set among rows of (nearly) equal score
        gb, ob = gi.pred_boxes.tensor.cpu().numpy(), one.pred_boxes.tensor.cpu().numpy()
        gs, os_ = gi.scores.cpu().numpy(), one.scores.cpu().numpy()
        used = np.zeros(len(gb), dtype=bool)
        for i in range(len(ob)):
            cand = np.nonzero(~used & (np.abs(gs - os_[i]) <= 1e-4 * abs(os_[i]) + 1e-6))[0]
            hit = [j for j in cand if np.allclose(gb[j], ob[i], rtol=1e-4, atol=0.05)]
            assert hit, "detection %d of the one-at-a-time pass (score %.6f) has no partner in the folded pass" % (i, os_[i])
            used[hit[0]] = True


# ------------------------------------------------------------------------------------------ batched-level / fused entry points
def test_conv_fused_colsum_and_gate(ore):
    """The concat conv's epilogue column sums (eSE average pool) + gate kernel == avgpool -> fc -> hsigmoid."""
    g = torch.Generator().manual_seed(11)
    for (H, W, Cin, Cout) in ((80, 80, 352, 256), (20, 20, 720, 512), (160, 160, 320, 112), (7, 9, 64, 48)):
        x = torch.randn(1, Cin, H, W, generator=g)
        w = torch.randn(Cout, Cin, 1, 1, generator=g) / Cin ** 0.5
        fw = torch.randn(Cout, Cout, 1, 1, generator=g) / Cout ** 0.5
        fb = torch.randn(Cout, generator=g)
        y_ref = F.relu(F.conv2d(x, w))
        gate_ref = F.relu6(F.conv2d(F.adaptive_avg_pool2d(y_ref, 1), fw, fb) + 3.0) / 6.0
        y, cs = ore.conv2d(nhwc(x), ore.pack_conv_weight(w).cuda(), Cout, 1, relu_cout=Cout, want_colsum=True)
        assert rel_err(nchw(y).numpy(), y_ref.numpy()) < TOL
        assert rel_err(cs.sum(0)[:Cout].cpu().numpy(), y_ref.sum((0, 2, 3)).numpy()) < 1e-5
        gate = ore.ese_gate_from_colsum(cs[:, :Cout].contiguous(), H * W, dev(fw), dev(fb))
        assert rel_err(gate.cpu().numpy(), gate_ref[:, :, 0, 0].numpy()) < 1e-5


def test_levels_entry_points_match_per_level(ore, sd):
    g = torch.Generator().manual_seed(12)
    B, C = 2, 128
    HW = [(20, 24), (10, 12), (5, 6)]
    feats = [torch.randn(B, C, h, w, generator=g) for h, w in HW]
    rows = torch.cat([nhwc(f).reshape(-1, C) for f in feats], 0).contiguous()
    # 3x3 conv + per-level scale/shift + input affine/relu, one launch vs per level
    w = torch.randn(5, C, 3, 3, generator=g) * 0.05
    wp = ore.pack_conv_weight(w).cuda()
    scale = torch.rand(3, 16, generator=g) + 0.5
    shift = torch.randn(3, 16, generator=g)
    mul = torch.rand(3 * B, C, generator=g) + 0.5
    add = torch.randn(3 * B, C, generator=g) * 0.1
    out = torch.zeros(rows.shape[0], 8).cuda()
    ore.conv2d_levels(rows, HW, B, wp, 5, 3, scale=dev(scale), shift=dev(shift), ep_stride=16, relu_cout=4, in_mul=dev(mul),
                      in_add=dev(add), in_relu=True, out=out)
    r0 = 0
    for l, (h, wd) in enumerate(HW):
        xin = F.relu(feats[l] * mul[l * B:(l + 1) * B, :, None, None] + add[l * B:(l + 1) * B, :, None, None])
        ref = F.conv2d(xin, w, None, 1, 1) * scale[l, :5].view(1, -1, 1, 1) + shift[l, :5].view(1, -1, 1, 1)
        ref[:, :4] = F.relu(ref[:, :4])
        got = out[r0:r0 + B * h * wd, :5].reshape(B, h, wd, 5).permute(0, 3, 1, 2).cpu()
        assert rel_err(got.numpy(), ref.numpy()) < TOL, l
        r0 += B * h * wd
    # GroupNorm statistics over levels
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    m, a = ore.groupnorm_affine_levels(rows, [h * w for h, w in HW], B, 32, dev(gamma), dev(beta))
    for l, f in enumerate(feats):
        ref = F.group_norm(f, 32, gamma, beta, 1e-5)
        got = f * m[l * B:(l + 1) * B].cpu()[:, :, None, None] + a[l * B:(l + 1) * B].cpu()[:, :, None, None]
        assert rel_err(got.numpy(), ref.numpy()) < 1e-5
    # correlation over levels
    sup = R.synth_support(0)
    ks = [R.support_kernels(sup[k]) for k in ("p3", "p4", "p5")]
    k11 = torch.stack([k[0] for k in ks]); k13 = torch.stack([k[1] for k in ks]); k31 = torch.stack([k[2] for k in ks])
    attn = ore.correlation_levels(rows, HW, B, dev(k11), dev(k13), dev(k31), C)
    r0 = 0
    for l, (h, wd) in enumerate(HW):
        q = feats[l]
        a1 = F.relu(F.conv2d(F.relu(F.conv2d(q, k11[l].view(C, 1, 1, 1), groups=C)), k11[l].view(C, 1, 1, 1), groups=C))
        b1 = F.relu(F.conv2d(q, k13[l].view(C, 1, 1, 3), padding=(0, 1), groups=C))
        b1 = F.relu(F.conv2d(b1, k31[l].view(C, 1, 3, 1), padding=(1, 0), groups=C))
        ref = a1 + b1 + q
        got = attn[r0:r0 + B * h * wd].reshape(B, h, wd, C).permute(0, 3, 1, 2).cpu()
        assert rel_err(got.numpy(), ref.numpy()) < 1e-5
        r0 += B * h * wd


@pytest.mark.parametrize("M_hw,Cin,Cout,k,splitk", [((20, 20), 384, 112, 3, 4), ((20, 20), 512, 128, 1, 0), ((40, 40), 256, 96, 3, 3),
                                                    ((40, 40), 544, 384, 1, 0), ((5, 5), 128, 128, 3, 0), ((80, 80), 112, 80, 3, 0)])
def test_conv_inkernel_splitk_repeatable(ore, M_hw, Cin, Cout, k, splitk):
    """In-kernel last-arriver split-K: correct, bitwise repeatable, and leaves the arrival counters at zero."""
    g = torch.Generator().manual_seed(Cin + Cout)
    x = torch.randn(1, Cin, *M_hw, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
    ref = F.conv2d(x, w, None, 1, k // 2)
    xd, wp = nhwc(x), ore.pack_conv_weight(w).cuda()
    outs = [ore.conv2d(xd, wp, Cout, k, splitk=splitk).clone() for _ in range(3)]
    assert rel_err(nchw(outs[0]).numpy(), ref.numpy()) < TOL
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[1], outs[2])
    ws = ore._default_ws(xd.device)
    assert int(ws[:4096].view(torch.int32).abs().sum()) == 0


# ------------------------------------------------------------------------------------------ 3x3 patch kernel (forced on small shapes)
@pytest.mark.parametrize("mode", [102, 16, 8, 4])
def test_conv3x3_patch_kernel(ore, mode):
    g = torch.Generator().manual_seed(21 + mode)
    with ore.conv_overrides((-1, mode)):
        for (B, H, W, Cin, Cout) in ((2, 17, 23, 32, 64), (1, 40, 40, 128, 128), (1, 9, 33, 16, 64), (1, 64, 48, 64, 192)):
            x = torch.randn(B, Cin, H, W, generator=g)
            w = torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5
            sc, sh = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.1
            ref = F.relu(F.conv2d(x, w, None, 1, 1) * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))
            # read a channel slice of a wider buffer, write a slice of a wider buffer (OSA concat usage)
            xin = torch.zeros(B, H, W, Cin + 16).cuda()
            xin[..., 16:] = nhwc(x)
            out = torch.full((B, H, W, Cout + 32), -3.0).cuda()
            ore.conv2d(xin, ore.pack_conv_weight(w).cuda(), Cout, 3, 1, in_coff=16, Cin=Cin, scale=dev(sc), shift=dev(sh), relu_cout=Cout,
                       out=out, out_coff=32, splitk=1)
            o = nchw(out)
            assert rel_err(o[:, 32:].numpy(), ref.numpy()) < TOL, (mode, B, H, W, Cin, Cout)
            assert (o[:, :32] == -3.0).all()
        # multi-level (head tower shape): one launch over three levels with per-level epilogue parameters
        B, C = 2, 64
        HW = [(20, 24), (10, 12), (5, 6)]
        feats = [torch.randn(B, C, h, w, generator=g) for h, w in HW]
        rows = torch.cat([nhwc(f).reshape(-1, C) for f in feats], 0).contiguous()
        w = torch.randn(128, C, 3, 3, generator=g) * 0.05
        scale, shift = torch.rand(3, 128, generator=g) + 0.5, torch.randn(3, 128, generator=g)
        out = ore.conv2d_levels(rows, HW, B, ore.pack_conv_weight(w).cuda(), 128, 3, scale=dev(scale), shift=dev(shift), ep_stride=128,
                                relu_cout=100, splitk=1)
        r0 = 0
        for l, (h, wd) in enumerate(HW):
            ref = F.conv2d(feats[l], w, None, 1, 1) * scale[l].view(1, -1, 1, 1) + shift[l].view(1, -1, 1, 1)
            ref[:, :100] = F.relu(ref[:, :100])
            got = out[r0:r0 + B * h * wd].reshape(B, h, wd, 128).permute(0, 3, 1, 2).cpu()
            assert rel_err(got.numpy(), ref.numpy()) < TOL, (mode, l)
            r0 += B * h * wd


def test_engines_on_concurrent_streams_are_bit_identical(model):
    """bench.py keeps several bs=1 forwards in flight, each on its own engine + stream: every engine must produce what a single
    sequential engine produces (no shared scratch, split-K counters or graphs between engines)."""
    e0 = model.engine()
    engines = [e0] + [model.make_engine() for _ in range(3)]
    streams = [torch.cuda.Stream() for _ in engines]
    imgs = [R.synth_image(20 + i, 320, 320).cuda() for i in range(4)]
    want = []
    for im in imgs:
        e0.eval_forward(im)
        torch.cuda.synchronize()
        want.append([t.clone() for t in e0.proposals()] + [t.clone() for t in e0.detections()])
    torch.cuda.synchronize()
    for rep in range(3):
        for k, (e, s) in enumerate(zip(engines, streams)):
            with torch.cuda.stream(s):
                e.eval_forward(imgs[(k + rep) % 4])
        torch.cuda.synchronize()
        for k, e in enumerate(engines):
            got = list(e.proposals()) + list(e.detections())
            assert all(torch.equal(a, b) for a, b in zip(got, want[(k + rep) % 4])), (rep, k)
    for e in engines[1:]:
        e.close()


def test_compute_support_dict_vs_oracle(model, sd, tmp_path):
    """init_model's compute (support crops -> prototypes + rcnn_8/rcnn_4) on the HIP kernels vs the oracle; pickle round trip."""
    from oracle import ref_train as T
    import pickle
    old = model.support_dict
    try:
        _, _, sup, sbox = T.synth_train_inputs(3, (64, 64), n_gt=1, shots=5, support_hw=144)
        out = model.compute_support_dict(sup, sbox, cls_id=7, merge=True)
        sf = R.backbone_fpn(T.preprocess_batch(sup), sd)
        for i, k in enumerate(("p3", "p4", "p5")):
            ref = R.support_prototype(sf[k], sd, 3 + i)
            assert tuple(out[k][7].shape) == tuple(ref.shape)
            assert rel_err(out[k][7].numpy(), ref.numpy()) < TOL, k
        for key, P in (("rcnn_8", 8), ("rcnn_4", 4)):
            ref = torch.cat([R.roi_pool_levels([sf[k][n:n + 1] for k in ("p3", "p4", "p5")], sbox[n:n + 1], P) for n in range(5)], 0)
            assert rel_err(out[key][7].numpy(), ref.numpy()) < TOL, key
        f = str(tmp_path / "support_dir" / "support_feature.pkl")
        model.save_support_file(f)
        with open(f, "rb") as fh:
            back = pickle.load(fh)
        assert set(back) == {"p3", "p4", "p5", "rcnn_8", "rcnn_4"} and torch.equal(back["p4"][7], out["p4"][7])
    finally:
        model.set_support_dict({k: {c: t.cpu() for c, t in v.items()} for k, v in old.items()})


def test_init_model_walks_the_support_dataframe(model, tmp_path):
    """init_model without a support_feature.pkl (ref fsod_cen.py:321-408): per category the first SUPPORT_SHOT rows of the support
    dataframe (reset_index order) -> crops + boxes -> compute_support_dict; the pickle is written in the reference's layout and a
    second model start reads it back.  Dataframe and image reader are synthetic (the ore dataset is not shipped)."""
    import pandas as pd
    import pickle
    from oracle import ref_train as T
    old = model.support_dict
    shot = model.support_shot
    try:
        rows, crops = [], {}
        for cls in (3, 9):
            _, _, sup, sbox = T.synth_train_inputs(20 + cls, (64, 64), n_gt=1, shots=shot + 2, support_hw=144)
            for i in range(shot + 2):
                path = f"support/{cls}_{i}.png"
                crops["./x/" + path] = sup[i].permute(1, 2, 0).to(torch.uint8).numpy()
                rows.append({"id": 100 * cls + i, "image_id": 50 + i, "category_id": cls, "file_path": path, "support_box": sbox[i].tolist()})
        df = pd.DataFrame(rows).sample(frac=1.0, random_state=1)                     # shuffled: the walk keeps dataframe order per class
        want = {}
        for cls in (3, 9):
            sel = df.loc[df["category_id"] == cls].iloc[:shot]
            imgs = [torch.as_tensor(crops["./x/" + p].transpose(2, 0, 1).copy()) for p in sel["file_path"]]
            want[cls] = model.compute_support_dict(imgs, torch.tensor(sel["support_box"].tolist()), cls_id=cls, merge=False)
        model.support_dict = None
        f = str(tmp_path / "support_dir" / "support_feature.pkl")
        model.init_model(support_file=f, support_df=df, read_image=lambda p, format=None: crops[p], image_root="./x")
        assert set(model.support_dict) == {"p3", "p4", "p5", "rcnn_8", "rcnn_4"} and set(model.support_dict["p3"]) == {3, 9}
        for cls in (3, 9):
            for k in ("p3", "p4", "p5", "rcnn_8", "rcnn_4"):
                assert torch.equal(model.support_dict[k][cls].cpu(), want[cls][k][cls]), (cls, k)
        assert tuple(model.support_dict["rcnn_8"][3].shape) == (shot, 128, 8, 8)
        with open(f, "rb") as fh:
            back = pickle.load(fh)
        assert torch.equal(back["p5"][9], want[9]["p5"][9])
        model.support_dict = None
        model.init_model(support_file=f)                                             # second start: the pickle is simply read
        assert torch.equal(model.support_dict["p4"][3].cpu(), want[3]["p4"][3])
    finally:
        model.set_support_dict({k: {c: t.cpu() for c, t in v.items()} for k, v in old.items()})


def test_eval_end_to_end_vs_reference_run(ore, golden, tmp_path):
    """The product's whole eval path -- `init_model` walking a support dataframe, then `model([{image, height, width}])` -- against
    the reference's own init_model + inference EXECUTED end to end (tests/golden/eval_end_to_end.npz, ref:fewx/modeling/fsod/
    fsod_cen.py:309-408, :417-535) on the two shipped demo images: support features at 1e-4, detections as a set (boxes to 0.05 px on
    the 300x300 output, scores to 1e-3 relative)."""
    import os
    from conftest import PKG
    from fewx.config import get_cfg
    from detectron2.modeling import build_model
    from oracle import ref_train as RT
    from test_oracle_golden import _match_detections, eval_end_to_end_state
    g = golden("eval_end_to_end")
    shots = int(g["shots"])
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(PKG, "configs", "fsod", "finetune_vovnet.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", "cuda", "INPUT.FS.SUPPORT_SHOT", shots])
    cfg.freeze()
    m = build_model(cfg).eval()
    missing, unexpected = m.load_state_dict(eval_end_to_end_state(), strict=False)
    assert not unexpected and not missing, (missing, unexpected)
    m.init_model(support_file=str(tmp_path / "support_dir" / "support_feature.pkl"), support_df=RT.eval_support_df(shots),
                 read_image=RT.eval_support_crop)
    for k in ("p3", "p4", "p5", "rcnn_8", "rcnn_4"):
        assert set(m.support_dict[k]) == {1}
        assert rel_err(m.support_dict[k][1].cpu().numpy(), g["support_" + k]) < TOL, k
    from near_tie import guided_nms_explain, match_rows
    imgs = golden("demo_images_320")["images"]
    H = W = imgs.shape[-1]
    for i in range(2):
        for rep in range(2):                                                # second call = hipGraph replay
            out = m([{"image": torch.from_numpy(imgs[i]), "height": 300, "width": 300}])[0]["instances"]
        rb, rs = g[f"img{i}_boxes"], g[f"img{i}_scores"]
        ob, osc = out.pred_boxes.tensor.cpu().numpy(), out.scores.cpu().numpy()
        assert out.image_size == (300, 300) and (out.pred_classes == 0).all()
        ok = _match_detections(ob, osc, rb, rs, 0.05, 1e-3)
        # ---- every row on which the two outputs differ is a near-tie of one of the two greedy NMS passes, or its cascade (tests/near_tie.py).
        # The walk runs on THIS path's candidate rows (read back from the engine that just served the call) and lets the reference's
        # output decide only decisions within 2e-5 of the IoU threshold / 2e-6 relative of a score cut; with identical outputs it
        # needs no such decision (measured on MI355X, round 5: both images match row for row, boxes to 1e-3 px, 0 ambiguous decisions).
        e = m._engine
        n_pre, n_prop = (int(v) for v in e.buffer("counts")[:2, 0].tolist())
        pb, ps = e.buffer("pre_boxes")[:n_pre].cpu().numpy(), e.buffer("pre_scores")[:n_pre, 0].cpu().numpy()
        # first stage: candidates -> NMS 0.6 -> score >= 256th (ref:fewx/modeling/fsod/fsod_rpn.py:1185-1210)
        s1 = guided_nms_explain(pb, ps, g[f"img{i}_prop_boxes"], g[f"img{i}_prop_scores"], 0.6, post_topk=256, box_tol=2e-2, score_rtol=2e-4)
        assert s1["unexplained"] == [], (i, "proposals", s1["unexplained"][:6])
        props = e.proposals()[0].cpu().numpy()
        which = match_rows(props, e.proposals()[1].cpu().numpy(), g[f"img{i}_prop_boxes"], g[f"img{i}_prop_scores"], 2e-2, 2e-4)
        # second stage VALUES, proposal by proposal: box after apply_deltas + clip and foreground probability of every proposal both sides
        # have (ref:fewx/modeling/fsod/fsod_roi_heads.py:404-455 -> d2z:modeling/roi_heads/fast_rcnn.py:118-171 clips inside)
        raw_b, raw_s = e.buffer("roi_raw_boxes")[:n_prop].cpu().numpy(), e.buffer("roi_raw_scores")[:n_prop, 0].cpu().numpy()
        ref_b = g[f"img{i}_stage2_boxes"].copy()
        ref_b[:, 0::2] = ref_b[:, 0::2].clip(0, W)
        ref_b[:, 1::2] = ref_b[:, 1::2].clip(0, H)
        ref_s = g[f"img{i}_stage2_scores"][:, 0]
        both = np.where(which >= 0)[0]
        assert len(both) >= 0.97 * len(which), (len(both), len(which))
        assert np.abs(raw_b[which[both]] - ref_b[both]).max() <= 5e-2, float(np.abs(raw_b[which[both]] - ref_b[both]).max())
        assert (np.abs(raw_s[which[both]] - ref_s[both]) <= 1e-3 * ref_s[both] + 1e-6).all()
        # second stage decisions: score > 0.05 -> NMS 0.9 -> the best 100, in output coordinates (detector_postprocess scales by 300/320)
        okf = e.buffer("roi_ok")[:n_prop, 0].cpu().numpy() != 0
        # this engine runs fc1 K-split (8192 -> 128, cap 320): the rows exist only as partial sums, so the never-written "roi_h" is no buffer
        with pytest.raises(ore.OreError, match="unknown buffer 'roi_h'"):
            e.buffer("roi_h")
        s2 = guided_nms_explain(raw_b[okf] * (300.0 / W), raw_s[okf], rb, rs, 0.9, max_out=100, box_tol=5e-2, score_rtol=1e-3, drop_empty=True)
        assert s2["unexplained"] == [], (i, "detections", s2["unexplained"][:6])
        print(f"image {i}: {int(ok.sum())}/{len(ok)} detections match row for row; near-tie decisions used: proposals {s1['ambiguous']}, "
              f"detections {s2['ambiguous']}")
        # ... and the number of rows that needed an explanation at all stays small (a broken kernel would not hide behind "ties")
        assert ok.mean() >= 0.97 and abs(len(out) - len(rs)) <= 2, (i, ok.mean(), len(out), len(rs))
        assert s1["ambiguous"] + s2["ambiguous"] <= 4, (s1["ambiguous"], s2["ambiguous"])


def test_engine_batched_eval_matches_single_image_engines(ore, sd):
    """ore_engine_eval_batch_fwd: B independent images in one pass (dense stages batched, detection tail + second stage per image)
    against the bs = 1 path on each image: feature maps to 1e-5 (another tile plan = another summation order, never another result),
    every image's proposals BIT-EXACT against ref_decode.c on that image's own head outputs, detections equal to the bs = 1 engine's."""
    B = 3
    imgs = torch.stack([R.synth_image(10 + i) for i in range(B)]).cuda()
    roi_sd = R.synth_roi_state(sd, 0)
    sup8 = torch.randn(4, 128, 8, 8, generator=torch.Generator().manual_seed(3))

    def make(mb):
        e = ore.Engine(max_batch=mb, max_h=640, max_w=640)
        e.load_state_dict(sd)
        e.set_support(R.synth_support(0))
        e.finalize()
        e.set_roi_head(roi_sd, sup8, (10.0, 10.0, 5.0, 5.0), 0.05, 0.5, 100)
        return e
    eb, e1 = make(B), make(1)
    for use_graph in (False, True, True):
        eb.eval_forward_batch(imgs, use_graph=use_graph)
        torch.cuda.synchronize()
        for b in range(B):
            e1.eval_forward(imgs[b], use_graph=False)
            torch.cuda.synchronize()
            hms, regs = [], []
            for l in range(3):
                s = 640 >> (l + 3)
                for name in (f"p{l + 3}", f"pos{l + 3}", f"head{l + 3}"):
                    got = eb.buffer(name, (B, s, s))[b].cpu().numpy()
                    want = e1.buffer(name, (1, s, s))[0].cpu().numpy()
                    assert rel_err(got, want) < 1e-5, (name, b)
                hd = eb.buffer(f"head{l + 3}").cpu().numpy().reshape(B, s, s, 5)[b]
                hms.append(np.ascontiguousarray(hd[..., 4]))
                regs.append(np.ascontiguousarray(hd[..., :4]))
            want = odec.decode_nms(hms, regs, (8, 16, 32), 1e-5, 1000, 0.6, 256)
            boxes, scores, keep = eb.proposals(b)
            assert np.array_equal(keep.cpu().numpy(), want["keep"]) and len(want["keep"]) > 0
            assert np.array_equal(boxes.cpu().numpy(), want["boxes"]) and np.array_equal(scores.cpu().numpy(), want["scores"])
            db, ds, _ = eb.detections(b)
            d1, s1, _ = e1.detections(0)
            assert db.shape == d1.shape and db.shape[0] > 0
            # 1e-6 feature differences go through exp(dw) * proposal size: up to ~0.1 px on a 640-px box with the synthetic head
            assert float((db - d1).abs().max()) < 0.5 and float((ds - s1).abs().max()) < 1e-4     # boxes in pixels (of 640), scores in [0,1]
    eb.close()
    e1.close()


def test_engine_batched_eval_non_divisible_size_and_bf16(ore, sd):
    """Folded pass at a size that needs padding (300x420 -> 320x448) and in the bf16-operand mode: per-image heads equal the bs = 1
    engine of the same mode (1e-5 in fp32; in bf16 mode the batched tile plan rounds the same operands, so 1e-5 as well), proposals
    bit-exact against ref_decode.c on the image's own heads."""
    B = 2
    imgs = torch.stack([R.synth_image(30 + i, 300, 420) for i in range(B)]).cuda()
    for mode in ("fp32", "bf16"):
        prev = ore.set_conv_precision(mode)
        try:
            eb, e1 = ore.Engine(max_batch=B, max_h=320, max_w=448), ore.Engine(max_batch=1, max_h=320, max_w=448)
        finally:
            ore.set_conv_precision(prev)
        for e in (eb, e1):
            e.load_state_dict(sd)
            e.set_support(R.synth_support(0))
            e.finalize()
        eb.eval_forward_batch(imgs, use_graph=True)
        torch.cuda.synchronize()
        for b in range(B):
            e1.eval_forward(imgs[b], use_graph=False)
            torch.cuda.synchronize()
            hms, regs = [], []
            for l in range(3):
                hh, ww = 320 >> (l + 3), 448 >> (l + 3)
                got = eb.buffer(f"head{l + 3}", (B, hh, ww))[b].cpu().numpy()
                want = e1.buffer(f"head{l + 3}", (1, hh, ww))[0].cpu().numpy()
                assert rel_err(got, want) < (1e-5 if mode == "fp32" else 2e-2), (mode, l, b)
                hd = eb.buffer(f"head{l + 3}").cpu().numpy().reshape(B, hh, ww, 5)[b]
                hms.append(np.ascontiguousarray(hd[..., 4]))
                regs.append(np.ascontiguousarray(hd[..., :4]))
            want = odec.decode_nms(hms, regs, (8, 16, 32), 1e-5, 1000, 0.6, 256)
            boxes, scores, keep = eb.proposals(b)
            assert np.array_equal(keep.cpu().numpy(), want["keep"]) and len(want["keep"]) > 0
            assert np.array_equal(boxes.cpu().numpy(), want["boxes"]) and np.array_equal(scores.cpu().numpy(), want["scores"])
        eb.close()
        e1.close()
