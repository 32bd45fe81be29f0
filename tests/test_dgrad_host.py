"""CPU: the float64 data-gradient reference of tests/dgrad_ref.py is the conv input gradient, and its two bounds have teeth.

tests/test_hip_dgrad.py holds every data-gradient launch form of ore_conv2d_fwd to a float64 reference with an element-wise bound
2 d u (A + E) and a 16 x 16 block rms bound C_S u sqrt(d) (tests/dgrad_ref.py derives both).  Here, without a GPU: the reference is
float64 autograd of F.conv2d; a correct fp32 implementation (a k-ordered fma chain, split into S slabs; an fp32 Winograd F(2x2,3x3))
passes both bounds with headroom from the smallest to the largest production K class; and each fault the bounds are there to catch
fails at least one of them: unflipped taps, a dropped 16-channel K chunk in one output block at the largest K, a dropped split-K
slab, a 1e-3 error in one block of the smallest-scale channel, live values in dZ's padded channels, a halo row read from the
neighbouring image, and Winograd weights transformed from the unflipped layout."""
import math

import pytest
import torch

import dgrad_ref as DR

# production K classes (k * k * Cout16 of the layer): the 16-channel dZ of the class / box linears, the 128-channel linears and
# laterals, the stage-5 concat (720 -> 512: K = 512), and the 3x3 layers at 112 and 128 channels (the largest, 1152)
K_CLASSES = [(2, 64, 1), (128, 64, 1), (512, 48, 1), (112, 32, 3), (128, 32, 3)]      # (Cout, Cin, k)


def _fma_chain(dz, w, S=1, drop_slab=None, drop_chunk=None):
    """fp32 dX of the data-gradient conv as the launch computes it: K in (tap, channel) order, one fma (one rounding) per product,
    S split slabs of ceil(K / S) products added in order.  drop_slab: a slab left out; drop_chunk: (row block, chunk) -- that K
    chunk of 16 channels is left out of those 16 output rows."""
    B, H, W, cl = dz.shape
    co, ci, k, _ = w.shape
    p = k // 2
    wd = torch.zeros(cl, ci, k, k)
    wd[:co] = w
    zp = torch.nn.functional.pad(dz, (0, 0, p, p, p, p))
    a = torch.cat([zp[:, ky:ky + H, kx:kx + W, :].reshape(-1, cl) for ky in range(k) for kx in range(k)], 1).double()   # [M, K]
    b = torch.cat([wd[:, :, k - 1 - ky, k - 1 - kx] for ky in range(k) for kx in range(k)], 0).double()                  # [K, Cin]
    M, K = a.shape
    if drop_chunk is not None:
        blk, ch = drop_chunk
        a[blk * 16:(blk + 1) * 16, ch * 16:(ch + 1) * 16] = 0
    per = -(-K // S)
    out = torch.zeros(M, ci)
    for s in range(S):
        acc = torch.zeros(M, ci)
        for kk in range(s * per, min(K, (s + 1) * per)):
            acc = (acc.double() + a[:, kk:kk + 1] * b[kk:kk + 1]).float()
        if s != drop_slab:
            out = (out.double() + acc.double()).float()
    return out


def _ref(dz, w, **kw):
    return DR.dgrad_ref(dz, w, **kw)


def _wino32(dz, w, flip=True):
    g = torch.zeros(dz.shape[-1], w.shape[1], 3, 3)
    g[:w.shape[0]] = w.flip(2, 3) if flip else w
    return DR.winograd(dz, g, dtype=torch.float32).reshape(-1, w.shape[1])


def test_reference_is_the_conv_input_gradient():
    g = torch.Generator().manual_seed(1)
    for k, co in ((3, 20), (1, 5)):
        x = torch.randn(3, 7, 5, 24, dtype=torch.float64, generator=g, requires_grad=True)
        w = torch.randn(co, 24, k, k, dtype=torch.float64, generator=g)
        y = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2), w, padding=k // 2)
        dy = torch.randn(y.shape, dtype=torch.float64, generator=g)
        (y * dy).sum().backward()
        dz = torch.zeros(3, 7, 5, DR.c16(co), dtype=torch.float64)
        dz[..., :co] = dy.permute(0, 2, 3, 1)
        ref, mag = DR.dgrad_ref(dz, w)
        assert torch.allclose(ref, x.grad.reshape(-1, 24), rtol=1e-12, atol=1e-12)
        assert bool((mag >= ref.abs() - 1e-12).all())
        if k == 3:                                            # the Winograd algorithm in float64 is the same gradient
            assert torch.allclose(DR.winograd(dz, _g(dz, w)).reshape(-1, 24), ref, rtol=1e-10, atol=1e-10)
            assert bool((DR.dgrad_wino_mag(dz, w) >= ref.abs() - 1e-10).all())


def _g(dz, w):
    g = torch.zeros(dz.shape[-1], w.shape[1], 3, 3, dtype=torch.float64)
    g[:w.shape[0]] = w.double().flip(2, 3)
    return g


def test_forward_form_reference():
    """scale / shift / ReLU epilogue and the nearest-2x upsampled add of the forward form (used by the production replay)."""
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 5, 7, 16, dtype=torch.float64, generator=g)
    w = torch.randn(16, 16, 3, 3, dtype=torch.float64, generator=g)     # forward conv x -> 16 channels, as OIHW of a layer 16 -> 16
    sc, sh = torch.rand(16, dtype=torch.float64, generator=g) + 0.5, torch.randn(16, dtype=torch.float64, generator=g)
    add = torch.randn(2, 3, 4, 16, dtype=torch.float64, generator=g)
    # forward form = a "data-gradient" call of the transposed, flipped weights
    wt = w.transpose(0, 1).flip(2, 3)
    ref, mag = DR.dgrad_ref(x, wt, scale=sc, shift=sh, add=add, relu=16)
    y = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2), w, padding=1).permute(0, 2, 3, 1) * sc + sh
    y = (y + add.repeat_interleave(2, 1).repeat_interleave(2, 2)[:, :5, :7]).clamp(min=0)
    assert torch.allclose(ref, y.reshape(-1, 16), rtol=1e-12, atol=1e-12)


def test_pack_layout_restatement():
    w = torch.arange(5 * 20 * 9, dtype=torch.float32).reshape(5, 20, 3, 3) + 1
    p = DR.pack_dgrad(w).reshape(32, 9, 16)
    for ci in (0, 7, 19):
        for tap in range(9):
            for co in range(5):
                assert p[ci, tap, co] == w[co, ci, 2 - tap // 3, 2 - tap % 3]
    assert float(p[20:].abs().max()) == 0 and float(p[:, :, 5:].abs().max()) == 0


@pytest.mark.parametrize("Cout,Cin,k", K_CLASSES)
def test_fp32_fma_chain_passes_with_headroom(Cout, Cin, k):
    dz, w = DR.scaled_operands(2, 5, 7, Cout, Cin, k, seed=Cout + k)
    ref, mag = _ref(dz, w)
    K = k * k * dz.shape[-1]
    for S in (1, 3):
        r = DR.dgrad_check(_fma_chain(dz, w, S), ref, mag, DR.depth(K, S))
        assert r["hard"] < 0.1 and r["rms"] < 0.2, (S, r)


@pytest.mark.parametrize("Cout", [64, 80, 112, 128])
def test_fp32_winograd_emulation_passes_with_headroom(Cout):
    dz, w = DR.scaled_operands(2, 9, 7, Cout, 32, 3, seed=Cout)
    ref, _ = _ref(dz, w)
    r = DR.dgrad_check(_wino32(dz, w), ref, DR.dgrad_wino_mag(dz, w), DR.depth(0, wino_cin=Cout))
    assert r["hard"] < 0.1 and r["rms"] < 0.2, r


def test_bf16_operands_pass_against_the_bf16_reference_only():
    dz, w = DR.scaled_operands(1, 6, 6, 128, 32, 3, seed=4)
    got = _fma_chain(DR.bf16_rne(dz), DR.bf16_rne(w))
    d = DR.depth(9 * 128)
    ref, mag = _ref(dz, w, bf16=True)
    r = DR.dgrad_check(got, ref, mag, d)
    assert r["hard"] < 0.1 and r["rms"] < 0.2, r
    ref, mag = _ref(dz, w)
    assert DR.dgrad_check(got, ref, mag, d)["hard"] > 1


# ---- teeth ---------------------------------------------------------------------------------------------------------------------
def test_unflipped_taps_fail():
    dz, w = DR.scaled_operands(2, 6, 6, 64, 32, 3, seed=5)
    ref, mag = _ref(dz, w)
    r = DR.dgrad_check(_fma_chain(dz, w.flip(2, 3)), ref, mag, DR.depth(9 * 64))
    assert r["hard"] > 1 and r["rms"] > 1, r


def test_dropped_k_chunk_in_one_block_fails_at_the_largest_k():
    """K = 9 x 128 = 1152: 2 d u = 1.4e-4 of A, the hard bound alone cannot see one missing 16-channel chunk; the block rms does."""
    dz, w = DR.scaled_operands(1, 8, 8, 128, 32, 3, seed=6)
    ref, mag = _ref(dz, w)
    d = DR.depth(9 * 128)
    ok = DR.dgrad_check(_fma_chain(dz, w), ref, mag, d)
    assert ok["hard"] <= 1 and ok["rms"] <= 1
    # the chunk of the centre tap that holds the largest-scale dZ channel, left out of output rows 16..31
    ch = 4 * 8 + int(dz.abs().amax((0, 1, 2)).argmax()) // 16
    r = DR.dgrad_check(_fma_chain(dz, w, drop_chunk=(1, ch)), ref, mag, d)
    assert r["rms"] > 1, r


@pytest.mark.parametrize("drop", [0, 2])
def test_dropped_split_slab_fails(drop):
    dz, w = DR.scaled_operands(1, 6, 6, 128, 32, 1, seed=7)
    ref, mag = _ref(dz, w)
    r = DR.dgrad_check(_fma_chain(dz, w, S=3, drop_slab=drop), ref, mag, DR.depth(128, 3))
    assert r["hard"] > 1 and r["rms"] > 1, r


def test_small_channel_block_error_fails_where_max_norm_passes():
    """dX rows 16..31 of the smallest-scale output channel, 1e-3 relative off."""
    dz, w = DR.scaled_operands(1, 8, 8, 112, 48, 3, seed=8)
    ref, mag = _ref(dz, w)
    got = _fma_chain(dz, w)
    c = int(w.abs().amax((0, 2, 3)).argmin())
    bad = got.clone()
    bad[16:32, c] *= 1.0 + 1e-3
    assert float((bad.double() - ref).abs().max() / ref.abs().max()) < 2e-5        # invisible to the suite's max-norm measure
    d = DR.depth(9 * 112)
    r = DR.dgrad_check(bad, ref, mag, d)
    assert r["rms"] > 1, r


def test_live_padded_dz_channels_fail():
    """Cout 5 -> a 16-channel dZ: values in channels 5..15 read against weights that are not zero there."""
    dz, w = DR.scaled_operands(2, 6, 6, 5, 32, 3, seed=9)
    ref, mag = _ref(dz, w)
    g = torch.Generator().manual_seed(1)
    dzb = dz.clone()
    dzb[..., 5:] = torch.randn(dzb[..., 5:].shape, generator=g) * dz[..., :5].abs().max()
    wb = torch.cat([w, torch.randn(11, 32, 3, 3, generator=g) * w.abs().max()], 0)
    r = DR.dgrad_check(_fma_chain(dzb, wb), ref, mag, DR.depth(9 * 16))
    assert r["hard"] > 1, r


def test_halo_from_the_neighbouring_image_fails():
    """B = 2: the images stacked as one tall image, so the 3x3 taps at the seam read the other image's rows instead of zeros."""
    dz, w = DR.scaled_operands(2, 5, 6, 64, 32, 3, seed=10)
    ref, mag = _ref(dz, w)
    tall = dz.reshape(1, 10, 6, dz.shape[-1])
    r = DR.dgrad_check(_fma_chain(tall, w), ref, mag, DR.depth(9 * 64))
    assert r["hard"] > 1, r


def test_winograd_from_unflipped_weights_fails():
    dz, w = DR.scaled_operands(1, 8, 8, 128, 32, 3, seed=11)
    ref, _ = _ref(dz, w)
    r = DR.dgrad_check(_wino32(dz, w, flip=False), ref, DR.dgrad_wino_mag(dz, w), DR.depth(0, wino_cin=128))
    assert r["hard"] > 1, r


def test_check_requires_exact_zeros():
    ref = torch.zeros(16, 16, dtype=torch.float64)
    got = torch.zeros(16, 16)
    got[3, 4] = 1e-30
    assert DR.dgrad_check(got, ref, torch.zeros_like(ref), 10)["hard"] == math.inf
    assert DR.dgrad_check(torch.zeros(16, 16), ref, torch.zeros_like(ref), 10) == {"hard": 0.0, "rms": 0.0}


def test_shape_matrix_covers_every_trained_layer():
    """Every trained conv / linear weight of configs/fsod/finetune_vovnet.yaml is a class of the GPU shape matrix (dgrad_ref.LAYERS)
    or is listed, with its reason, in dgrad_ref.NOT_DGRAD; both lists name only layers the model has."""
    import os
    from conftest import PKG
    from detectron2.modeling import build_model
    from fewx.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(PKG, "configs", "fsod", "finetune_vovnet.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", "cpu"])
    cfg.freeze()
    m = build_model(cfg)
    trained = {(p.shape[0], p.shape[1], p.shape[2] if p.dim() == 4 else 1) for p in m.parameters() if p.requires_grad and p.dim() in (2, 4)}
    listed = set(DR.LAYERS) | set(DR.NOT_DGRAD)
    merged = {(5, 128, 3)}                                  # the head prediction: agn_hm (1) + bbox_pred (4) in one launch
    assert trained - listed == set(), sorted(trained - listed)
    assert listed - merged <= trained, sorted(listed - merged - trained)
    assert not set(DR.LAYERS) & set(DR.NOT_DGRAD)
    assert len(DR.matrix()) == 2 * sum(len(v) for v in DR.LAYERS.values())
