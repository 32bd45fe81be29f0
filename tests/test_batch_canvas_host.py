"""Host side of the batch canvases ("batch canvas v1", include/ore_hip.h): orehip.batch_canvas_plan packs a step's raw images -- table
and slab -- into one buffer (pinned where there is a GPU to pin for).  No GPU needed."""
import numpy as np
import pytest
import torch


def _img(seed, h, w, dtype=torch.uint8):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 256, (3, h, w), generator=g, dtype=torch.uint8)
    return x if dtype == torch.uint8 else x.float() + 0.25


def _word_pair(row, at):
    return (int(row[at]) & 0xffffffff) | ((int(row[at + 1]) & 0xffffffff) << 32)


def test_plan_packs_images_into_one_buffer():
    import orehip
    sizes = [(33, 41), (64, 96), (50, 70)]
    imgs = [_img(i, h, w) for i, (h, w) in enumerate(sizes)]
    sups = [_img(10 + i, 40, 40, torch.float32)[None].repeat(2, 1, 1, 1) for i in range(3)]           # [N = 2, 3, 40, 40] per image
    plan = orehip.batch_canvas_plan(imgs, sups, div=32)
    g = plan.geom
    assert g.n_query == 3 and g.n_support == 6 and g.q_canvas == (64, 96) and g.s_canvas == (64, 64) and g.q_u8 and not g.s_u8
    assert plan.host.dtype == torch.uint8 and plan.host.dim() == 1 and plan.host.numel() == g.table_bytes + g.slab_bytes
    assert plan.host.is_pinned() == torch.cuda.is_available()
    assert g.table_bytes % 16 == 0 and g.table_bytes >= 9 * orehip.BATCH_CANVAS_JOB_INTS * 4 and g.slab_bytes % 16 == 0
    assert plan.used <= plan.host.numel()
    assert g.out_floats == 3 * 3 * 64 * 96 + 6 * 3 * 64 * 64
    t = plan.table.numpy()
    assert t.shape == (9, orehip.BATCH_CANVAS_JOB_INTS) and t.dtype == np.int32
    assert plan.table.data_ptr() == plan.host.data_ptr()                       # the rows ARE the head of the buffer
    slab = plan.host[g.table_bytes:]
    src, dst = 0, 0
    everything = imgs + [s[i] for s in sups for i in range(2)]
    for j, im in enumerate(everything):
        Hc, Wc = (64, 96) if j < 3 else (64, 64)
        h, w = int(im.shape[1]), int(im.shape[2])
        # row: byte offset in the slab (low, high), h, w, float offset in the output (low, high), canvas
        assert _word_pair(t[j], 0) == src and _word_pair(t[j], 4) == dst and tuple(t[j][[2, 3, 6, 7]]) == (h, w, Hc, Wc), (j, t[j])
        assert src % 16 == 0 and dst % 4 == 0
        nb = 3 * h * w * im.element_size()
        got = slab[src:src + nb]
        got = got if im.dtype == torch.uint8 else got.view(torch.float32)
        assert torch.equal(got.view(3, h, w), im)                                # planar, contiguous at its own size
        src += (nb + 15) // 16 * 16
        dst += 3 * Hc * Wc
    assert plan.used == g.table_bytes + src


def test_plan_capacity_fixed_canvas_and_full_slab():
    import orehip
    a, b = _img(1, 30, 50), _img(2, 60, 20)
    p1 = orehip.batch_canvas_plan([a, b], [], div=32, capacity=(4, 0), full_slab=True)
    p2 = orehip.batch_canvas_plan([b, a, a], [], div=32, capacity=(4, 0), full_slab=True)
    assert p1.geom == p2.geom and p1.geom.q_canvas == (64, 64) and p1.geom.n_query == 4       # the launch depends on the canvas alone
    assert p1.geom.slab_bytes == 4 * 3 * 64 * 64 and p1.used < p2.used <= p1.host.numel()
    t = p1.table.numpy()
    assert tuple(t[2][[2, 3]]) == (0, 0) and tuple(t[3][[2, 3]]) == (0, 0)                     # empty jobs: all-padding canvases
    assert _word_pair(t[3], 4) == 3 * 3 * 64 * 64
    p3 = orehip.batch_canvas_plan([a], [], q_canvas=(96, 128))
    assert p3.geom.q_canvas == (96, 128)


def test_plan_refusals():
    import orehip
    a, b = _img(1, 33, 41), _img(2, 64, 96)
    with pytest.raises(ValueError, match="larger than its"):
        orehip.batch_canvas_plan([a, b], [], q_canvas=(64, 64))
    with pytest.raises(ValueError, match="one dtype per group"):
        orehip.batch_canvas_plan([a, b.float()], [])
    with pytest.raises(ValueError, match="one dtype per group"):
        orehip.batch_canvas_plan([a], [_img(3, 40, 40), _img(4, 40, 40, torch.float32)])
    with pytest.raises(ValueError, match="capacity"):
        orehip.batch_canvas_plan([a, b], [], capacity=(1, 0))
    with pytest.raises(ValueError, match="capacity"):
        orehip.batch_canvas_plan([a], [_img(3, 40, 40)[None].repeat(3, 1, 1, 1)], capacity=(1, 2))
    with pytest.raises(ValueError, match="uint8 or fp32"):
        orehip.batch_canvas_plan([a.to(torch.int16)], [])
    with pytest.raises(ValueError, match=r"\[3, h, w\]"):
        orehip.batch_canvas_plan([a[:1]], [])
    # a query group of uint8 beside a support group of fp32 is no mix: the dtype is per group
    orehip.batch_canvas_plan([a, b], [_img(4, 40, 40, torch.float32)])


def test_symbol_and_layout_constants_match_the_header():
    import re
    import orehip
    assert "ore_batch_canvas_fwd" in orehip.SYMBOLS
    with open(orehip.HEADER) as f:
        src = f.read()
    defs = {m[1]: int(m[2]) for m in re.finditer(r"#define (ORE_BATCH_CANVAS_JOB_INTS|ORE_BCJ_\w+) (\d+)", src)}
    assert defs == {"ORE_BATCH_CANVAS_JOB_INTS": orehip.BATCH_CANVAS_JOB_INTS, "ORE_BCJ_SRC": orehip._BCJ_SRC, "ORE_BCJ_H": orehip._BCJ_H,
                    "ORE_BCJ_W": orehip._BCJ_W, "ORE_BCJ_DST": orehip._BCJ_DST, "ORE_BCJ_HC": orehip._BCJ_HC, "ORE_BCJ_WC": orehip._BCJ_WC}
