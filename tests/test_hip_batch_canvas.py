"""ore_batch_canvas_fwd on the GPU: the query and the support canvas of a training step from one launch, bit for bit the tensors the
mixed-size branch of train_forward.train_core composes from torch ops (`_normalise_pad`, then the two pads) -- that composition is the
definition, copied here as `_compose`."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DIV = 32
NORMS = {"unit_std": ([103.530, 116.280, 123.675], [1.0, 1.0, 1.0]),                      # the config's PIXEL_MEAN / PIXEL_STD
         "real_std": ([103.530, 116.280, 123.675], [57.375, 57.120, 58.395])}             # a division that has to round


@pytest.fixture(scope="module")
def oh():
    import orehip
    orehip.lib()
    return orehip


def _img(seed, h, w, dtype=torch.uint8):
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.uint8:
        return torch.randint(0, 256, (3, h, w), generator=g, dtype=torch.uint8)
    return torch.rand(3, h, w, generator=g) * 255.0                                        # raw fp32: any value, not only whole numbers


def _norm(name):
    mean, std = NORMS[name]
    return torch.tensor(mean).view(3, 1, 1).cuda(), torch.tensor(std).view(3, 1, 1).cuda()


def _compose(imgs, sups, mean, std):
    """train_core's mixed-size branch, on device tensors."""
    from fewx.modeling.fsod.train_forward import _normalise_pad
    mean, std = mean.view(-1), std.view(-1)
    imgs = [i.float() for i in imgs]
    Hm, Wm = max(i.shape[-2] for i in imgs), max(i.shape[-1] for i in imgs)
    xq = torch.cat([F.pad(_normalise_pad(i[None], mean, std, 1), (0, Wm - i.shape[-1], 0, Hm - i.shape[-2])) for i in imgs], 0)
    xq = F.pad(xq, (0, (Wm + DIV - 1) // DIV * DIV - Wm, 0, (Hm + DIV - 1) // DIV * DIV - Hm)).contiguous()
    xs = _normalise_pad(torch.cat(sups, 0) if len(sups) > 1 else sups[0], mean, std, DIV) if sups else None
    return xq, xs


def _padding_is_plus_zero(canvas, sizes):
    for b, (h, w) in enumerate(sizes):
        pad = torch.ones(canvas.shape[-2:], dtype=torch.bool, device=canvas.device)
        pad[:h, :w] = False
        cells = canvas[b][:, pad]
        assert not bool(torch.signbit(cells).any()) and bool((cells == 0).all()), (b, h, w)


def _check(oh, imgs, sups, norm):
    mean, std = _norm(norm)
    plan = oh.batch_canvas_plan(imgs, sups, div=DIV)
    buf = plan.host[:plan.used].cuda()
    buf = torch.cat([buf, torch.zeros(plan.host.numel() - plan.used, dtype=torch.uint8, device="cuda")])
    xq, xs = oh.batch_canvas(buf, plan.geom, mean, std)
    rq, rs = _compose([i.cuda() for i in imgs], [s.cuda() for s in sups], mean, std)
    torch.cuda.synchronize()
    assert xq.shape == rq.shape and xq.dtype == torch.float32 and torch.equal(xq, rq), float((xq - rq).abs().max())
    _padding_is_plus_zero(xq, [tuple(i.shape[1:]) for i in imgs])
    if sups:
        assert xs.shape == rs.shape and torch.equal(xs, rs), float((xs - rs).abs().max())
        _padding_is_plus_zero(xs, [tuple(s.shape[2:]) for s in sups for _ in range(s.shape[0])])
    else:
        assert xs.numel() == 0


SIZES = [(33, 41), (64, 96), (50, 70)]                       # widths that are no multiple of 4: unaligned uint8 rows; one fills the canvas


@pytest.mark.parametrize("norm", sorted(NORMS))
@pytest.mark.parametrize("qdt,sdt", [(torch.uint8, torch.float32), (torch.float32, torch.uint8), (torch.uint8, torch.uint8)])
def test_three_images_and_their_supports(oh, norm, qdt, sdt):
    """Three query images of different sizes and a support group of [B*N, 3, 40, 40] (N = 2), both groups in one launch."""
    imgs = [_img(i, h, w, qdt) for i, (h, w) in enumerate(SIZES)]
    sups = [torch.stack([_img(10 + 2 * i + k, 40, 40, sdt) for k in range(2)]) for i in range(3)]
    _check(oh, imgs, sups, norm)


@pytest.mark.parametrize("dt", [torch.uint8, torch.float32])
@pytest.mark.parametrize("sizes", [[(64, 96)], [(1, 1)], [(1, 1), (31, 33), (32, 37)], [(7, 3)], [(1000, 1399)]],
                         ids=["fills_canvas_B1", "one_pixel_B1", "one_pixel_in_batch", "narrower_than_a_quad", "capped_grid"])
def test_edge_sizes(oh, dt, sizes):
    """An image that fills its canvas (no padding), a 1 x 1 image, B = 1, an image narrower than one 16-byte store, and a canvas with
    more quads than the capped grid has threads (the kernel's loop takes a second trip)."""
    _check(oh, [_img(20 + i, h, w, dt) for i, (h, w) in enumerate(sizes)], [], "real_std")
    if sizes == [(64, 96)]:
        _check(oh, [_img(30, 64, 96, dt)], [_img(31, 40, 40, dt)[None]], "real_std")


def test_captured_launch_serves_later_sizes(oh):
    """The launch captured ONCE over a fixed slab and table; the sizes are read on the device, so after one copy into the buffer the
    replay builds the canvases of another set of sizes with the same canvas."""
    mean, std = _norm("real_std")
    sets = [[(33, 41), (64, 96), (50, 70)], [(64, 96), (10, 13), (61, 95)], [(5, 90), (64, 2), (64, 96)]]
    batches = [([_img(40 + 10 * k + i, h, w) for i, (h, w) in enumerate(s)],
                [torch.stack([_img(70 + 10 * k + 2 * i + j, 40 - 3 * k, 40 - 5 * k, torch.float32) for j in range(2)]) for i in range(3)])
               for k, s in enumerate(sets)]
    plans = [oh.batch_canvas_plan(q, s, div=DIV, s_canvas=(64, 64), full_slab=True) for q, s in batches]
    geom = plans[0].geom
    assert all(p.geom == geom for p in plans)
    buf = torch.zeros(geom.table_bytes + geom.slab_bytes, dtype=torch.uint8, device="cuda")
    out = torch.empty(geom.out_floats, device="cuda")
    buf[:plans[0].used].copy_(plans[0].host[:plans[0].used])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        oh.batch_canvas(buf, geom, mean, std, out=out)                                   # (everything lazy happens before the capture)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        xq, xs = oh.batch_canvas(buf, geom, mean, std, out=out)
    for k in (1, 2, 0):
        out.fill_(float("nan"))
        buf[:plans[k].used].copy_(plans[k].host[:plans[k].used], non_blocking=True)
        g.replay()
        q, s = batches[k]
        rq, rs = _compose([i.cuda() for i in q], [t.cuda() for t in s], mean, std)
        rs = F.pad(rs, (0, 64 - rs.shape[-1], 0, 64 - rs.shape[-2]))                      # (the fixed support canvas of the capture)
        torch.cuda.synchronize()
        assert torch.equal(xq, rq) and torch.equal(xs, rs), k
        _padding_is_plus_zero(xq, sets[k])
