"""GPU: N-way inference -- one query image against K support classes in one engine pass (include/ore_hip.h, ore_engine_set_classes;
CenterNet2Detector.support_classes).  Every class block is checked against a single-class engine built on that class alone, the merged
record bit for bit against the numpy restatement of tests/test_nway_host.py applied to the engine's own per-class detections."""
import os

import numpy as np
import pytest
import torch

from oracle import decode as odec
from oracle import ref_model as R
from test_nway_host import merge_classes

pytestmark = pytest.mark.gpu
HW = (320, 320)
SCORE, NMS, TOPK = 0.05, 0.9, 100


@pytest.fixture(scope="module")
def ore():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import orehip
    orehip.lib()
    return orehip


@pytest.fixture(scope="module")
def sd():
    return R.synth_state_dict(0)


@pytest.fixture(scope="module")
def roi_sd(sd):
    s = R.synth_roi_state(sd, 0)
    s["roi_heads.box_head.0.fc1.weight"] = s["roi_heads.box_head.0.fc1.weight"] * 0.01    # un-saturated logits / deltas
    return s


def supports(n):
    """n classes: prototypes of distinct seeds, rcnn_8 features of distinct seeds."""
    out = []
    for k in range(n):
        rc8 = torch.randn(6, 128, 8, 8, generator=torch.Generator().manual_seed(40 + k)) * 0.1
        out.append((R.synth_support(10 + k), rc8))
    return out


def single_engine(ore, sd, roi_sd, sup, hw=HW):
    e = ore.Engine(max_batch=1, max_h=hw[0], max_w=hw[1])
    e.load_state_dict(sd)
    e.set_support(sup[0])
    e.finalize()
    e.set_roi_head(roi_sd, sup[1], (10.0, 10.0, 5.0, 5.0), SCORE, NMS, TOPK)
    return e


def nway_engine(ore, sd, roi_sd, sups, ids, max_batch=None, hw=HW):
    e = ore.Engine(max_batch=max_batch or len(sups), max_h=hw[0], max_w=hw[1])
    e.load_state_dict(sd)
    e.finalize()
    e.set_roi_head(roi_sd, sups[0][1], (10.0, 10.0, 5.0, 5.0), SCORE, NMS, TOPK)
    e.set_classes(ids)
    for k, (p, rc8) in enumerate(sups):
        e.set_support(p, slot=k)
        e.set_roi_support(roi_sd, rc8, slot=k)
    return e


def per_class_dets(e, K):
    out = []
    for k in range(K):
        b, s, _ = e.detections(k)
        out.append((b.cpu().numpy(), s.cpu().numpy()))
    return out


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


@pytest.fixture(scope="module")
def three(ore, sd, roi_sd):
    """A 3-class N-way engine and the three single-class engines of the same classes, run on one image."""
    sups = supports(3)
    img = R.synth_image(7, *HW).cuda()
    en = nway_engine(ore, sd, roi_sd, sups, [11, 12, 13])
    en.eval_classes_forward(img, use_graph=False)
    torch.cuda.synchronize()
    singles = []
    for s in sups:
        e = single_engine(ore, sd, roi_sd, s)
        e.eval_forward(img, use_graph=False)
        torch.cuda.synchronize()
        singles.append(e)
    yield en, singles, sups, img
    en.close()
    for e in singles:
        e.close()


def test_fanout_correlation_bit_identical_per_class(three):
    en, singles, _, _ = three
    K = len(singles)
    for l in (3, 4, 5):
        h, w = HW[0] >> l, HW[1] >> l
        attn = en.buffer(f"attn{l}", (K, h, w))
        q = en.buffer(f"p{l}", (K, h, w))
        for k, e1 in enumerate(singles):
            assert torch.equal(attn[k], e1.buffer(f"attn{l}", (1, h, w))[0]), (l, k)
            assert torch.equal(q[k], q[0]), (l, k)
        assert torch.equal(q[0], singles[0].buffer(f"p{l}", (1, h, w))[0])


def test_per_class_first_stage(three):
    en, singles, _, _ = three
    K = len(singles)
    for k, e1 in enumerate(singles):
        hms, regs = [], []
        for l in range(3):
            h, w = HW[0] >> (l + 3), HW[1] >> (l + 3)
            for name in (f"pos{l + 3}", f"head{l + 3}"):
                got = en.buffer(name, (K, h, w))[k].cpu().numpy()
                want = e1.buffer(name, (1, h, w))[0].cpu().numpy()
                assert rel_err(got, want) < 1e-5, (name, k)
            hd = en.buffer(f"head{l + 3}").cpu().numpy().reshape(K, h, w, 5)[k]
            hms.append(np.ascontiguousarray(hd[..., 4]))
            regs.append(np.ascontiguousarray(hd[..., :4]))
        want = odec.decode_nms(hms, regs, (8, 16, 32), 1e-5, 1000, 0.6, 256)
        boxes, scores, keep = en.proposals(k)
        assert len(want["keep"]) > 0
        assert np.array_equal(keep.cpu().numpy(), want["keep"]) and np.array_equal(boxes.cpu().numpy(), want["boxes"])
        assert np.array_equal(scores.cpu().numpy(), want["scores"])


def test_per_class_second_stage(three):
    en, singles, _, _ = three
    for k, e1 in enumerate(singles):
        db, ds, _ = en.detections(k)
        d1, s1, _ = e1.detections(0)
        assert db.shape == d1.shape and db.shape[0] > 0, k
        assert float((db - d1).abs().max()) < 0.5 and float((ds - s1).abs().max()) < 1e-4, k


def _check_record(e, ids, got, in_hw, out_hw):
    want = merge_classes(per_class_dets(e, len(ids)), ids, TOPK, in_hw, out_hw)
    b, s, c = (t.cpu().numpy() for t in got)
    assert len(s) > 0
    assert np.array_equal(b, want[0]) and np.array_equal(s, want[1]) and np.array_equal(c, want[2])
    return c


def test_merge_record_bit_exact(three):
    en, singles, _, img = three
    ids = [11, 12, 13]
    cases = [(img, (320, 320)), (img.cpu(), (480, 800)), (img.float(), (200, 111)), (img.float().cpu(), (640, 640))]
    for image, out_hw in cases:
        got = en.detect_classes(image, *out_hw)
        c = _check_record(en, ids, got, HW, out_hw)
        assert set(c.tolist()) <= set(ids) and got[2].dtype == torch.int64 and got[0].is_cuda


def test_merge_tie_order_by_slot(ore, sd, roi_sd):
    """Two slots with identical supports give identical per-class lists: every score appears twice, slot 0's row first."""
    s = supports(1)[0]
    e = nway_engine(ore, sd, roi_sd, [s, s], [7, 3])
    img = R.synth_image(8, *HW).cuda()
    got = e.detect_classes(img, 320, 320)
    dets = per_class_dets(e, 2)
    assert np.array_equal(dets[0][0], dets[1][0]) and np.array_equal(dets[0][1], dets[1][1]) and len(dets[0][1]) > 0
    c = _check_record(e, [7, 3], got, HW, (320, 320))
    n = min(len(dets[0][1]), TOPK // 2)
    assert c[:2 * n].tolist() == [7, 3] * n
    e.close()


def _model(ore, sd, roi_sd):
    from conftest import PKG
    from fewx.config import get_cfg
    from detectron2.modeling import build_model
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(PKG, "configs", "fsod", "finetune_vovnet.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", "cuda", "INPUT.MAX_SIZE_TEST", HW[0]])
    cfg.freeze()
    m = build_model(cfg)
    m.load_state_dict(roi_sd, strict=False)
    return m.eval()


def _support_dict(sups, ids):
    d = {k: {} for k in ("p3", "p4", "p5", "rcnn_8", "rcnn_4")}
    for (p, rc8), c in zip(sups, ids):
        for k in ("p3", "p4", "p5"):
            d[k][c] = p[k]
        d["rcnn_8"][c] = rc8
        d["rcnn_4"][c] = torch.zeros(6, 128, 4, 4)
    return d


@pytest.fixture(scope="module")
def model(ore, sd, roi_sd):
    return _model(ore, sd, roi_sd)


def _run(m, img, oh=320, ow=320):
    inst = m([{"image": img, "height": oh, "width": ow}])[0]["instances"]
    return inst.pred_boxes.tensor.clone(), inst.scores.clone(), inst.pred_classes.clone()


def test_k1_non_last_class_equals_a_model_of_that_class(model):
    sups = supports(3)
    img = R.synth_image(9, *HW)
    model.support_classes = None
    model.set_support_dict(_support_dict(sups[1:2], [21]))
    want = _run(model, img, 400, 360)
    model.set_support_dict(_support_dict(sups, [20, 21, 22]))
    model.support_classes = [21]
    got = _run(model, img, 400, 360)
    model.support_classes = None
    assert len(want[1]) > 0
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert got[2].tolist() == [21] * len(got[2])


def test_default_path_unchanged(model):
    sups = supports(3)
    img = R.synth_image(10, *HW)
    model.support_classes = None
    model.set_support_dict(_support_dict(sups[2:3], [0]))                 # today's result: the last class alone
    want = _run(model, img)
    model.set_support_dict(_support_dict(sups, [5, 6, 0]))
    got = _run(model, img)
    assert not hasattr(model._engine, "class_ids") or not model._engine.class_ids
    assert len(want[1]) > 0 and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert got[2].tolist() == [0] * len(got[2])


def test_graph_and_eager_and_switching_selection(ore, sd, roi_sd, model):
    sups = supports(3)
    img = R.synth_image(11, *HW).cuda()
    e = nway_engine(ore, sd, roi_sd, sups, [1, 2, 3])
    e.eval_classes_forward(img, use_graph=False)
    torch.cuda.synchronize()
    eager = [t.clone() for k in range(3) for t in e.detections(k)]
    e.eval_classes_forward(img, use_graph=True)
    torch.cuda.synchronize()
    graph = [t.clone() for k in range(3) for t in e.detections(k)]
    assert all(torch.equal(a, b) for a, b in zip(eager, graph))
    r3 = [t.clone() for t in e.detect_classes(img, 320, 320)]
    e.set_classes([1, 2])                                              # slots 0, 1 keep their supports
    r2 = [t.clone() for t in e.detect_classes(img, 320, 320)]
    e.set_classes([1, 2, 3])
    r3b = [t.clone() for t in e.detect_classes(img, 320, 320)]
    assert all(torch.equal(a, b) for a, b in zip(r3, r3b))
    f2 = nway_engine(ore, sd, roi_sd, sups[:2], [1, 2])
    want2 = f2.detect_classes(img, 320, 320)
    assert all(torch.equal(a, b) for a, b in zip(r2, want2))
    f2.close()
    e.close()
    # the same through the module attribute: the engine cache follows the selection
    model.set_support_dict(_support_dict(sups, [1, 2, 3]))
    outs = []
    for sel in ("all", [1, 2], [1, 2, 3]):
        model.support_classes = sel
        outs.append(_run(model, img.cpu()))
    model.support_classes = None
    assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[2]))
    for out, sel in ((outs[1], [1, 2]), (outs[2], [1, 2, 3])):
        fresh = model.make_engine(classes=sel)
        want = fresh.detect_classes(img, 320, 320)
        assert len(want[1]) > 0 and all(torch.equal(a, b) for a, b in zip(out, want)), sel
        fresh.close()
    assert set(outs[0][2].tolist()) <= {1, 2, 3}


def test_refusals(ore, sd, roi_sd):
    prev = ore.set_conv_precision("bf16s")
    try:
        eb = ore.Engine(max_batch=1, max_h=HW[0], max_w=HW[1])
    finally:
        ore.set_conv_precision(prev)
    with pytest.raises(ore.OreError, match="bf16-storage"):
        eb.set_classes([0])
    eb.close()
    sups = supports(3)
    e = ore.Engine(max_batch=2, max_h=HW[0], max_w=HW[1])
    e.load_state_dict(sd)
    e.finalize()
    e.set_roi_head(roi_sd, sups[0][1], (10.0, 10.0, 5.0, 5.0), SCORE, NMS, TOPK)
    with pytest.raises(ore.OreError, match="max_batch"):
        e.set_classes([0, 1, 2])
    e.set_classes([0, 1])
    e.set_support(sups[0][0], slot=0)
    e.set_roi_support(roi_sd, sups[0][1], slot=0)
    img = R.synth_image(12, *HW).cuda()
    with pytest.raises(ore.OreError, match="slot 1"):
        e.detect_classes(img, 320, 320)
    e.set_support(sups[1][0], slot=1)
    with pytest.raises(ore.OreError, match="slot 1"):
        e.detect_classes(img, 320, 320)
    e.set_roi_support(roi_sd, sups[1][1], slot=1)
    b, s, c = e.detect_classes(img, 320, 320)                          # complete now, and nothing was left pending by the refusals
    assert len(s) > 0 and set(c.tolist()) <= {0, 1}
    e.close()
