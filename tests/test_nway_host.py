"""CPU: the N-way inference contract (include/ore_hip.h, ore_engine_set_classes) without a GPU.

`merge_classes` below is the numpy restatement of the merge + detector_postprocess that k_roi_merge_classes runs; tests/test_hip_nway.py
holds the engine's record against it bit for bit.  Here it is pinned on hand-made cases, and CenterNet2Detector.support_classes'
resolution (None / "all" / a list of ids) is checked."""
import numpy as np
import pytest
import torch

from roitail_ref import scale_clip_drop


def merge_classes(dets, class_ids, topk, in_hw, out_hw):
    """dets: per class slot (boxes [n,4] f32, scores [n] f32), each list score-descending as the per-class second stage leaves it.
    Union ordered by score descending, ties by class slot, then by row within the class; the first `topk` rows; then
    detector_postprocess (d2z:modeling/postprocessing.py:10-75) in fp32: scale by (out_w / in_w, out_h / in_h) rounded once to fp32,
    clip to the output size, drop boxes with no area.  Returns (boxes [m,4] f32, scores [m] f32, classes [m] int64)."""
    boxes = [np.asarray(b, np.float32).reshape(-1, 4) for b, _ in dets]
    scores = [np.asarray(s, np.float32).reshape(-1) for _, s in dets]
    cls = [np.full(len(s), c, np.int64) for s, c in zip(scores, class_ids)]
    B, S, Cl = np.concatenate(boxes), np.concatenate(scores), np.concatenate(cls)
    order = np.argsort(-S, kind="stable")[:topk]         # concatenation index = (slot, row): the stable sort breaks ties by it
    B, S, Cl = B[order], S[order], Cl[order]
    (H, W), (oh, ow) = in_hw, out_hw
    sx, sy = np.float32(ow / W), np.float32(oh / H)
    B, keep = scale_clip_drop(B, sx, sy, ow, oh)          # the arithmetic k_roi_tail's postprocess is held to as well
    return B[keep], S[keep], Cl[keep]


def _box(x, y, w=10.0, h=10.0):
    return [x, y, x + w, y + h]


def test_merge_ties_across_classes_follow_the_slot_order():
    a = (np.array([_box(0, 0), _box(1, 1), _box(2, 2)]), np.array([0.9, 0.5, 0.5]))
    b = (np.array([_box(3, 3), _box(4, 4)]), np.array([0.9, 0.5]))
    boxes, scores, cls = merge_classes([a, b], [7, 3], 100, (100, 100), (100, 100))
    assert scores.tolist() == pytest.approx([0.9, 0.9, 0.5, 0.5, 0.5])
    assert cls.tolist() == [7, 3, 7, 7, 3]                 # slot 0 before slot 1 at equal score, rows in order within a slot
    assert boxes[:, 0].tolist() == [0, 3, 1, 2, 4]


def test_merge_cuts_the_union_at_topk():
    rng = np.random.default_rng(0)
    dets = []
    for k in range(3):
        s = np.sort(rng.random(60).astype(np.float32))[::-1]
        dets.append((np.array([_box(i, k) for i in range(60)], np.float32), s))
    boxes, scores, cls = merge_classes(dets, [0, 1, 2], 100, (200, 200), (200, 200))
    assert len(scores) == 100
    allscores = np.sort(np.concatenate([d[1] for d in dets]))[::-1]
    assert np.array_equal(scores, allscores[:100])
    assert np.all(np.diff(scores) <= 0)
    assert set(cls.tolist()) == {0, 1, 2}


def test_merge_drops_boxes_that_are_empty_after_scaling():
    a = (np.array([_box(10, 10), [50, 50, 50, 60], [95, 5, 120, 20]], np.float32), np.array([0.8, 0.7, 0.6], np.float32))
    b = (np.array([[-30, 10, -5, 20]], np.float32), np.array([0.75], np.float32))     # entirely left of the image: clipped to width 0
    boxes, scores, cls = merge_classes([a, b], [1, 2], 100, (100, 100), (50, 200))     # output 200 wide, 50 high
    assert scores.tolist() == pytest.approx([0.8, 0.6])
    assert cls.tolist() == [1, 1]
    np.testing.assert_array_equal(boxes[0], np.array([20, 5, 40, 10], np.float32))
    np.testing.assert_array_equal(boxes[1], np.array([190, 2.5, 200, 10], np.float32))


def test_merge_with_a_class_that_has_no_rows():
    empty = (np.zeros((0, 4), np.float32), np.zeros(0, np.float32))
    a = (np.array([_box(0, 0), _box(5, 5)], np.float32), np.array([0.4, 0.3], np.float32))
    boxes, scores, cls = merge_classes([empty, a, empty], [5, 6, 8], 100, (64, 64), (64, 64))
    assert cls.tolist() == [6, 6] and scores.tolist() == pytest.approx([0.4, 0.3])
    boxes, scores, cls = merge_classes([empty, empty], [5, 6], 100, (64, 64), (64, 64))
    assert len(boxes) == len(scores) == len(cls) == 0


def test_merge_of_one_class_is_detector_postprocess_of_its_rows():
    a = (np.array([_box(0, 0), _box(30, 40, 5, 7)], np.float32), np.array([0.4, 0.3], np.float32))
    boxes, scores, cls = merge_classes([a], [4], 100, (80, 80), (160, 120))
    np.testing.assert_array_equal(boxes, np.array([[0, 0, 15, 20], [45, 80, 52.5, 94]], np.float32))
    assert cls.tolist() == [4, 4]


# ---------------------------------------------------------------------------------------------- support_classes resolution
def _support(classes, rcnn=None):
    t = torch.zeros(1)
    d = {k: {c: t for c in classes} for k in ("p3", "p4", "p5")}
    d["rcnn_8"] = {c: t for c in (classes if rcnn is None else rcnn)}
    return d


def test_support_classes_resolution():
    from fewx.modeling.fsod.fsod_cen import resolve_support_classes
    sd = _support([3, 1, 2])
    assert resolve_support_classes(sd, None) is None
    assert resolve_support_classes(sd, "all") == [3, 1, 2]          # insertion order, as the reference's .items() loops
    assert resolve_support_classes(sd, [2, 3]) == [2, 3]            # the given order
    assert resolve_support_classes(sd, (1,)) == [1]
    with pytest.raises(ValueError, match="no p3"):
        resolve_support_classes(sd, [3, 9])
    with pytest.raises(ValueError, match="rcnn_8"):
        resolve_support_classes(_support([3, 1], rcnn=[3]), "all")
    with pytest.raises(ValueError, match="rcnn_8"):
        resolve_support_classes(_support([3, 1], rcnn=[3]), [1])
    for bad in ([], "every", [1, 1], list(range(17))):
        with pytest.raises(ValueError):
            resolve_support_classes(_support(list(range(20))), bad)


def test_support_classes_is_an_attribute_not_a_config_key():
    from fewx.config import get_cfg
    from fewx.modeling.fsod.fsod_cen import CenterNet2Detector
    import inspect
    src = inspect.getsource(CenterNet2Detector.__init__)
    assert "self.support_classes = None" in src
    assert "SUPPORT_CLASSES" not in str(get_cfg())
