"""CPU: proposal recall ("box_proposals": AR@100 .. ARl@1000).  The restatement of its contract (tests/proposal_recall_ref.py) against
what the reference's own function returned for the recorded set (tests/golden/box_proposals_ref.npz) and on hand-computed cases, one
per rule; the evaluator's host side with the device call replaced by the restatement; the model's switch.  The device code itself is
pinned to the restatement in tests/test_hip_proposal_recall.py."""
import os
import pickle

import numpy as np
import pytest
import torch

import proposal_recall_ref as R
from conftest import GOLDEN
from test_coco_eval_host import _gt, _instances, _register

f32 = np.float32


@pytest.fixture(scope="module")
def recorded():
    gt, entries, z = R.load_fixture(os.path.join(GOLDEN, "box_proposals_ref.npz"))
    return gt, entries, z, R.evaluate_all(gt, entries)


# ------------------------------------------------------------------ the reference's recorded results

@pytest.mark.parametrize("n", range(8))
def test_restatement_reproduces_the_reference_bytes(recorded, n):
    _, _, z, res = recorded
    key = R.KEYS[n]
    r = res[key]
    assert r["num_pos"] == int(z["num_pos"][n]) and r["num_pos"] > 0, key
    assert r["gt_overlaps"].dtype == np.float32 and r["gt_overlaps"].tobytes() == z[f"gt_overlaps_{n}"].tobytes(), key
    assert r["recalls"].tobytes() == z["recalls"][n].tobytes() and r["ar"].tobytes() == z["ar"][n].tobytes(), key
    assert np.array_equal(R.thresholds().numpy(), z["thresholds"])


def test_recorded_set_covers_the_cases(recorded):
    gt, entries, z, res = recorded
    crowd = {a["image_id"] for a in gt["annotations"] if a["iscrowd"]}
    noncrowd = {a["image_id"]: 0 for a in gt["annotations"] if not a["iscrowd"]}
    for a in gt["annotations"]:
        if not a["iscrowd"]:
            noncrowd[a["image_id"]] += 1
    counts = {im: len(s) for im, _, s in entries}
    assert crowd and any(counts[im] == 0 and noncrowd.get(im) for im in counts)              # GTs, no proposal
    assert any(counts[im] > 0 and not noncrowd.get(im) for im in counts)                      # proposals, no non-crowd GT
    assert any(0 < counts[im] < noncrowd.get(im, 0) for im in counts)                         # G > P
    assert any(100 < counts[im] <= 1000 for im in counts) and any(counts[im] > 1000 for im in counts)
    assert all(len(np.unique(s)) == len(s) for _, _, s in entries)                            # distinct logits within an image
    assert any(len(np.unique(r["gt_overlaps"][r["gt_overlaps"] > 0])) < (r["gt_overlaps"] > 0).sum() for r in res.values())   # IoU ties
    assert res["AR@100"]["ar"] != res["AR@1000"]["ar"]                                        # the limit decides something
    assert os.path.getsize(os.path.join(GOLDEN, "box_proposals_ref.npz")) < 100 * 1024


# ------------------------------------------------------------------ hand-computed cases, one per rule

def _a(im, box, **kw):
    return dict({"image_id": im, "category_id": 1, "bbox": box}, **kw)


def _e(im, boxes, logits):
    return (im, np.array(boxes, dtype=np.float32).reshape(-1, 4), np.array(logits, dtype=np.float32))


def test_tied_logits_keep_input_order():
    gt = _gt([1], [_a(1, [0, 0, 10, 10])])
    quarter, full = [0, 0, 5, 5], [0, 0, 10, 10]
    r = R.evaluate(gt, [_e(1, [quarter, full], [0.5, 0.5])], limit=1)
    assert r["per_entry"][0].tolist() == [0.25]                  # the first of the tied pair survives the cut
    r = R.evaluate(gt, [_e(1, [full, quarter], [0.5, 0.5])], limit=1)
    assert r["per_entry"][0].tolist() == [1.0]
    r = R.evaluate(gt, [_e(1, [quarter, full], [0.5, 0.75])], limit=1)
    assert r["per_entry"][0].tolist() == [1.0]                   # descending otherwise


def test_iou_tie_goes_to_the_lower_gt_index():
    # p0 covers g0 and g1 equally (50 / 150); p1 covers only g1 (20 / 100).  g0 takes p0, then g1 still has p1.  Had g1 taken p0, g0
    # would be left with nothing.
    gt = _gt([1], [_a(1, [0, 0, 10, 10]), _a(1, [10, 0, 10, 10])])
    r = R.evaluate(gt, [_e(1, [[5, 0, 15, 10], [18, 0, 20, 10]], [2, 1])])
    assert r["per_entry"][0].tolist() == [f32(50) / f32(150), f32(20) / f32(100)]
    assert r["gt_overlaps"].tolist() == [f32(20) / f32(100), f32(50) / f32(150)] and r["num_pos"] == 2


def test_iou_tie_then_goes_to_the_lower_proposal_index():
    # p0 and p1 each cover half of g0 (0.5); only p0 touches g1 (10 / 250).  g0 takes p0 (lower index), so g1 is left with 0.
    gt = _gt([1], [_a(1, [0, 20, 10, 10]), _a(1, [0, 0, 10, 21])])
    r = R.evaluate(gt, [_e(1, [[0, 20, 10, 25], [0, 25, 10, 30]], [2, 1])])
    assert r["per_entry"][0].tolist() == [0.5, 0.0]
    # the proposal index is the one after the sort by logit: with p1 ahead, g0 takes it and p0 is left for g1
    r = R.evaluate(gt, [_e(1, [[0, 20, 10, 25], [0, 25, 10, 30]], [1, 2])])
    assert r["per_entry"][0].tolist() == [0.5, f32(10) / f32(250)]


def test_trailing_zeros_when_more_gts_than_proposals():
    gt = _gt([1], [_a(1, [0, 0, 10, 10]), _a(1, [50, 50, 10, 10]), _a(1, [100, 100, 10, 10])])
    r = R.evaluate(gt, [_e(1, [[50, 50, 60, 55]], [0.0])])
    assert r["per_entry"][0].tolist() == [0.5, 0.0, 0.0] and r["num_pos"] == 3
    assert r["gt_overlaps"].tolist() == [0.0, 0.0, 0.5] and r["counts"].tolist() == [1] + [0] * 9
    assert r["recalls"].tolist() == [float(f32(1) / f32(3))] + [0.0] * 9


def test_limit_cuts_the_sorted_proposals():
    gt = _gt([1], [_a(1, [0, 0, 10, 10])])
    e = _e(1, [[0, 0, 5, 5], [0, 0, 10, 5], [0, 0, 10, 10]], [3, 2, 1])
    assert [R.evaluate(gt, [e], limit=k)["per_entry"][0].tolist() for k in (1, 2, 3, None)] == [[0.25], [0.5], [1.0], [1.0]]


def test_area_bounds_are_inclusive():
    gt = _gt([1], [_a(1, [0, 0, 32, 32]), _a(1, [100, 100, 96, 96])])
    assert [a["area"] for a in gt["annotations"]] == [32 ** 2, 96 ** 2]
    e = _e(1, [[0, 0, 32, 32]], [0.0])
    got = {a: R.evaluate(gt, [e], area=a) for a in R.AREA_LBL}
    assert {a: r["num_pos"] for a, r in got.items()} == {"all": 2, "small": 1, "medium": 2, "large": 1}
    assert got["small"]["per_entry"][0].tolist() == [1.0] and got["large"]["per_entry"][0].tolist() == [0.0]
    # the stated area decides, not the box; just past a bound it leaves the range
    gt["annotations"][0]["area"] = float(np.nextafter(f32(1024), f32(2000)))
    assert R.evaluate(gt, [e], area="small")["num_pos"] == 0 and R.evaluate(gt, [e], area="small")["per_entry"] == [None]


def test_crowd_only_image_and_image_without_proposals_add_nothing():
    gt = _gt([1, 2, 3], [_a(1, [0, 0, 10, 10], iscrowd=1), _a(2, [0, 0, 10, 10]), _a(3, [0, 0, 10, 10]), _a(3, [0, 0, 20, 20], iscrowd=1)])
    entries = [_e(1, [[0, 0, 10, 10]], [0.0]), _e(2, np.zeros((0, 4)), []), _e(3, [[0, 0, 20, 20]], [0.0])]
    r = R.evaluate(gt, entries)
    assert r["per_entry"][0] is None and r["per_entry"][1] is None and r["num_pos"] == 1
    assert r["per_entry"][2].tolist() == [0.25]                  # the crowd GT of image 3 is not a column
    r = R.evaluate(gt, entries[:2])
    assert r["num_pos"] == 0 and len(r["gt_overlaps"]) == 0 and np.isnan(r["recalls"]).all() and np.isnan(r["ar"])


def test_categories_outside_the_category_list_still_count():
    gt = _gt([1], [_a(1, [0, 0, 10, 10], category_id=77)])
    assert R.evaluate(gt, [_e(1, [[0, 0, 10, 10]], [0.0])])["num_pos"] == 1


# ------------------------------------------------------------------ evaluator host side

def _proposals(boxes, logits):
    from detectron2.structures import Boxes, Instances
    p = Instances((480, 640))
    p.proposal_boxes = Boxes(torch.tensor(boxes, dtype=torch.float32).reshape(-1, 4))
    p.objectness_logits = torch.tensor(logits, dtype=torch.float32)
    return p


def _patch_device_call(monkeypatch, gt_json, calls=None):
    """COCOEvaluator._proposal_recall answered by the restatement, in the device call's layout."""
    from detectron2.evaluation import COCOEvaluator

    def fake(self, props):
        if calls is not None:
            calls.append(len(props))
        res = R.evaluate_all(gt_json, [(i, b.cpu().numpy(), s.cpu().numpy()) for i, b, s in props])
        return {"num_pos": torch.tensor([r["num_pos"] for r in res.values()], dtype=torch.int64),
                "counts": torch.tensor(np.stack([r["counts"] for r in res.values()])), "status": torch.zeros(1, dtype=torch.int32)}

    monkeypatch.setattr(COCOEvaluator, "_proposal_recall", fake)


def _small_set():
    gt = _gt([4, 9], [_a(4, [0, 0, 10, 10]), _a(4, [10, 0, 10, 10], category_id=55), _a(9, [0, 0, 100, 100]), _a(9, [5, 5, 20, 20], iscrowd=1)])
    props = {4: _proposals([[5, 0, 15, 10], [18, 0, 20, 10]], [2.0, 1.0]), 9: _proposals([[0, 0, 100, 60]], [-3.0])}
    return gt, props


def test_process_keeps_proposals_without_copying(tmp_path):
    from detectron2.evaluation import COCOEvaluator
    gt, props = _small_set()
    _register("prop_host_process", gt, tmp_path)
    ev = COCOEvaluator("prop_host_process", distributed=False)
    ev.reset()
    inst = _instances([[1, 1, 3, 3]], [0.5], [0])
    ev.process([{"image_id": 4}, {"image_id": 9}, {"image_id": 9}], [{"proposals": props[4]}, {"instances": inst, "proposals": props[9]}, {"other": 1}])
    assert [p[0] for p in ev._proposals] == [4, 9] and [p[0] for p in ev._predictions] == [9]
    assert ev._proposals[0][1] is props[4].proposal_boxes.tensor and ev._proposals[0][2] is props[4].objectness_logits
    assert ev._proposals[1][1] is props[9].proposal_boxes.tensor and ev._predictions[0][1] is inst.pred_boxes.tensor
    ev.reset()
    assert ev._proposals == [] and ev._predictions == []


def test_gt_reader_has_a_per_image_view(tmp_path):
    from detectron2.evaluation import COCOEvaluator
    gt, _ = _small_set()
    _register("prop_host_gt", gt, tmp_path)
    g = COCOEvaluator("prop_host_gt", distributed=False)._gt
    assert g.img_ids == [4, 9] and g.img_off.tolist() == [0, 2, 4] and g.img_off.dtype == np.int32
    assert g.img_boxes.tolist() == [[0, 0, 10, 10], [10, 0, 10, 10], [0, 0, 100, 100], [5, 5, 20, 20]] and g.img_boxes.dtype == np.float64
    assert g.img_area.tolist() == [100, 100, 10000, 400] and g.img_crowd.tolist() == [0, 0, 0, 1]
    assert len(g.ids) == 3                                       # the (category, image) view still drops the unknown category


def test_box_proposals_keys_values_and_pickle(tmp_path, monkeypatch):
    from detectron2.evaluation import COCOEvaluator
    gt, props = _small_set()
    _register("prop_host_eval", gt, tmp_path)
    _patch_device_call(monkeypatch, gt)
    out = tmp_path / "inference"
    ev = COCOEvaluator("prop_host_eval", distributed=False, output_dir=str(out))
    ev.reset()
    ev.process([{"image_id": 9}, {"image_id": 4}], [{"proposals": props[9]}, {"proposals": props[4]}])
    res = ev.evaluate()
    assert list(res) == ["box_proposals"]                        # proposals only: no "bbox"
    assert list(res["box_proposals"]) == ["AR@100", "ARs@100", "ARm@100", "ARl@100", "AR@1000", "ARs@1000", "ARm@1000", "ARl@1000"]
    entries = [(9, props[9].proposal_boxes.tensor.numpy(), props[9].objectness_logits.numpy()),
               (4, props[4].proposal_boxes.tensor.numpy(), props[4].objectness_logits.numpy())]
    want = R.box_proposals(gt, entries)
    got = res["box_proposals"]
    assert all(isinstance(v, float) for v in got.values())
    assert all(got[k] == want[k] or (got[k] != got[k] and want[k] != want[k]) for k in want)     # no medium GT: NaN, as the reference
    assert got["ARm@100"] != got["ARm@100"] and got["ARl@1000"] == want["ARl@1000"] == 100.0 * float(torch.tensor([1.0] * 3 + [0.0] * 7).mean())
    # image 4: overlaps 1/3 and 0.2 (the GT of the unknown category counts); image 9: 0.6 -> recalls 1/3 at 0.5, 0.55, 0.6
    assert want["AR@100"] == float(torch.tensor([1 / 3] * 3 + [0.0] * 7, dtype=torch.float32).mean().item() * 100)
    assert ev.proposal_stats["AR@100"]["num_pos"] == 3 and ev.proposal_stats["ARs@100"]["num_pos"] == 2
    assert not os.path.exists(out / "coco_instances_results.json")
    data = pickle.load(open(out / "box_proposals.pkl", "rb"))
    assert list(data) == ["boxes", "objectness_logits", "ids", "bbox_mode"] and data["ids"] == [9, 4] and data["bbox_mode"] == 0
    assert all(isinstance(b, np.ndarray) for b in data["boxes"] + data["objectness_logits"])
    assert data["boxes"][1].tolist() == [[5, 0, 15, 10], [18, 0, 20, 10]] and data["objectness_logits"][0].tolist() == [-3.0]


def test_instances_only_is_unchanged_and_both_give_both(tmp_path, monkeypatch):
    from detectron2.evaluation import COCOEvaluator
    gt, props = _small_set()
    _register("prop_host_both", gt, tmp_path)
    calls = []
    _patch_device_call(monkeypatch, gt, calls)
    sentinel = {"AP": 12.5}
    seen = []
    monkeypatch.setattr(COCOEvaluator, "_eval_device", lambda self, preds: seen.append([p[0] for p in preds]) or dict(sentinel))
    ev = COCOEvaluator("prop_host_both", distributed=False)
    inst = _instances([[0, 0, 10, 10]], [0.9], [0])
    ev.reset()
    ev.process([{"image_id": 4}], [{"instances": inst}])
    res = ev.evaluate()
    assert list(res) == ["bbox"] and res["bbox"] == sentinel and calls == [] and seen == [[4]]
    ev.reset()
    ev.process([{"image_id": 4}, {"image_id": 9}], [{"instances": inst, "proposals": props[4]}, {"proposals": props[9]}])
    res = ev.evaluate()
    assert list(res) == ["box_proposals", "bbox"] and res["bbox"] == sentinel and calls == [2] and seen == [[4], [4]]
    ev.reset()
    ev.process([{"image_id": 4}], [{"neither": 0}])
    assert ev.evaluate() == {}


def test_unknown_image_id_in_proposals_is_refused(tmp_path, monkeypatch):
    from detectron2.evaluation import COCOEvaluator
    gt, props = _small_set()
    _register("prop_host_unknown", gt, tmp_path)
    _patch_device_call(monkeypatch, gt)
    ev = COCOEvaluator("prop_host_unknown", distributed=False)
    ev.reset()
    ev.process([{"image_id": 5}], [{"proposals": props[4]}])
    with pytest.raises(ValueError, match="do not correspond"):
        ev.evaluate()


# ------------------------------------------------------------------ the model's switch

def test_output_proposals_switch_swaps_only_this_objects_inference():
    from fewx.modeling.fsod.fsod_cen import CenterNet2Detector
    assert isinstance(CenterNet2Detector.__dict__["output_proposals"], property)
    m = CenterNet2Detector.__new__(CenterNet2Detector)
    torch.nn.Module.__init__(m)
    assert m.output_proposals is False and m.inference.__func__ is CenterNet2Detector.inference
    m.output_proposals = True
    assert m.output_proposals is True and m.inference.__func__ is CenterNet2Detector._inference_with_proposals
    m.output_proposals = False
    assert m.output_proposals is False and m.inference.__func__ is CenterNet2Detector.inference and "inference" not in m.__dict__
