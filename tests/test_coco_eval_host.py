"""CPU: COCO box AP (detectron2.evaluation.COCOEvaluator).  The numpy restatement of pycocotools' COCOeval (tests/coco_ref.py) on
hand-computed cases and against an independent brute-force 101-point AP; the evaluator's host side -- ground-truth reader and its
category-id mapping, results json, metric dict, all-NaN result, comm.gather order over 2 gloo ranks.  The device evaluation itself is
pinned to coco_ref in tests/test_hip_coco_eval.py."""
import json
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import coco_ref
from conftest import PKG


def _gt(images, annos, cats=(1,)):
    return {"images": [{"id": i, "width": 640, "height": 480, "file_name": f"{i}.png"} for i in images],
            "annotations": [dict(a, id=a.get("id", n + 1), iscrowd=a.get("iscrowd", 0), area=a.get("area", a["bbox"][2] * a["bbox"][3]))
                            for n, a in enumerate(annos)],
            "categories": [{"id": c, "name": f"c{c}"} for c in cats]}


def _det(img, box, score, cat=1):
    return {"image_id": img, "category_id": cat, "bbox": list(box), "score": score}


def _ap(r, k=0, a=0, m=2, t=slice(None)):
    p = r["precision"][t, :, k, a, m]
    return float(np.mean(p[p > -1])) if (p > -1).any() else -1.0


# ------------------------------------------------------------------ hand-computed cases

def test_perfect_detections_give_ap_1():
    gt = _gt([1, 2], [{"image_id": 1, "category_id": 1, "bbox": [10, 10, 50, 60]}, {"image_id": 2, "category_id": 1, "bbox": [5, 7, 200, 100]},
                      {"image_id": 2, "category_id": 1, "bbox": [300, 200, 20, 30]}])
    res = [_det(a["image_id"], a["bbox"], 0.9 - 0.1 * n) for n, a in enumerate(gt["annotations"])]
    r = coco_ref.evaluate(gt, res)
    assert _ap(r) == 1.0 and (r["recall"][:, 0, 0, 2] == 1.0).all()
    assert (r["precision"][:, :, 0, 0, 2] == 1.0).all()


def test_one_false_positive_above_all_true_positives():
    gt = _gt([1], [{"image_id": 1, "category_id": 1, "bbox": [10, 10, 50, 50]}, {"image_id": 1, "category_id": 1, "bbox": [100, 100, 50, 50]}])
    res = [_det(1, [300, 300, 40, 40], 0.9), _det(1, [10, 10, 50, 50], 0.8), _det(1, [100, 100, 50, 50], 0.7)]
    r = coco_ref.evaluate(gt, res)
    # sorted: FP, TP, TP -> precision 0, 1/2, 2/3; envelope 2/3 everywhere; recall thresholds all reached at the last TP
    want = 2.0 / (1.0 + 2.0 + np.spacing(1))
    assert (r["precision"][:, :, 0, 0, 2] == want).all()
    assert (r["scores"][:, 0, 0, 0, 2] == 0.9).all() and (r["scores"][:, 100, 0, 0, 2] == 0.7).all()
    assert (r["recall"][:, 0, 0, 2] == 1.0).all()
    # maxDets 1: only the FP of the image -> precision 0 at recall 0, nothing reached after it
    assert (r["precision"][:, :, 0, 0, 0] == 0.0).all() and (r["recall"][:, 0, 0, 0] == 0.0).all()


def test_crowd_gt_absorbs_several_detections():
    gt = _gt([1], [{"image_id": 1, "category_id": 1, "bbox": [10, 10, 50, 50]},
                   {"image_id": 1, "category_id": 1, "bbox": [100, 100, 200, 200], "iscrowd": 1}])
    res = [_det(1, [10, 10, 50, 50], 0.5), _det(1, [110, 110, 50, 50], 0.9), _det(1, [200, 200, 60, 60], 0.8),
           _det(1, [120, 220, 40, 40], 0.7)]
    r = coco_ref.evaluate(gt, res)
    e = r["eval_imgs"][0, 0, 0]
    assert e["gtIgnore"].tolist() == [0, 1]
    # the three detections inside the crowd region match it (area / det area = 1) and are ignored, at every threshold
    assert e["dtIgnore"][:, :3].all() and not e["dtIgnore"][:, 3].any()
    assert (e["dtMatches"][:, :3] == 2).all() and (e["dtMatches"][:, 3] == 1).all()
    assert _ap(r) == 1.0 / (1.0 + np.spacing(1))               # one TP, nothing else counted: 1 / (0 + 1 + eps)


def test_area_range_ignores():
    # a small GT (area 100) found exactly, a large GT missed, a medium detection on nothing
    gt = _gt([1], [{"image_id": 1, "category_id": 1, "bbox": [0, 0, 10, 10]}, {"image_id": 1, "category_id": 1, "bbox": [200, 200, 120, 120]}])
    res = [_det(1, [0, 0, 10, 10], 0.9), _det(1, [400, 10, 50, 50], 0.8)]
    r = coco_ref.evaluate(gt, res)
    small, medium, large = (r["eval_imgs"][0, a, 0] for a in (1, 2, 3))
    assert small["gtIgnore"].tolist() == [0, 1] and small["dtIgnore"][:, 0].sum() == 0 and small["dtIgnore"][:, 1].all()
    assert medium["gtIgnore"].tolist() == [1, 1]
    assert medium["dtIgnore"][:, 0].all()                       # matched to an ignored GT
    assert not medium["dtIgnore"][:, 1].any()                   # unmatched, area 2500 inside the medium range
    assert (r["precision"][:, :, 0, 2, :] == -1).all() and (r["recall"][:, 0, 2, :] == -1).all()   # no medium GT: -1
    assert _ap(r, a=1) == 1.0 / (1.0 + np.spacing(1)) and _ap(r, a=3) == 0.0
    assert (r["recall"][:, 0, 0, 2] == 0.5).all()


def test_more_than_100_detections_in_an_image():
    gt = _gt([1], [{"image_id": 1, "category_id": 1, "bbox": [0, 0, 40, 40]}])
    res = [_det(1, [500, 400, 10, 10], 1.0 - i / 1000) for i in range(150)]
    res.append(_det(1, [0, 0, 40, 40], 0.5))                  # rank 150: cut by maxDets[-1] = 100
    r = coco_ref.evaluate(gt, res)
    assert len(r["eval_imgs"][0, 0, 0]["dtIds"]) == 100
    assert (r["recall"][:, 0, 0, :] == 0).all() and _ap(r) == 0.0
    res[-1]["score"] = 0.9995                                 # now rank 1: inside maxDets 10 and 100, not 1
    r = coco_ref.evaluate(gt, res)
    assert (r["recall"][:, 0, 0, 0] == 0).all() and (r["recall"][:, 0, 0, 1] == 1).all() and (r["recall"][:, 0, 0, 2] == 1).all()
    assert (r["precision"][:, 0, 0, 0, 1] == 1.0 / (1.0 + 1.0 + np.spacing(1))).all()


@pytest.mark.parametrize("fp_first", [True, False])
def test_score_ties_across_images_go_by_image_id(fp_first):
    fp_img, tp_img = (3, 8) if fp_first else (8, 3)
    gt = _gt([3, 8], [{"image_id": tp_img, "category_id": 1, "bbox": [0, 0, 40, 40]}])
    res = [_det(tp_img, [0, 0, 40, 40], 0.5), _det(fp_img, [100, 100, 40, 40], 0.5)]
    r = coco_ref.evaluate(gt, res)
    p = r["precision"][0, :, 0, 0, 2]
    if fp_first:      # FP, TP: precision 0, 1/2 -> envelope 1/2
        assert (p == 1.0 / (1.0 + 1.0 + np.spacing(1))).all()
    else:             # TP, FP: 1, 1/2 -> 1 at every recall up to 1
        assert (p == 1.0 / (1.0 + np.spacing(1))).all()


def test_gt_with_id_0_counts_as_false_positive():
    gt = _gt([1], [{"image_id": 1, "category_id": 1, "bbox": [0, 0, 40, 40], "id": 0}])
    r = coco_ref.evaluate(gt, [_det(1, [0, 0, 40, 40], 0.9)])
    e = r["eval_imgs"][0, 0, 0]
    assert (e["dtMatches"] == 0).all() and not e["dtIgnore"].any()     # matched, but "matched" means id != 0
    assert (r["precision"][:, :, 0, 0, 2] == 0).all() and (r["recall"][:, 0, 0, 2] == 0).all()


def test_empty_category_gives_minus_1_then_nan():
    from detectron2.evaluation.coco_evaluation import derive_coco_results, summarize
    gt = _gt([1], [{"image_id": 1, "category_id": 1, "bbox": [0, 0, 40, 40]}], cats=(1, 2))
    r = coco_ref.evaluate(gt, [_det(1, [0, 0, 40, 40], 0.9)])
    assert (r["precision"][:, :, 1] == -1).all() and (r["recall"][:, 1] == -1).all()
    stats, lines = summarize(r["precision"], r["recall"])
    res = derive_coco_results(stats, r["precision"], ["c1", "c2"])
    one = 100.0 / (1.0 + np.spacing(1))
    assert res["AP"] == one and res["AP-c1"] == one and math.isnan(res["AP-c2"])
    assert math.isnan(res["APs"]) and math.isnan(res["APl"]) and res["APm"] == one     # the one GT (40 x 40) is medium


# ------------------------------------------------------------------ brute force

def _random_case(seed, n_img=6, n_cat=2):
    rng = np.random.default_rng(seed)
    images = list(rng.choice(1000, n_img, replace=False) + 1)
    annos = []
    for im in images:
        for _ in range(int(rng.integers(0, 7))):
            x, y = rng.integers(0, 20, 2) * 8.0
            w, h = rng.integers(1, 16, 2) * 4.0
            annos.append({"image_id": int(im), "category_id": int(rng.integers(1, n_cat + 1)), "bbox": [x, y, w, h],
                          "iscrowd": int(rng.random() < 0.1), "area": float(w * h * rng.choice([0.5, 1.0, 40.0]))})
    gt = _gt([int(i) for i in images], annos, cats=tuple(range(1, n_cat + 1)))
    res = []
    for im in images:
        for _ in range(int(rng.integers(0, 14))):
            if annos and rng.random() < 0.6:
                a = annos[int(rng.integers(len(annos)))]
                b = [v + float(rng.integers(-2, 3)) * 2 for v in a["bbox"]]
                b[2], b[3] = max(b[2], 1.0), max(b[3], 1.0)
            else:
                b = [float(v) for v in rng.integers(0, 160, 2) * 1.0] + [float(v) for v in rng.integers(1, 60, 2) * 1.0]
            res.append(_det(int(im), b, float(np.float32(rng.integers(1, 8) / 8)), int(rng.integers(1, n_cat + 1))))
    return gt, res


def _brute_force(r, max_dets=coco_ref.MAX_DETS, rec_thrs=coco_ref.REC_THRS):
    """101-point AP from the per-image matches alone: explicit sort key, running counts by counting, envelope as a max over the
    tail, the recall index by a linear scan (no cumsum, no searchsorted)."""
    T, R = len(coco_ref.IOU_THRS), len(rec_thrs)
    K, A, M = len(r["cat_ids"]), len(coco_ref.AREA_RNG), len(max_dets)
    prec, rec, sc = -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M)), -np.ones((T, R, K, A, M))
    n_img = len(r["img_ids"])
    for k in range(K):
        for a in range(A):
            E = [(i, r["eval_imgs"][k, a, i]) for i in range(n_img) if r["eval_imgs"][k, a, i] is not None]
            if not E:
                continue
            npig = sum(int((e["gtIgnore"] == 0).sum()) for _, e in E)
            if npig == 0:
                continue
            for m, md in enumerate(max_dets):
                for t in range(T):
                    items = [(-e["dtScores"][j], i, j, bool(e["dtMatches"][t, j]), bool(e["dtIgnore"][t, j]), e["dtScores"][j])
                             for i, e in E for j in range(min(md, len(e["dtScores"])))]
                    items.sort(key=lambda x: (x[0], x[1], x[2]))
                    nd = len(items)
                    tp = [float(sum(1 for x in items[:j + 1] if x[3] and not x[4])) for j in range(nd)]
                    fp = [float(sum(1 for x in items[:j + 1] if not x[3] and not x[4])) for j in range(nd)]
                    pr = [tp[j] / (fp[j] + tp[j] + np.spacing(1)) for j in range(nd)]
                    env = [max(pr[j:]) for j in range(nd)]
                    rec[t, k, a, m] = tp[-1] / npig if nd else 0
                    for ri, thr in enumerate(rec_thrs):
                        j = next((j for j in range(nd) if tp[j] / npig >= thr), None)
                        prec[t, ri, k, a, m] = env[j] if j is not None else 0.0
                        sc[t, ri, k, a, m] = items[j][5] if j is not None else 0.0
    return prec, rec, sc


@pytest.mark.parametrize("seed", range(12))
def test_brute_force_101_point_ap_agrees(seed):
    gt, res = _random_case(seed)
    r = coco_ref.evaluate(gt, res)
    p, rc, s = _brute_force(r)
    assert np.array_equal(p, r["precision"]) and np.array_equal(rc, r["recall"]) and np.array_equal(s, r["scores"])


# ------------------------------------------------------------------ evaluator host side

def _instances(boxes_xyxy, scores, classes):
    from detectron2.structures import Boxes, Instances
    inst = Instances((480, 640))
    inst.pred_boxes = Boxes(torch.tensor(boxes_xyxy, dtype=torch.float32).reshape(-1, 4))
    inst.scores = torch.tensor(scores, dtype=torch.float32)
    inst.pred_classes = torch.tensor(classes, dtype=torch.int64)
    return inst


def _register(name, gt, tmp_path):
    from fewx.data.datasets.register_coco import register_coco_instances
    from detectron2.data import DatasetCatalog, MetadataCatalog
    path = os.path.join(str(tmp_path), name + ".json")
    with open(path, "w") as f:
        json.dump(gt, f)
    if name in DatasetCatalog:
        DatasetCatalog.remove(name)
        MetadataCatalog.pop(name)
    register_coco_instances(name, {}, path, str(tmp_path))
    return path


def test_import_surface():
    from detectron2.evaluation import COCOEvaluator, DatasetEvaluator, DatasetEvaluators, print_csv_format  # noqa: F401
    assert issubclass(COCOEvaluator, DatasetEvaluator) and issubclass(DatasetEvaluators, DatasetEvaluator)


def test_tasks_other_than_bbox_refused(tmp_path):
    from detectron2.evaluation import COCOEvaluator
    gt = _gt([1], [{"image_id": 1, "category_id": 1, "bbox": [0, 0, 4, 4]}])
    _register("coco_host_tasks", gt, tmp_path)
    for tasks in (("segm",), ("bbox", "keypoints")):
        with pytest.raises(ValueError, match="bbox"):
            COCOEvaluator("coco_host_tasks", tasks)
    COCOEvaluator("coco_host_tasks", ("bbox",), False, use_fast_impl=False)


def test_gt_reader_groups_by_category_and_image_with_id_mapping(tmp_path):
    from detectron2.evaluation import COCOEvaluator
    annos = [{"image_id": 20, "category_id": 7, "bbox": [1, 2, 3, 4], "id": 11}, {"image_id": 5, "category_id": 3, "bbox": [5, 6, 7, 8], "id": 12},
             {"image_id": 20, "category_id": 3, "bbox": [9, 9, 9, 9], "id": 13, "iscrowd": 1},
             {"image_id": 20, "category_id": 7, "bbox": [2, 2, 2, 2], "id": 14, "area": 77.5}]
    _register("coco_host_gt", _gt([20, 5], annos, cats=(7, 3)), tmp_path)
    ev = COCOEvaluator("coco_host_gt", distributed=False)
    g = ev._gt
    assert g.img_ids == [5, 20] and g.cat_ids == [3, 7] and g.cat_names == ["c3", "c7"]
    assert g.off.tolist() == [0, 1, 2, 2, 4]                   # pairs (cat 3, img 5), (3, 20), (7, 5), (7, 20)
    assert g.ids.tolist() == [12, 13, 11, 14] and g.crowd.tolist() == [0, 1, 0, 0]
    assert g.area.tolist() == [56.0, 81.0, 12.0, 77.5] and g.boxes[3].tolist() == [2, 2, 2, 2]
    assert g.contiguous_to_dataset_id == {0: 3, 1: 7}


def test_results_json_is_instances_to_coco_json(tmp_path):
    from detectron2.evaluation import COCOEvaluator
    gt = _gt([4, 9], [{"image_id": 4, "category_id": 7, "bbox": [0, 0, 4, 4]}], cats=(7, 3))
    _register("coco_host_json", gt, tmp_path)
    out = tmp_path / "inference"
    ev = COCOEvaluator("coco_host_json", distributed=False, output_dir=str(out))
    ev.reset()
    b0 = [[0.1, 0.2, 10.3, 20.7], [5.5, 6.25, 7.0, 9.125]]
    ev.process([{"image_id": 9}, {"image_id": 4}], [{"instances": _instances(b0, [0.7, 0.3], [0, 1])},
                                                   {"instances": _instances([[1, 1, 3, 3]], [0.123456789], [1])}])
    rows = ev._coco_results(ev._gather_predictions())
    assert [r["image_id"] for r in rows] == [9, 9, 4] and [r["category_id"] for r in rows] == [3, 7, 7]
    b = np.float32(b0[0])
    assert rows[0]["bbox"] == [float(b[0]), float(b[1]), float(b[2] - b[0]), float(b[3] - b[1])]
    assert rows[2]["score"] == float(np.float32(0.123456789))
    # written by evaluate() only when there are detections to evaluate; exercised here through the no-detection path
    ev.reset()
    ev.process([{"image_id": 4}], [{"instances": _instances(np.zeros((0, 4)), [], [])}])
    res = ev.evaluate()
    assert json.load(open(out / "coco_instances_results.json")) == []
    assert list(res) == ["bbox"] and all(math.isnan(v) for v in res["bbox"].values())
    assert sorted(res["bbox"]) == sorted(["AP", "AP50", "AP75", "APs", "APm", "APl"])


def test_no_predictions_at_all_gives_empty_dict(tmp_path):
    from detectron2.evaluation import COCOEvaluator
    _register("coco_host_empty", _gt([1], []), tmp_path)
    ev = COCOEvaluator("coco_host_empty", distributed=False)
    ev.reset()
    assert ev.evaluate() == {}


def test_gt_from_dataset_catalog_without_json_file():
    from detectron2.data import DatasetCatalog, MetadataCatalog
    from detectron2.evaluation import COCOEvaluator
    name = "coco_host_catalog"
    if name in DatasetCatalog:
        DatasetCatalog.remove(name)
        MetadataCatalog.pop(name)
    dicts = [{"image_id": 3, "height": 10, "width": 10, "file_name": "a", "annotations": [
        {"bbox": [0.12345, 0.2, 3.33333, 4.4], "bbox_mode": 1, "category_id": 1}, {"bbox": [1, 1, 5, 6], "bbox_mode": 0, "category_id": 0, "iscrowd": 1}]}]
    DatasetCatalog.register(name, lambda: dicts)
    MetadataCatalog.get(name).set(thing_classes=["a", "b"])
    ev = COCOEvaluator(name, distributed=False)
    g = ev._gt
    assert g.cat_ids == [0, 1] and g.ids.tolist() == [2, 1]    # ids 1..N in record order; pair (cat 0) first
    x, y, w, h = np.float32([0.12345, 0.2, 3.33333, 4.4])
    assert g.area[1] == float((np.float32(x + w) - x) * (np.float32(y + h) - y))   # from the unrounded box
    assert g.boxes[1].tolist() == [0.123, 0.2, 3.333, 4.4]          # convert_to_coco_json rounds the stored box to 3 decimals
    assert g.boxes[0].tolist() == [1.0, 1.0, 4.0, 5.0] and g.crowd.tolist() == [1, 0]


def test_metric_dict_and_csv(caplog):
    from collections import OrderedDict
    from detectron2.evaluation import print_csv_format
    from detectron2.evaluation.coco_evaluation import derive_coco_results, summarize
    gt, res = _random_case(3)
    r = coco_ref.evaluate(gt, res)
    stats, lines = summarize(r["precision"], r["recall"])
    assert len(lines) == 12 and lines[0].startswith(" Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = ")
    assert lines[6].startswith(" Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=  1 ] = ")
    p = r["precision"]
    assert stats[0] == np.mean(p[:, :, :, 0, 2][p[:, :, :, 0, 2] > -1]) and stats[1] == np.mean(p[0, :, :, 0, 2][p[0, :, :, 0, 2] > -1])
    d = derive_coco_results(stats, p, ["x", "y"])
    assert list(d) == ["AP", "AP50", "AP75", "APs", "APm", "APl", "AP-x", "AP-y"] and d["AP"] == float(stats[0] * 100)
    assert list(derive_coco_results(stats, p, ["x"])) == ["AP", "AP50", "AP75", "APs", "APm", "APl"]
    with caplog.at_level("INFO"):
        print_csv_format(OrderedDict(bbox=d))
    assert "copypaste: AP,AP50,AP75,APs,APm,APl" in caplog.text


def test_dataset_evaluators_merge():
    from detectron2.evaluation import DatasetEvaluator, DatasetEvaluators

    class E(DatasetEvaluator):
        def __init__(self, key):
            self.key, self.n = key, 0

        def reset(self):
            self.n = 0

        def process(self, inputs, outputs):
            self.n += len(inputs)

        def evaluate(self):
            return {self.key: self.n}

    ev = DatasetEvaluators([E("a"), E("b")])
    ev.reset()
    ev.process([1, 2], [1, 2])
    assert ev.evaluate() == {"a": 2, "b": 2}
    with pytest.raises(AssertionError):
        DatasetEvaluators([E("a"), E("a")]).evaluate()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gather_worker(rank, world, port, json_path, q):
    import sys
    sys.path.insert(0, PKG)
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from detectron2.data import MetadataCatalog
        from detectron2.evaluation import COCOEvaluator
        MetadataCatalog.get("coco_host_dist").set(json_file=json_path)
        ev = COCOEvaluator("coco_host_dist", distributed=True)
        ev.reset()
        for n in range(2):                                     # rank r processes images 10r+1, 10r+2
            img = 10 * rank + n + 1
            ev.process([{"image_id": img}], [{"instances": _instances([[img, 0, img + 5, 5]], [0.5 + rank / 10 + n / 100], [0])}])
        preds = ev._gather_predictions()
        q.put((rank, [(p[0], p[1].tolist(), p[2].tolist()) for p in preds]))
    finally:
        dist.destroy_process_group()


def test_gather_order_over_two_gloo_ranks(tmp_path):
    gt = _gt([1, 2, 11, 12], [{"image_id": 1, "category_id": 1, "bbox": [0, 0, 4, 4]}])
    path = str(tmp_path / "gt.json")
    with open(path, "w") as f:
        json.dump(gt, f)
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gather_worker, args=(r, world, port, path, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert got[1] == []
    assert [p[0] for p in got[0]] == [1, 2, 11, 12]            # rank 0's predictions, then rank 1's
    assert got[0][2][1] == [[11.0, 0.0, 16.0, 5.0]] and got[0][3][2] == [pytest.approx(0.61)]
