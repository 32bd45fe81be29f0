"""GPU: COCO box AP on the device (csrc/ore_coco_eval.hip through orehip.coco_eval and detectron2.evaluation.COCOEvaluator), bit for
bit against the numpy restatement of pycocotools' COCOeval (tests/coco_ref.py): the per-image stage's arrays and precision / recall /
scores, on seeded random datasets and end to end through a seeded model (as bench.py builds it)."""
import json
import os

import numpy as np
import pytest
import torch

import coco_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ore():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import orehip
    orehip.lib()
    return orehip


def _dataset(seed, big_image=False):
    """A random COCO set on a quantised grid (exact IoU and score ties), crowd GTs, GT-only and detection-only images, several
    categories, sometimes more than 100 detections in an image.  Detections as the model returns them: XYXY fp32 rows."""
    rng = np.random.default_rng(seed)
    n_img, n_cat = int(rng.integers(1, 9)), int(rng.integers(1, 4))
    img_ids = sorted(int(v) for v in rng.choice(500, n_img, replace=False) + 1)
    cat_ids = sorted(int(v) for v in rng.choice(20, n_cat, replace=False))        # category id 0 allowed
    q = float(rng.choice([1.0, 4.0, 0.5]))
    annos, dets = [], []
    aid = int(rng.integers(0, 2))                                                   # sometimes a GT with id 0
    for im in img_ids:
        mode = rng.integers(0, 4)                                                    # 0: GT only, 1: detections only, else both
        n_gt = 0 if mode == 1 else int(rng.integers(0, 12))
        if big_image and im == img_ids[0]:
            n_gt = 3000
        for _ in range(n_gt):
            x, y = rng.integers(0, 40, 2) * q * 4
            w, h = rng.integers(1, 30, 2) * q * 2
            annos.append({"id": aid, "image_id": im, "category_id": cat_ids[int(rng.integers(n_cat))], "bbox": [float(x), float(y), float(w), float(h)],
                          "iscrowd": int(rng.random() < 0.08), "area": float(w * h * rng.choice([1.0, 1.0, 0.3, 30.0]))})
            aid += 1
        n_dt = 0 if mode == 0 else int(rng.choice([rng.integers(0, 20), rng.integers(90, 160)], p=[0.85, 0.15]))
        if big_image and im == img_ids[0]:
            n_dt = 40
        mine = [a for a in annos if a["image_id"] == im]
        for _ in range(n_dt):
            if mine and rng.random() < 0.6:
                a = mine[int(rng.integers(len(mine)))]
                x0, y0 = a["bbox"][0] + rng.integers(-2, 3) * q, a["bbox"][1] + rng.integers(-2, 3) * q
                x1, y1 = x0 + a["bbox"][2] + rng.integers(-2, 3) * q, y0 + a["bbox"][3] + rng.integers(-2, 3) * q
                c = a["category_id"] if rng.random() < 0.9 else cat_ids[int(rng.integers(n_cat))]
            else:
                x0, y0 = rng.integers(0, 40, 2) * q * 4 + rng.random(2) * q
                x1, y1 = x0 + rng.integers(1, 30) * q * 2, y0 + rng.integers(1, 30) * q * 2
                c = cat_ids[int(rng.integers(n_cat))]
            s = float(np.float32(rng.integers(1, 9) / 8 if rng.random() < 0.7 else rng.random()))
            dets.append((im, c, [float(x0), float(y0), float(max(x1, x0 + q)), float(max(y1, y0 + q))], s))
    gt = {"images": [{"id": i} for i in img_ids], "annotations": annos, "categories": [{"id": c, "name": f"c{c}"} for c in cat_ids]}
    perm = rng.permutation(len(dets))                                              # results order is not image order
    return gt, [dets[i] for i in perm]


def _results(dets):
    """instances_to_coco_json of the XYXY fp32 rows."""
    out = []
    for im, c, b, s in dets:
        x0, y0, x1, y1 = np.float32(b)
        out.append({"image_id": im, "category_id": c, "bbox": [float(x0), float(y0), float(x1 - x0), float(y1 - y0)], "score": s})
    return out


def _run(ore, gt, dets):
    from detectron2.evaluation.coco_evaluation import AREA_RNG, IOU_THRS, MAX_DETS, REC_THRS, CocoGT
    g = CocoGT(gt)
    dev = torch.device("cuda")
    boxes = torch.tensor([d[2] for d in dets], dtype=torch.float32).reshape(-1, 4).to(dev)
    scores = torch.tensor([d[3] for d in dets], dtype=torch.float32).to(dev)
    img = torch.tensor([g.img_index[d[0]] for d in dets], dtype=torch.int32).to(dev)
    cat = torch.tensor([g.cat_index[d[1]] for d in dets], dtype=torch.int32).to(dev)
    out = ore.coco_eval(boxes, scores, img, cat, g.device(dev), len(g.img_ids), len(g.cat_ids), IOU_THRS, REC_THRS, AREA_RNG, MAX_DETS,
                        per_image=True)
    torch.cuda.synchronize()
    return g, {k: v.cpu().numpy() for k, v in out.items()}


def _check(gt, dets, got, g):
    ref = coco_ref.evaluate(gt, _results(dets))
    I = len(g.img_ids)
    units = [(k, i) for k in range(len(g.cat_ids)) for i in range(I) if ref["eval_imgs"][k, 0, i] is not None]
    n = int(got["n_units"][0])
    assert n == len(units) and [tuple(divmod(int(p), I)) for p in got["unit_pair"][:n]] == units
    for u, (k, i) in enumerate(units):
        for a in range(len(coco_ref.AREA_RNG)):
            e = ref["eval_imgs"][k, a, i]
            D = len(e["dtIds"])
            assert np.array_equal(got["det_index"][u, :D], np.array(e["dtIds"], dtype=np.int64) - 1), (u, a)
            assert np.array_equal(got["dt_matches"][u, a, :, :D], e["dtMatches"].astype(np.int64)), (u, a)
            assert np.array_equal(got["dt_ignore"][u, a, :, :D], e["dtIgnore"].astype(np.uint8)), (u, a)
            assert got["gt_npig"][u, a] == int((e["gtIgnore"] == 0).sum()), (u, a)
    for key in ("precision", "recall", "scores"):
        assert got[key].tobytes() == ref[key].tobytes(), key
    return ref


@pytest.mark.parametrize("block", range(6))
def test_random_datasets_bitwise(ore, block):
    """300 seeded random datasets (50 per parametrised block)."""
    for seed in range(50 * block, 50 * block + 50):
        gt, dets = _dataset(seed)
        g, got = _run(ore, gt, dets)
        _check(gt, dets, got, g)


def test_image_with_3000_gts_bitwise(ore):
    """Past the LDS sizes: the IoU matrix and the matched flags of that image live in the workspace."""
    gt, dets = _dataset(1234, big_image=True)
    g, got = _run(ore, gt, dets)
    assert int(np.diff(g.off).max()) >= 1000
    ref = _check(gt, dets, got, g)
    assert (ref["precision"] > 0).any()


def _hand_cases():
    """The hand-computed cases of tests/test_coco_eval_host.py (whose expected values are pinned there against coco_ref), as
    (gt, detections with XYXY rows and fp32 scores)."""
    from test_coco_eval_host import _det, _gt
    a = lambda im, box, **kw: dict({"image_id": im, "category_id": 1, "bbox": box}, **kw)
    cases = {
        "perfect": (_gt([1, 2], [a(1, [10, 10, 50, 60]), a(2, [5, 7, 200, 100]), a(2, [300, 200, 20, 30])]),
                    [_det(1, [10, 10, 50, 60], 0.9), _det(2, [5, 7, 200, 100], 0.8), _det(2, [300, 200, 20, 30], 0.7)]),
        "fp_above": (_gt([1], [a(1, [10, 10, 50, 50]), a(1, [100, 100, 50, 50])]),
                     [_det(1, [300, 300, 40, 40], 0.9), _det(1, [10, 10, 50, 50], 0.8), _det(1, [100, 100, 50, 50], 0.7)]),
        "crowd": (_gt([1], [a(1, [10, 10, 50, 50]), a(1, [100, 100, 200, 200], iscrowd=1)]),
                  [_det(1, [10, 10, 50, 50], 0.5), _det(1, [110, 110, 50, 50], 0.9), _det(1, [200, 200, 60, 60], 0.8),
                   _det(1, [120, 220, 40, 40], 0.7)]),
        "areas": (_gt([1], [a(1, [0, 0, 10, 10]), a(1, [200, 200, 120, 120])]), [_det(1, [0, 0, 10, 10], 0.9), _det(1, [400, 10, 50, 50], 0.8)]),
        "over_100": (_gt([1], [a(1, [0, 0, 40, 40])]),
                     [_det(1, [500, 400, 10, 10], 1.0 - i / 1000) for i in range(150)] + [_det(1, [0, 0, 40, 40], 0.9995)]),
        "ties_fp_first": (_gt([3, 8], [a(8, [0, 0, 40, 40])]), [_det(8, [0, 0, 40, 40], 0.5), _det(3, [100, 100, 40, 40], 0.5)]),
        "ties_tp_first": (_gt([3, 8], [a(3, [0, 0, 40, 40])]), [_det(3, [0, 0, 40, 40], 0.5), _det(8, [100, 100, 40, 40], 0.5)]),
        "gt_id_0": (_gt([1], [a(1, [0, 0, 40, 40], id=0)]), [_det(1, [0, 0, 40, 40], 0.9)]),
        "empty_category": (_gt([1], [a(1, [0, 0, 40, 40])], cats=(1, 2)), [_det(1, [0, 0, 40, 40], 0.9)]),
    }
    out = {}
    for name, (gt, rows) in cases.items():
        dets = [(r["image_id"], r["category_id"], [r["bbox"][0], r["bbox"][1], r["bbox"][0] + r["bbox"][2], r["bbox"][1] + r["bbox"][3]],
                 float(np.float32(r["score"]))) for r in rows]
        out[name] = (gt, dets)
    return out


@pytest.mark.parametrize("case", sorted(_hand_cases()))
def test_hand_computed_cases_bitwise(ore, case):
    gt, dets = _hand_cases()[case]
    g, got = _run(ore, gt, dets)
    _check(gt, dets, got, g)


def _large_dataset(seed, n_img=1100):
    """Sized to run every multi-block path of the device code: > 1024 (category, image) pairs (k_pairs_scan's carry across
    1024-pair tiles), > 5000 kept detections in one category (k_accumulate's carry across 4096-element tiles) and > 8192 detections
    in all (a padded sort of 16384: global bitonic steps between the 2048-element LDS blocks).  Scores on a 1/16 grid: ties across
    images everywhere, so the sort's (image, rank) tie-break decides the order."""
    rng = np.random.default_rng(seed)
    img_ids = sorted(int(v) for v in rng.choice(5 * n_img, n_img, replace=False) + 1)
    annos, dets = [], []
    for im in img_ids:
        mine = []
        for _ in range(int(rng.integers(0, 5))):
            x, y = rng.integers(0, 30, 2) * 8.0
            w, h = rng.integers(2, 24, 2) * 4.0
            a = {"id": len(annos) + 1, "image_id": im, "category_id": 1 if rng.random() < 0.7 else 2, "bbox": [x, y, w, h],
                 "iscrowd": int(rng.random() < 0.05), "area": float(w * h)}
            annos.append(a)
            mine.append(a)
        for c, n in ((1, int(rng.integers(4, 10))), (2, int(rng.integers(0, 4)))):
            for _ in range(n):
                if mine and rng.random() < 0.5:
                    a = mine[int(rng.integers(len(mine)))]
                    x0, y0 = a["bbox"][0] + rng.integers(-2, 3), a["bbox"][1] + rng.integers(-2, 3)
                    x1, y1 = x0 + a["bbox"][2] + rng.integers(-2, 3), y0 + a["bbox"][3] + rng.integers(-2, 3)
                else:
                    x0, y0 = rng.integers(0, 30, 2) * 8.0
                    x1, y1 = x0 + rng.integers(2, 24) * 4.0, y0 + rng.integers(2, 24) * 4.0
                dets.append((im, c, [float(x0), float(y0), float(x1), float(y1)], float(rng.integers(1, 17) / 16)))
    gt = {"images": [{"id": i} for i in img_ids], "annotations": annos, "categories": [{"id": 1, "name": "ore"}, {"id": 2, "name": "gangue"}]}
    perm = rng.permutation(len(dets))
    return gt, [dets[i] for i in perm]


def test_large_set_multi_block_paths_bitwise(ore):
    gt, dets = _large_dataset(2024)
    g, got = _run(ore, gt, dets)
    kept_cat1 = sum(min(n, 100) for n in np.unique([d[0] for d in dets if d[1] == 1], return_counts=True)[1])
    sort_size = max(2048, 1 << (len(dets) - 1).bit_length())
    assert int(got["n_units"][0]) > 1024 and kept_cat1 > 5000 and sort_size >= 16384, (int(got["n_units"][0]), kept_cat1, sort_size)
    ref = _check(gt, dets, got, g)
    assert (ref["precision"] > 0).any() and (ref["precision"][:, :, 1] > 0).any()


def test_deterministic_and_no_detections(ore):
    gt, dets = _dataset(77)
    _, a = _run(ore, gt, dets)
    _, b = _run(ore, gt, dets)
    for key in ("precision", "recall", "scores", "dt_matches", "dt_ignore"):
        assert a[key].tobytes() == b[key].tobytes()
    g, got = _run(ore, gt, [])
    _check(gt, [], got, g)


# ------------------------------------------------------------------ end to end

def _setup_script(tmp_path, monkeypatch, two_categories):
    from test_entry_script import _args, _load_script, _write_dataset
    monkeypatch.chdir(tmp_path)
    _write_dataset(str(tmp_path), n_img=6, per_img=3)
    m = _load_script()
    cfg = m.setup(_args(m, tmp_path))
    name = cfg.DATASETS.TEST[0]
    path = os.path.join("datasets", "coco", "annotations", "instances_val2017.json")
    gt = json.load(open(path))
    if two_categories:                                         # categories 1 and 4; every other GT of category 4
        gt["categories"].append({"id": 4, "name": "gangue"})
        for n, a in enumerate(gt["annotations"]):
            a["category_id"] = 4 if n % 2 else 1
        json.dump(gt, open(path, "w"))
    from detectron2.data import DatasetCatalog
    DatasetCatalog.get(name)                                   # refreshes the catalog's id mapping for this json
    return m, cfg, name, gt


def _model(two_categories):
    import bench
    model, _ = bench.build_model("cuda")
    if two_categories:
        g = torch.Generator().manual_seed(5)
        sd = model.support_dict
        for key in sd:
            sd[key][1] = sd[key][0] + torch.randn(sd[key][0].shape, generator=g).to(sd[key][0].device) * 0.05
        model.set_support_dict(sd)
        model.support_classes = "all"
    return model


@pytest.mark.parametrize("two_categories", [False, True], ids=["default", "nway_all"])
def test_end_to_end_matches_reference_on_results_json(ore, tmp_path, monkeypatch, two_categories):
    from detectron2.evaluation import COCOEvaluator, inference_on_dataset
    m, cfg, name, gt = _setup_script(tmp_path, monkeypatch, two_categories)
    model = _model(two_categories)
    outs = {}
    for how in ("inference_on_dataset", "trainer_test"):
        out_dir = str(tmp_path / how)
        ev = COCOEvaluator(name, output_dir=out_dir)
        if how == "trainer_test":
            res = m.Trainer.test(cfg, model, evaluators=[ev])
        else:
            res = inference_on_dataset(model, m.Trainer.build_test_loader(cfg, name), ev)
        rows = json.load(open(os.path.join(out_dir, "coco_instances_results.json")))
        assert len(rows) > 0
        ref = coco_ref.evaluate(gt, rows)
        for key in ("precision", "recall", "scores"):
            assert getattr(ev, key).tobytes() == ref[key].tobytes(), (how, key)
        assert set(r["category_id"] for r in rows) <= {c["id"] for c in gt["categories"]}
        if two_categories:
            assert {r["category_id"] for r in rows} == {1, 4}
            assert set(res["bbox"]) >= {"AP-ore", "AP-gangue"}
        outs[how] = (rows, res)
    assert outs["inference_on_dataset"][0] == outs["trainer_test"][0]
    a, b = outs["inference_on_dataset"][1]["bbox"], outs["trainer_test"][1]["bbox"]
    assert list(a) == list(b) and all(x == y or (x != x and y != y) for x, y in zip(a.values(), b.values()))
