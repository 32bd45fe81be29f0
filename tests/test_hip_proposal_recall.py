"""GPU: proposal recall on the device (csrc/ore_proposal_recall.hip through orehip.proposal_recall and
detectron2.evaluation.COCOEvaluator), bit for bit against the restatement of its contract (tests/proposal_recall_ref.py): the per-entry
recorded vectors, gt_overlaps, counts, recalls, ar and num_pos of all eight (limit, area) chains -- on seeded random sets, on images past
the LDS sizes and past both limits, on the recorded set whose expected bytes are the reference's own, and end to end through a seeded
model with CenterNet2Detector.output_proposals."""
import os

import numpy as np
import pytest
import torch

import proposal_recall_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ore():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import orehip
    orehip.lib()
    return orehip


def _dataset(seed, big=None):
    """1-8 images with 0-12 GTs on a quantised grid (exact IoU ties), some crowd, some of a category that is not in `categories`; per
    image 0-20 or 90-160 proposals, now and then 1001-1100, logits on a 1/8 grid (ties); the entries shuffled, and in some sets one
    image answered twice.  big = (GTs, proposals) of the first image."""
    rng = np.random.default_rng(seed)
    n_img = int(rng.integers(1, 9))
    img_ids = sorted(int(v) for v in rng.choice(500, n_img, replace=False) + 1)
    q = float(rng.choice([1.0, 4.0, 0.5]))
    annos, entries = [], []

    def proposals(mine, n_pr):
        boxes = []
        for _ in range(n_pr):
            if mine and rng.random() < 0.6:
                a = mine[int(rng.integers(len(mine)))]
                x0, y0 = a["bbox"][0] + rng.integers(-2, 3) * q, a["bbox"][1] + rng.integers(-2, 3) * q
                x1, y1 = x0 + a["bbox"][2] + rng.integers(-2, 3) * q, y0 + a["bbox"][3] + rng.integers(-2, 3) * q
            else:
                x0, y0 = rng.integers(0, 40, 2) * q * 4
                x1, y1 = x0 + rng.integers(1, 30) * q * 2, y0 + rng.integers(1, 30) * q * 2
            boxes.append([x0, y0, max(x1, x0 + q), max(y1, y0 + q)])
        logits = (rng.integers(-40, 41, n_pr) / 8).astype(np.float32) if rng.random() < 0.8 else rng.normal(size=n_pr).astype(np.float32)
        return np.array(boxes, dtype=np.float32).reshape(-1, 4), logits

    for im in img_ids:
        mode = rng.integers(0, 5)                                # 0: GTs only, 1: proposals only, else both
        n_gt = 0 if mode == 1 else int(rng.integers(0, 13))
        n_pr = 0 if mode == 0 else int(rng.choice([rng.integers(0, 21), rng.integers(90, 161), rng.integers(1001, 1101)], p=[0.84, 0.14, 0.02]))
        if big and im == img_ids[0]:
            n_gt, n_pr = big
        mine = []
        for _ in range(n_gt):
            x, y = rng.integers(0, 40, 2) * q * 4
            w, h = rng.integers(1, 30, 2) * q * 2
            a = {"id": len(annos) + 1, "image_id": im, "category_id": int(rng.choice([1, 2, 9])), "bbox": [float(x), float(y), float(w), float(h)],
                 "iscrowd": int(rng.random() < 0.1), "area": float(w * h * rng.choice([1.0, 1.0, 0.3, 30.0]))}
            annos.append(a)
            mine.append(a)
        entries.append((im,) + proposals(mine, n_pr))
        if rng.random() < 0.15:                                  # the same image id once more, with other proposals
            entries.append((im,) + proposals(mine, int(rng.integers(0, 21))))
    gt = {"images": [{"id": i} for i in img_ids], "annotations": annos, "categories": [{"id": 1, "name": "ore"}, {"id": 2, "name": "gangue"}]}
    return gt, [entries[i] for i in rng.permutation(len(entries))]


def _run(ore, gt, entries, workspace=None):
    from detectron2.evaluation.coco_evaluation import AREA_RNG, PROPOSAL_LIMITS, CocoGT, proposal_iou_thrs
    g = CocoGT(gt)
    dev = torch.device("cuda")
    boxes = torch.from_numpy(np.concatenate([np.zeros((0, 4), np.float32)] + [e[1] for e in entries]).reshape(-1, 4)).to(dev)
    logits = torch.from_numpy(np.concatenate([np.zeros(0, np.float32)] + [e[2] for e in entries])).to(dev)
    out = ore.proposal_recall(boxes, logits, [len(e[2]) for e in entries], [g.img_index[e[0]] for e in entries], g.device_images(dev), g.img_off,
                              AREA_RNG, PROPOSAL_LIMITS, proposal_iou_thrs().numpy(), per_image=True, workspace=workspace)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check(gt, entries, got):
    from detectron2.evaluation.coco_evaluation import proposal_recalls
    ref = R.evaluate_all(gt, entries)
    assert got["status"][0] == 0
    off = got["entry_slot_off"]
    per_img = {}
    for a in gt["annotations"]:
        per_img[a["image_id"]] = per_img.get(a["image_id"], 0) + 1
    assert np.array_equal(np.diff(off), [per_img.get(e[0], 0) for e in entries])
    for c, (key, r) in enumerate(ref.items()):
        n = r["num_pos"]
        assert int(got["num_pos"][c]) == n, key
        assert got["gt_overlaps"][c, :n].tobytes() == r["gt_overlaps"].tobytes(), key
        assert (got["gt_overlaps"][c, n:].view(np.uint32) == 0xffffffff).all(), key
        assert np.array_equal(got["counts"][c], r["counts"]), key
        recalls, ar = proposal_recalls(torch.from_numpy(got["counts"][c]), int(got["num_pos"][c]))
        assert recalls.numpy().tobytes() == r["recalls"].tobytes() and ar.numpy().tobytes() == r["ar"].tobytes(), key
        for e, vec in enumerate(r["per_entry"]):
            k = int(got["entry_valid"][e, c])
            assert k == (0 if vec is None else len(vec)), (key, e)
            row = got["entry_overlaps"][c, off[e]:off[e + 1]]
            assert vec is None or row[:k].tobytes() == vec.tobytes(), (key, e)
            assert (row[k:].view(np.uint32) == 0xffffffff).all(), (key, e)
    return ref


@pytest.mark.parametrize("block", range(6))
def test_random_sets_bitwise(ore, block):
    """300 seeded random sets (50 per parametrised block)."""
    for seed in range(50 * block, 50 * block + 50):
        gt, entries = _dataset(seed)
        _check(gt, entries, _run(ore, gt, entries))


def test_random_sets_cover_the_paths():
    sets = [_dataset(seed) for seed in range(300)]
    counts = [len(e[2]) for _, es in sets for e in es]
    assert any(c == 0 for c in counts) and any(100 < c <= 1000 for c in counts) and any(c > 1000 for c in counts)
    assert any(len(es) > len({e[0] for e in es}) for _, es in sets)                             # one image id twice
    assert any(len(np.unique(e[2])) < len(e[2]) for _, es in sets for e in es)                  # tied logits
    assert any(a["category_id"] == 9 for gt, _ in sets for a in gt["annotations"]) and any(a["iscrowd"] for gt, _ in sets for a in gt["annotations"])


@pytest.mark.parametrize("big,n_entries", [((3000, 40), None), ((300, 1100), None), ((300, 1100), 1025)],
                         ids=["3000_gts_40_proposals", "300_gts_1100_proposals", "1025_entries"])
def test_past_the_lds_sizes_and_both_limits_bitwise(ore, big, n_entries):
    """The IoU matrix and the column state of that image live in the workspace; 1100 proposals are cut by both limits.  With 1025
    entries k_entry_scan walks two 1024-entry tiles, and the last entry -- the big image once more -- takes its slot and matrix
    offsets from the first tile's totals."""
    gt, entries = _dataset(4321, big=big)
    if n_entries:
        first = max(entries, key=lambda e: len(e[2]))
        small = min((e for e in entries if len(e[2]) > 0), key=lambda e: len(e[2]))
        entries = entries + [small] * (n_entries - 1 - len(entries)) + [first]
        assert len(entries) == n_entries and sum(a["image_id"] == first[0] for a in gt["annotations"]) == big[0]
    assert max(len(e[2]) for e in entries) >= big[1] and big[0] * min(big[1], 1000) > ore.lib().ore_proposal_recall_lds_cells()
    ref = _check(gt, entries, _run(ore, gt, entries))
    assert ref["AR@1000"]["num_pos"] >= 0.8 * big[0] and (ref["AR@1000"]["gt_overlaps"] > 0).any()


def test_recorded_set_equals_the_reference_bytes(ore):
    from detectron2.evaluation.coco_evaluation import proposal_recalls
    gt, entries, z = R.load_fixture(os.path.join(GOLDEN, "box_proposals_ref.npz"))
    got = _run(ore, gt, entries)
    assert got["status"][0] == 0
    for c in range(8):
        n = int(z["num_pos"][c])
        assert int(got["num_pos"][c]) == n
        assert got["gt_overlaps"][c, :n].tobytes() == z[f"gt_overlaps_{c}"].tobytes(), c
        recalls, ar = proposal_recalls(torch.from_numpy(got["counts"][c]), n)
        assert recalls.numpy().tobytes() == z["recalls"][c].tobytes() and ar.numpy().tobytes() == z["ar"][c].tobytes(), c


def test_deterministic_and_workspace_reuse(ore):
    big_gt, big_entries = _dataset(4321, big=(300, 1100))
    gt, entries = _dataset(77)
    a, b = _run(ore, gt, entries), _run(ore, gt, entries)
    for key in a:
        assert a[key].tobytes() == b[key].tobytes(), key
    ws = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")
    first = _run(ore, big_gt, big_entries, workspace=ws)
    again = _run(ore, gt, entries, workspace=ws)                 # a smaller call on the workspace the larger one used
    for key in a:
        assert a[key].tobytes() == again[key].tobytes(), key
    _check(big_gt, big_entries, first)
    _check(gt, entries, again)
    empty = _run(ore, gt, [])                                    # no entry at all
    assert (empty["num_pos"] == 0).all() and (empty["counts"] == 0).all() and empty["status"][0] == 0


def test_bad_sizes_are_refused(ore):
    from detectron2.evaluation.coco_evaluation import AREA_RNG, CocoGT, proposal_iou_thrs
    gt, entries = _dataset(77)
    g = CocoGT(gt)
    dev = torch.device("cuda")
    boxes = torch.zeros(3, 4, device=dev)
    logits = torch.zeros(3, device=dev)
    args = (boxes, logits, [3], [0], g.device_images(dev), g.img_off)
    thr = proposal_iou_thrs().numpy()
    with pytest.raises(ore.OreError):
        ore.proposal_recall(*args, AREA_RNG, [100, 5000], thr)                     # a limit past the row mask
    with pytest.raises(ore.OreError):
        ore.proposal_recall(*args, AREA_RNG, [10, 100, 1000], thr)                 # more than 8 chains
    with pytest.raises(ore.OreError):
        ore.proposal_recall(*args, AREA_RNG, [100], np.zeros(17, np.float32))      # more than 16 thresholds
    with pytest.raises(ore.OreError):
        ore.proposal_recall(boxes, logits, [2], [0], g.device_images(dev), g.img_off, AREA_RNG, [100], thr)   # counts do not add up
    assert ore.lib().ore_proposal_recall_workspace_bytes(1, 1, 1, 0, 4, 3) == 0


# ------------------------------------------------------------------ end to end

def _same_metrics(a, b):
    return list(a) == list(b) and all(x == y or (x != x and y != y) for x, y in zip(a.values(), b.values()))


def test_end_to_end_through_the_model_switch(ore, tmp_path, monkeypatch):
    from detectron2.evaluation import COCOEvaluator
    from detectron2.modeling.postprocessing import detector_postprocess
    from test_hip_coco_eval import _model, _setup_script
    m, cfg, name, gt = _setup_script(tmp_path, monkeypatch, False)
    model = _model(False)
    batches = list(m.Trainer.build_test_loader(cfg, name))
    assert 0 < len(batches) <= 8 and all(len(b) == 1 for b in batches)
    assert model.output_proposals is False
    ev = COCOEvaluator(name)
    ev.reset()
    off = []
    for b in batches:
        out = model(b)
        assert list(out[0]) == ["instances"]
        ev.process(b, out)
        off.append(out[0]["instances"])
    res_off = ev.evaluate()
    assert list(res_off) == ["bbox"]

    model.output_proposals = True
    out_dir = str(tmp_path / "with_proposals")
    ev = COCOEvaluator(name, output_dir=out_dir)
    ev.reset()
    entries, on = [], []
    for b, inst_off in zip(batches, off):
        out = model(b)
        assert list(out[0]) == ["instances", "proposals"]
        inst, prop = out[0]["instances"], out[0]["proposals"]
        assert inst.image_size == inst_off.image_size and torch.equal(inst.pred_boxes.tensor, inst_off.pred_boxes.tensor)
        assert torch.equal(inst.scores, inst_off.scores) and torch.equal(inst.pred_classes, inst_off.pred_classes)
        raw = model.inference_proposals(b)[0]
        want = detector_postprocess(raw, b[0].get("height", raw.image_size[0]), b[0].get("width", raw.image_size[1]))
        assert prop.image_size == want.image_size == inst.image_size and 0 < len(prop) <= 256
        assert torch.equal(prop.proposal_boxes.tensor, want.proposal_boxes.tensor) and torch.equal(prop.objectness_logits, want.objectness_logits)
        assert sorted(prop.get_fields()) == ["objectness_logits", "proposal_boxes"]
        ev.process(b, out)
        on.append(out[0])
        entries.append((b[0]["image_id"], prop.proposal_boxes.tensor.cpu().numpy(), prop.objectness_logits.cpu().numpy()))
    res_on = ev.evaluate()
    assert list(res_on) == ["box_proposals", "bbox"]
    assert _same_metrics(res_on["box_proposals"], R.box_proposals(gt, entries))
    assert any(v == v and v > 0 for v in res_on["box_proposals"].values())
    assert _same_metrics(res_on["bbox"], res_off["bbox"])
    assert os.path.exists(os.path.join(out_dir, "box_proposals.pkl"))

    many = model.inference_many([b[0] for b in batches])
    for one, got in zip(on, many):
        assert list(got) == ["instances", "proposals"]
        assert torch.equal(got["instances"].pred_boxes.tensor, one["instances"].pred_boxes.tensor)
        assert torch.equal(got["instances"].scores, one["instances"].scores)
        assert torch.equal(got["proposals"].proposal_boxes.tensor, one["proposals"].proposal_boxes.tensor)
        assert torch.equal(got["proposals"].objectness_logits, one["proposals"].objectness_logits)

    model.support_classes = "all"
    with pytest.raises(ValueError, match="support_classes"):
        model(batches[0])
    model.support_classes = None
    model.output_proposals = False
    out = model(batches[0])
    assert list(out[0]) == ["instances"] and torch.equal(out[0]["instances"].pred_boxes.tensor, off[0].pred_boxes.tensor)
