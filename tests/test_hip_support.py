"""GPU: support crops on the device (csrc/ore_support.hip) byte for byte against tests/support_ref.py (pure-Python geometry, Pillow's
pixels), and what is built on them: CenterNet2Detector.enrol / forget, detection with an enrolled class (one class and N-way), and
fewx.data.support.build_support_df writing the crop files that DatasetMapperWithSupport.generate_support reads back."""
import os

import numpy as np
import pytest
import torch

import support_ref as SR
from conftest import rel_err
from test_hip_resize import _cfg, _load, assert_same, ramp_image, random_image, raw_image

pytestmark = pytest.mark.gpu

S = SR.SIZE


@pytest.fixture(scope="module")
def ore():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import orehip
    orehip.lib()
    return orehip


def guarded_crops(ore_, frames, boxes, frame_index=None, **kw):
    """support_crops into the middle of a buffer of 0xA5 bytes; returns (crops, boxes) on the host and checks both guard bands."""
    K, band = len(boxes), 4096
    n = K * 3 * S * S
    buf = torch.full((n + 2 * band,), 0xA5, dtype=torch.uint8, device="cuda")
    out = buf[band:band + n].view(K, 3, S, S)
    got, sboxes = ore_.support_crops([torch.from_numpy(f) for f in frames], boxes, frame_index, out=out, **kw)
    assert got.data_ptr() == out.data_ptr() and sboxes.dtype == torch.float32 and not sboxes.is_cuda
    host = buf.cpu().numpy()
    assert (host[:band] == 0xA5).all() and (host[band + n:] == 0xA5).all(), "bytes outside the output were written"
    return host[band:band + n].reshape(K, 3, S, S), sboxes.numpy()


def assert_crops_equal(got, want, label):
    for k in range(len(want)):
        diff = int((got[k] != want[k]).sum())
        print(f"{label} job {k}: {diff} differing bytes")
    assert np.array_equal(got, want), label


def small_frame_boxes(h, w):
    """An interior small box (a window of 20 pixels: an upscale of 12), one box clipped at each corner, the whole frame (fill bands
    on two sides), and a 1 x 1 box."""
    return np.array([[w - 33, h - 27, w - 17, h - 13], [-4, -3, 9.5, 8.25], [w - 12.5, -6, w + 3, 11], [-2, h - 9, 14, h + 5],
                     [w - 10, h - 11.75, w + 8, h + 1], [0, 0, w, h], [w // 2, h // 2, w // 2 + 1, h // 2 + 1]], dtype=np.float32)


@pytest.mark.parametrize("hw", [(37, 53), (96, 128)], ids=lambda v: "%dx%d" % v)
@pytest.mark.parametrize("kind", ["random", "ramp"])
def test_crops_equal_reference(ore, hw, kind):
    h, w = hw
    frame = random_image(h, w) if kind == "random" else ramp_image(h, w)
    boxes = small_frame_boxes(h, w)
    g = SR.geometry(h, w, boxes[0])
    assert g["src"][2] - g["src"][0] == 20 and g["dst"] == (0, 0, S, S)           # the interior case is interior, and an upscale of 12
    assert all(ore.support_crop_form(h, w, b) == ore.RESIZE_FORM_LDS for b in boxes)
    want, wboxes = SR.crops([frame], boxes)
    got, gboxes = guarded_crops(ore, [frame], boxes)
    assert_crops_equal(got, want, f"{h}x{w} {kind}")
    assert np.array_equal(gboxes, wboxes)


@pytest.fixture(scope="module")
def big_frame():
    return random_image(1300, 1300)


def test_large_box_takes_the_workspace_form(ore, big_frame):
    box = np.array([[50, 50, 1250, 1250]], dtype=np.float32)
    assert ore.support_crop_form(1300, 1300, box[0]) == ore.RESIZE_FORM_WORKSPACE
    want, wboxes = SR.crops([big_frame], box)
    got, gboxes = guarded_crops(ore, [big_frame], box)
    assert_crops_equal(got, want, "1300x1300 box 1200")
    assert np.array_equal(gboxes, wboxes)


def test_mixed_forms_two_frames_custom_fill(ore, big_frame):
    """K = 7 jobs of both forms from two frames of different sizes in one call, fill (7, 200, 91)."""
    small = ramp_image(211, 317)
    frames = [small, big_frame]
    fi = [0, 1, 0, 1, 1, 0, 1]
    boxes = np.array([[100, 80, 140, 130], [0, 0, 1300, 1300], [-10, 150, 60, 230], [600, 640, 660, 700], [100, 200, 1290, 1100],
                      [0, 0, 317, 211], [1250.5, 3, 1299, 40.25]], dtype=np.float32)
    forms = [ore.support_crop_form(*frames[f].shape[:2], b) for f, b in zip(fi, boxes)]
    assert set(forms) == {ore.RESIZE_FORM_LDS, ore.RESIZE_FORM_WORKSPACE} and forms[1] == forms[4] == ore.RESIZE_FORM_WORKSPACE
    fill = (7, 200, 91)
    want, wboxes = SR.crops(frames, boxes, fi, fill=fill)
    got, gboxes = guarded_crops(ore, frames, boxes, fi, fill=fill)
    assert_crops_equal(got, want, "mixed")
    assert np.array_equal(gboxes, wboxes)
    with pytest.raises(ValueError, match="box 2"):
        ore.support_crops([torch.from_numpy(small)], np.array([[1, 1, 9, 9], [5, 5, 30, 30], [400, 10, 420, 30]], dtype=np.float32))


def test_back_to_back_calls_do_not_share_a_plan(ore):
    """Calls issued one after another with no synchronise between them, each with other boxes: every call's crops are its own (a
    pinned job buffer is not rewritten under an upload that has not run yet), and the host is not made to wait in between."""
    frame = random_image(96, 128)
    dev = torch.from_numpy(frame).cuda()
    rng = np.random.default_rng(3)
    sets = []
    for _ in range(6):
        x, y = rng.uniform(0, 100, 3), rng.uniform(0, 70, 3)
        sets.append(np.stack([x, y, x + rng.uniform(4, 40, 3), y + rng.uniform(4, 40, 3)], 1).astype(np.float32))
    torch.cuda.synchronize()
    got = [ore.support_crops(dev, b) for b in sets]
    torch.cuda.synchronize()
    for (crops, sboxes), b in zip(got, sets):
        want, wboxes = SR.crops([frame], b)
        assert np.array_equal(crops.cpu().numpy(), want) and np.array_equal(sboxes.numpy(), wboxes)


# ------------------------------------------------------------------------------------------------ enrolment
FRAME_HW = (300, 420)
ENROL_BOXES = np.array([[30, 40, 110, 100], [200.5, 150.25, 260, 222], [350, 20, 419, 90], [5, 220, 70, 299], [150, 60, 190, 95]], dtype=np.float32)


@pytest.fixture(scope="module")
def frame():
    return raw_image(123, *FRAME_HW)


def fresh_model(seed=0):
    """A randomly initialised detector (fixed seed), eval mode."""
    from detectron2.modeling import build_model
    cfg = _cfg()
    cfg.freeze()
    torch.manual_seed(seed)
    return build_model(cfg).eval()


@pytest.fixture(scope="module")
def rand_model(ore):
    return fresh_model()


def test_enrol_equals_compute_support_dict_on_reference_crops(ore, rand_model, frame):
    m = rand_model
    want_crops, want_boxes = SR.crops([frame], ENROL_BOXES)
    want = m.compute_support_dict(torch.from_numpy(want_crops), torch.from_numpy(want_boxes), cls_id=3, merge=False)
    m.support_dict = None
    crops, sboxes = m.enrol(frame, ENROL_BOXES, cls_id=3)
    assert crops.is_cuda and np.array_equal(crops.cpu().numpy(), want_crops) and np.array_equal(sboxes.numpy(), want_boxes)
    assert set(m.support_dict) == set(want) == {"p3", "p4", "p5", "rcnn_8", "rcnn_4"}
    for k in want:
        assert list(m.support_dict[k]) == [3]
        assert torch.equal(m.support_dict[k][3].cpu(), want[k][3]), k


def test_enrol_append_equals_one_call_and_forget(ore, rand_model, frame):
    m = rand_model
    m.support_dict = None
    m.enrol(frame, ENROL_BOXES, cls_id=3)
    one = {k: v[3].cpu() for k, v in m.support_dict.items()}
    m.enrol(frame, ENROL_BOXES[:2], cls_id=3)
    assert m.support_dict["rcnn_8"][3].shape[0] == 2
    m.enrol(frame, ENROL_BOXES[2:], cls_id=3, replace=False)
    two = {k: v[3].cpu() for k, v in m.support_dict.items()}
    for k in ("rcnn_8", "rcnn_4"):
        assert two[k].shape[0] == 5
        print(k, "max abs difference", float((two[k] - one[k]).abs().max()))
        assert torch.equal(two[k], one[k]), k
    for k in ("p3", "p4", "p5"):
        err = rel_err(two[k].numpy(), one[k].numpy())
        print(k, "rel err", err)
        assert err < 1e-4, (k, err)
    # a class installed another way has no per-shot prototypes to add to
    m.set_support_dict({k: {3: v[3], 4: v[3]} for k, v in m.support_dict.items()})
    with pytest.raises(ValueError, match="replace=True"):
        m.enrol(frame, ENROL_BOXES[:1], cls_id=4, replace=False)
    # forget
    with pytest.raises(KeyError):
        m.forget(9)
    m.forget(4)
    assert all(list(v) == [3] for v in m.support_dict.values()) and m._engine_key is None
    m.forget(3)
    assert m.support_dict is None
    with pytest.raises(KeyError):
        m.forget(3)


@pytest.fixture(scope="module")
def det_models(ore):
    """Two detectors with the same synthetic state (the one of tests/test_hip_resize.py)."""
    from detectron2.modeling import build_model
    cfg = _cfg()
    cfg.freeze()
    return _load(build_model(cfg)), _load(build_model(cfg))


def test_detection_after_enrol_equals_installed_dict(ore, det_models, frame):
    a, b = det_models
    a.support_dict = None
    a.enrol(frame, ENROL_BOXES, cls_id=3)
    b.set_support_dict({k: {c: t.clone() for c, t in v.items()} for k, v in a.support_dict.items()})
    req = {"image_raw": raw_image(7, 360, 480)}
    got, want = a([req])[0], b([req])[0]
    print("detections:", len(want["instances"]))
    assert_same(got, want, need=1)                               # equal, and not for want of detections


def test_nway_sees_enrolled_classes(ore, det_models, frame):
    """support_classes = "all": two enrolled classes are detected with no further call, and equal the N-way path fed the same dict."""
    a, b = det_models
    a.support_dict = None
    a.support_classes = b.support_classes = "all"
    try:
        a.enrol(frame, ENROL_BOXES[:3], cls_id=3)
        req = {"image_raw": raw_image(8, 360, 480)}
        first = a([req])[0]
        assert set(first["instances"].pred_classes.tolist()) == {3}          # detections exist, all of the one enrolled class
        a.enrol(frame, ENROL_BOXES[3:], cls_id=8)                  # picked up by the next forward
        assert a._support_selection() == (3, 8)
        b.set_support_dict({k: {c: t.clone() for c, t in v.items()} for k, v in a.support_dict.items()})
        got, want = a([req])[0], b([req])[0]
        print("detections:", len(want["instances"]), "classes:", sorted(set(want["instances"].pred_classes.tolist())))
        assert_same(got, want, need=2)
        assert set(want["instances"].pred_classes.tolist()) == {3, 8}             # both enrolled classes are detected
        a.forget(3)
        assert a._support_selection() == (8,)
    finally:
        a.support_classes = b.support_classes = None


# ------------------------------------------------------------------------------------------------ the dataset-level builder
def test_build_support_df_writes_crops_the_mapper_reads_back(ore, tmp_path):
    from PIL import Image
    from fewx.data.dataset_mapper import DatasetMapperWithSupport
    from fewx.data.support import build_support_df
    frames = {f"{i}.png": raw_image(40 + i, 120 + 10 * i, 160) for i in range(5)}

    def ann(i, cat, x, y, bw, bh):
        return {"id": i, "category_id": cat, "bbox": [x, y, bw, bh], "bbox_mode": 1, "iscrowd": 0}
    recs = [{"file_name": f"{i}.png", "image_id": i, "height": 120 + 10 * i, "width": 160,
             "annotations": [ann(10 * i, 0, 10 + i, 20, 40, 30 + i), ann(10 * i + 1, 1, 90.5, 50.25 - i, 60, 45)][:1 if i == 2 else 2]}
            for i in range(5)]                                  # image 2, the query's, holds class 0 only
    root = str(tmp_path)

    def reader(path, format="BGR"):
        if path in frames:
            return frames[path]
        assert path.startswith(DatasetMapperWithSupport.SUPPORT_DIR), path
        rgb = np.asarray(Image.open(os.path.join(root, path[len(DatasetMapperWithSupport.SUPPORT_DIR):])).convert("RGB"))
        return np.ascontiguousarray(rgb[:, :, ::-1] if format == "BGR" else rgb)
    cfg = _cfg(["INPUT.FS.SUPPORT_WAY", 2, "INPUT.FS.SUPPORT_SHOT", 2])
    df = build_support_df(recs, image_root=root, read_image=reader, format=cfg.INPUT.FORMAT)
    assert len(df) == 9 and sorted(os.listdir(os.path.join(root, "support"))) == ["0", "1"]
    want = {}
    for r in recs:
        for a in r["annotations"]:
            x, y, bw, bh = a["bbox"]
            want[a["id"]] = SR.crop(frames[r["file_name"]], np.array([x, y, x + bw, y + bh], dtype=np.float32))
    for _, row in df.iterrows():
        crop = reader(DatasetMapperWithSupport.SUPPORT_DIR + row["file_path"], cfg.INPUT.FORMAT).transpose(2, 0, 1)
        assert np.array_equal(crop, want[row["id"]][0]) and np.array_equal(row["support_box"], want[row["id"]][1]), row["id"]
    mp = DatasetMapperWithSupport(cfg, is_train=True, support_df=df, read_image=reader)
    data, boxes, flags = mp.generate_support({"annotations": [{"id": 20}]})
    assert data.shape == (4, 3, S, S) and flags == [0, 0, 1, 1]
    ids = []
    for k in range(4):                                          # each drawn crop is one of the written ones, bytes and box
        hit = [i for i, (c, b) in want.items() if np.array_equal(data[k], c.astype(np.float32)) and np.array_equal(boxes[k], b)]
        assert len(hit) == 1, k
        ids.append(hit[0])
    assert all(i % 10 == 0 and i != 20 for i in ids[:2]) and all(i % 10 == 1 and i != 21 for i in ids[2:]) and len(set(ids)) == 4


def test_enrol_from_records_equals_enrol_per_category(ore, rand_model):
    """fewx.data.support.enrol_from_records (what demo.py --support-json runs): every category enrolled from its annotated frames,
    equal to one enrol call per category with the frames and boxes listed by hand."""
    from fewx.data.support import enrol_from_records
    frames = {f"{i}.png": raw_image(60 + i, 100 + 20 * i, 150) for i in range(3)}
    recs = [{"file_name": f"{i}.png", "image_id": i, "height": 100 + 20 * i, "width": 150,
             "annotations": [{"id": 10 * i, "category_id": 2, "bbox": [10, 15 + i, 50, 40], "bbox_mode": 1, "iscrowd": 0},
                             {"id": 10 * i + 1, "category_id": 5, "bbox": [80.5, 30, 60, 55.5], "bbox_mode": 1, "iscrowd": 0}]} for i in range(3)]
    m = rand_model
    m.support_dict = None
    assert enrol_from_records(m, recs, shot=2, read_image=lambda path, format="BGR": frames[path]) == {2: 2, 5: 2}
    got = {k: {c: t.cpu() for c, t in v.items()} for k, v in m.support_dict.items()}
    m.support_dict = None
    fl = [frames["0.png"], frames["1.png"]]
    m.enrol(fl, np.array([[10, 15, 60, 55], [10, 16, 60, 56]], dtype=np.float32), cls_id=2, frame_index=[0, 1])
    m.enrol(fl, np.array([[80.5, 30, 140.5, 85.5]] * 2, dtype=np.float32), cls_id=5, frame_index=[0, 1])
    for k, v in m.support_dict.items():
        assert list(v) == [2, 5] == list(got[k])
        for c in v:
            assert torch.equal(v[c].cpu(), got[k][c]), (k, c)
    m.support_dict = None
