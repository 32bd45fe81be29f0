"""CPU: the support-crop planner (csrc/ore_support_plan.cpp, orehip.support_crop_plan) against the pure-Python geometry and numpy
float32 box of tests/support_ref.py, its tables against orehip.resize_plan, the form function, and the dataset-level selection of
fewx.data.support.build_support_df(write=False).  No GPU."""
import numpy as np
import pytest

import support_ref as SR


@pytest.fixture(scope="module")
def ore():
    import orehip
    if not __import__("os").path.exists(orehip.LIB_PATH):
        orehip.build()
    orehip.lib()
    return orehip


# (h, w, box) -> D, origin, source rectangle, destination rectangle, support box: the worked cases of the contract
WORKED = [
    ((100, 120), (30.5, 40.25, 60, 55.5), 36, (27, 30), (27, 30, 63, 66), (0, 0, 240, 240), (23.333332, 68.33333, 220.0, 170.0)),
    ((100, 120), (0, 0, 10, 100), 116, (-53, -8), (0, 0, 63, 100), (110, 17, 240, 223), (110.0, 17.0, 130.63492, 223.0)),
    ((480, 640), (0, 0, 640, 480), 740, None, None, (16, 42, 224, 198), None),
]


def check(ore, h, w, box):
    got = ore.support_crop_plan(h, w, box)
    want = SR.geometry(h, w, box)
    assert {k: got[k] for k in want} == want, (h, w, box, got, want)
    wbox = SR.support_box(box, want)
    assert got["box"].dtype == np.float32 and np.array_equal(got["box"], wbox), (h, w, box, got["box"], wbox)
    return got


@pytest.mark.parametrize("case", WORKED, ids=["interior", "left-edge", "whole-frame"])
def test_worked_cases(ore, case):
    (h, w), box, D, origin, src, dst, sbox = case
    got = check(ore, h, w, box)
    assert got["D"] == D and got["dst"] == dst
    if origin is not None:
        assert got["origin"] == origin and got["src"] == src
    if sbox is not None:
        assert np.array_equal(got["box"], np.asarray(sbox, dtype=np.float32))
    # the reference itself reproduces the table (so the table pins both)
    assert SR.geometry(h, w, box)["D"] == D and SR.geometry(h, w, box)["dst"] == dst


def test_corners_tiny_and_overhanging_boxes(ore):
    h, w = 97, 131
    for box in [(0, 0, 20, 14), (w - 20, 0, w, 14), (0, h - 14, 20, h), (w - 20, h - 14, w, h),           # at each corner
                (50, 40, 51, 41), (50.2, 40.7, 50.4, 40.9), (0, 0, 1, 1), (w - 1, h - 1, w, h),            # 1 x 1
                (-30.5, -12.25, 40, 33), (100, 70, 400.5, 300), (-50, 20, 500, 60), (-5, -5, w + 5, h + 5)]:   # overhanging
        g = check(ore, h, w, box)
        (dx0, dy0, dx1, dy1), (rx0, ry0, rx1, ry1) = g["dst"], g["src"]
        assert 0 <= dx0 < dx1 <= 240 and 0 <= dy0 < dy1 <= 240 and 0 <= rx0 < rx1 <= w and 0 <= ry0 < ry1 <= h
        assert (g["box"] >= 0).all() and (g["box"] <= 240).all()


def test_random_cases(ore):
    rng = np.random.default_rng(20240)
    for _ in range(2000):
        h, w = int(rng.integers(8, 2200)), int(rng.integers(8, 3900))
        bw, bh = rng.uniform(1, w), rng.uniform(1, h)
        cx, cy = rng.uniform(0, w), rng.uniform(0, h)
        box = np.array([cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2], dtype=np.float32)
        try:
            SR.geometry(h, w, box)
        except ValueError:                                   # a sliver that rounds out of the frame: refused by both
            with pytest.raises(ValueError):
                ore.support_crop_plan(h, w, box)
            continue
        check(ore, h, w, box)


def test_box_outside_the_frame_is_refused(ore):
    for box in [(130, 10, 150, 30), (-40, 10, -2, 30), (10, 100, 30, 140), (10, -9, 30, -0.5), (30, 30, 30, 50)]:
        with pytest.raises(ValueError):
            SR.geometry(100, 120, box)
        with pytest.raises(ValueError, match="outside"):
            ore.support_crop_plan(100, 120, box)
        with pytest.raises(ValueError):
            ore.support_crop_form(100, 120, box)


def test_tables_are_the_resize_planner_s(ore):
    """The job's tables are orehip.resize_plan of (source side, destination side), integer for integer: one coefficient source."""
    for (h, w), box in [((100, 120), (30.5, 40.25, 60, 55.5)), ((100, 120), (0, 0, 10, 100)), ((480, 640), (0, 0, 640, 480)),
                        ((1300, 1300), (50, 50, 1250, 1250)), ((37, 53), (20, 11, 21, 12)), ((1080, 1920), (900, 500, 1000, 540))]:
        g = ore.support_crop_plan(h, w, box)
        (rx0, ry0, rx1, ry1), (dx0, dy0, dx1, dy1) = g["src"], g["dst"]
        xb, kx = ore.resize_plan(rx1 - rx0, dx1 - dx0)
        yb, ky = ore.resize_plan(ry1 - ry0, dy1 - dy0)
        assert np.array_equal(g["x_bounds"], xb) and np.array_equal(g["x_coeffs"], kx)
        assert np.array_equal(g["y_bounds"], yb) and np.array_equal(g["y_coeffs"], ky)


def test_form(ore):
    """A small box is served by the one-launch LDS form, the whole-frame job of a 1300 x 1300 frame (a reduction of about 6) goes through
    the workspace; the threshold is the form function's own: the same sizing ore_resize_form applies to a whole-image resize, which
    agrees wherever the destination rectangle starts on a tile boundary of the canvas."""
    small = ore.support_crop_plan(1080, 1920, (900, 500, 1000, 540))
    assert small["form"] == ore.RESIZE_FORM_LDS == ore.support_crop_form(1080, 1920, (900, 500, 1000, 540)) and small["workspace_bytes"] == 0
    big = ore.support_crop_plan(1300, 1300, (0, 0, 1300, 1300))
    assert big["form"] == ore.RESIZE_FORM_WORKSPACE == ore.support_crop_form(1300, 1300, (0, 0, 1300, 1300))
    (rx0, ry0, rx1, ry1), (dx0, dy0, dx1, dy1) = big["src"], big["dst"]
    assert big["workspace_bytes"] >= (ry1 - ry0) * (dx1 - dx0) * 3
    # a job whose destination rectangle is the whole canvas is tiled exactly as a whole-image resize: the two form functions agree
    for (h, w), box in [((100, 120), (30.5, 40.25, 60, 55.5)), ((3000, 3000), (600, 600, 2400, 2400))]:
        g = ore.support_crop_plan(h, w, box)
        assert g["dst"] == (0, 0, 240, 240)
        sw, sh = g["src"][2] - g["src"][0], g["src"][3] - g["src"][1]
        assert g["form"] == ore.resize_form(sh, sw, 240, 240)
    assert ore.support_crop_plan(3000, 3000, (600, 600, 2400, 2400))["form"] == ore.RESIZE_FORM_WORKSPACE


# ------------------------------------------------------------------------------------------------ the dataset-level builder
def records():
    """Four images, three categories; annotation ids deliberately out of order inside an image."""
    def ann(i, cat, box, crowd=0):
        return {"id": i, "category_id": cat, "bbox": list(box), "bbox_mode": 1, "iscrowd": crowd}
    return [
        {"file_name": "b.png", "image_id": 2, "height": 100, "width": 120,
         "annotations": [ann(21, 0, (10, 10, 30, 20)), ann(20, 1, (50, 40, 20, 20)), ann(22, 0, (60, 5, 8, 8))]},
        {"file_name": "a.png", "image_id": 1, "height": 80, "width": 90,
         "annotations": [ann(11, 0, (5, 5, 40, 30)), ann(10, 0, (20, 30, 2, 2)), ann(12, 1, (0, 0, 90, 80), crowd=1), ann(13, 2, (70, 60, 15, 15))]},
        {"file_name": "c.png", "image_id": 3, "height": 60, "width": 60,
         "annotations": [ann(30, 0, (1, 1, 50, 50)), ann(31, 1, (10, 10, 3, 30)), ann(32, 2, (20, 20, 10, 10))]},
        {"file_name": "d.png", "image_id": 4, "height": 60, "width": 60, "annotations": [ann(40, 0, (5, 5, 20, 20)), ann(41, 1, (30, 30, 20, 20))]},
    ]


def test_build_support_df_from_the_plan_alone(ore, tmp_path):
    from fewx.data.support import build_support_df
    recs = records()
    df = build_support_df(recs, write=False, image_root=str(tmp_path))
    assert list(df.columns) == ["id", "image_id", "category_id", "file_path", "support_box"]
    assert not any(tmp_path.iterdir()), "write=False wrote files"
    # every eligible annotation, category by category, (image id, annotation id) order inside; the crowd annotation 12 is skipped
    assert df["id"].tolist() == [10, 11, 21, 22, 30, 40, 20, 31, 41, 13, 32]
    assert df["category_id"].value_counts().to_dict() == {0: 6, 1: 3, 2: 2}
    assert df.loc[df["id"] == 21, "file_path"].item() == "support/0/21.png" and df.loc[df["id"] == 21, "image_id"].item() == 2
    by_id = {a["id"]: (r, a) for r in recs for a in r["annotations"]}
    for _, row in df.iterrows():
        r, a = by_id[row["id"]]
        x, y, bw, bh = a["bbox"]
        box = np.array([x, y, x + bw, y + bh], dtype=np.float32)
        assert np.array_equal(row["support_box"], SR.support_box(box, SR.geometry(r["height"], r["width"], box)))
    # the first `shot` per category under seed=None
    assert build_support_df(recs, shot=2, write=False)["id"].tolist() == [10, 11, 20, 31, 13, 32]
    # a seed: reproducible, `shot` per category drawn from the eligible ones, and not simply the first ones for every seed
    a, b = build_support_df(recs, shot=2, seed=5, write=False), build_support_df(recs, shot=2, seed=5, write=False)
    assert a["id"].tolist() == b["id"].tolist() and a["category_id"].value_counts().to_dict() == {0: 2, 1: 2, 2: 2}
    assert set(a["id"]) <= {10, 11, 21, 22, 30, 40, 20, 31, 41, 13, 32}
    rng = np.random.default_rng(5)
    want = [[10, 11, 21, 22, 30, 40][i] for i in rng.permutation(6)[:2]] + [[20, 31, 41][i] for i in rng.permutation(3)[:2]] + \
           [[13, 32][i] for i in rng.permutation(2)[:2]]
    assert a["id"].tolist() == want
    assert any(build_support_df(recs, shot=2, seed=s, write=False)["id"].tolist() != [10, 11, 20, 31, 13, 32] for s in range(4))
    # one annotation per (image, category): 11 (after 10 in image 1) and 22 (after 21 in image 2) go
    assert build_support_df(recs, one_per_image=True, write=False)["id"].tolist() == [10, 21, 30, 40, 20, 31, 41, 13, 32]
    # min_side: 10 (2 x 2) goes at 3, 31 (3 x 30) stays; at 4 it goes too
    assert build_support_df(recs, min_side=3, write=False)["id"].tolist() == [11, 21, 22, 30, 40, 20, 31, 41, 13, 32]
    assert build_support_df(recs, min_side=4, write=False)["id"].tolist() == [11, 21, 22, 30, 40, 20, 41, 13, 32]


def test_demo_support_flags():
    """demo.py --support-json / --support-root / --shots: parsed, and refused on the host where they do not go together."""
    import demo
    args = demo.get_parser().parse_args(["--input", "a.jpg", "--output", "o", "--support-json", "ann.json", "--support-root", "imgs", "--shots", "5"])
    assert (args.support_json, args.support_root, args.shots) == ("ann.json", "imgs", 5)
    none = demo.get_parser().parse_args(["--input", "a.jpg", "--output", "o"])
    assert none.support_json is None and none.support_root is None and none.shots is None
    for argv in (["--support-json", "ann.json"], ["--support-root", "imgs"], ["--shots", "3"],
                 ["--support-json", "ann.json", "--support-root", "imgs", "--shots", "0"]):
        with pytest.raises(SystemExit) as e:
            demo.main(["--input", "a.jpg", "--output", "o"] + argv)
        assert "--support" in str(e.value.code) or "--shots" in str(e.value.code)


def test_support_json_path_from_a_coco_file(ore, tmp_path):
    """What demo.py --support-json runs, up to the model: a COCO json on disk -> load_coco_json -> the selection, the planned
    dataframe, and enrol_support's enrol calls (frames read from image files, boxes XYXY, frame indices) on a recording stand-in."""
    import json
    import types
    from PIL import Image
    import demo
    from fewx.data.datasets.register_coco import load_coco_json
    from fewx.data.support import build_support_df, select_support_annotations
    imgs = {1: (60, 80), 2: (50, 70)}
    pix = {i: np.random.default_rng(i).integers(0, 256, (h, w, 3), dtype=np.uint8) for i, (h, w) in imgs.items()}
    (tmp_path / "img").mkdir()
    for i, a in pix.items():
        Image.fromarray(a).save(tmp_path / "img" / f"{i}.png")
    js = {"images": [{"id": i, "file_name": f"{i}.png", "height": h, "width": w} for i, (h, w) in imgs.items()],
          "categories": [{"id": 7, "name": "ore"}, {"id": 9, "name": "gangue"}],
          "annotations": [{"id": 5, "image_id": 2, "category_id": 7, "bbox": [10, 5, 20, 30], "iscrowd": 0, "area": 600},
                          {"id": 3, "image_id": 1, "category_id": 7, "bbox": [4.5, 6, 30, 20], "iscrowd": 0, "area": 600},
                          {"id": 4, "image_id": 1, "category_id": 9, "bbox": [40, 30, 25, 25], "iscrowd": 0, "area": 625},
                          {"id": 6, "image_id": 2, "category_id": 9, "bbox": [0, 0, 70, 50], "iscrowd": 1, "area": 3500}]}
    f = tmp_path / "ann.json"
    f.write_text(json.dumps(js))
    recs = load_coco_json(str(f), str(tmp_path / "img"), extra_annotation_keys=["id"])
    assert [(a["id"], a["category_id"]) for _, a, _ in select_support_annotations(recs)] == [(3, 0), (5, 0), (4, 1)]
    df = build_support_df(recs, write=False)
    assert df["id"].tolist() == [3, 5, 4] and df["file_path"].tolist() == ["support/0/3.png", "support/0/5.png", "support/1/4.png"]
    assert np.array_equal(df["support_box"][0], SR.support_box((4.5, 6, 34.5, 26), SR.geometry(60, 80, (4.5, 6, 34.5, 26))))
    calls = []
    model = types.SimpleNamespace(input_format="BGR", support_classes=None,
                                  enrol=lambda frames, boxes, cls_id, frame_index: calls.append((frames, boxes, cls_id, frame_index)))
    args = demo.get_parser().parse_args(["--input", "a.jpg", "--output", "o", "--support-json", str(f), "--support-root", str(tmp_path / "img")])
    demo.enrol_support(model, args, __import__("logging").getLogger("test"))
    assert model.support_classes == "all" and [c[2] for c in calls] == [0, 1]
    frames, boxes, _, fi = calls[0]
    assert fi == [0, 1] and np.array_equal(boxes, np.array([[4.5, 6, 34.5, 26], [10, 5, 30, 35]], dtype=np.float32))
    assert np.array_equal(frames[0], pix[1][:, :, ::-1]) and np.array_equal(frames[1], pix[2][:, :, ::-1])        # read as BGR
    assert calls[1][3] == [0] and np.array_equal(calls[1][1], np.array([[40, 30, 65, 55]], dtype=np.float32))
    # --shots 1: the first annotation of each category
    calls.clear()
    args.shots = 1
    demo.enrol_support(model, args, __import__("logging").getLogger("test"))
    assert [(c[2], len(c[1])) for c in calls] == [(0, 1), (1, 1)]
