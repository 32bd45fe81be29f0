"""GPU: every launch form of the second stage's tail against its C twin, bit for bit (tests/roitail_ref.py holds the reference and the
case table, tests/test_roitail_host.py what the table can see).

Every case goes through the C ABI -- ore_roi_predict_fwd, ore_roi_predict_post_fwd or, for the engine's K-split form,
ore_roi_predict_parts_fwd -- and is launched twice into outputs filled with NaN / sentinels and a workspace filled with 0xFF bytes;
the two results must be equal, equal to the twin's, and every row at and beyond a count must keep its fill.  Then the NMS entry
points behind the general path (ore_nms_device_n_fwd) and the row-major scan of ore_nms_fwd (n > 3072) against oracle_nms."""
import ctypes as C

import numpy as np
import pytest
import torch

import roitail_ref as RT
from oracle import decode as odec

pytestmark = pytest.mark.gpu

SENT = -7
REC_FILL = 0xA5
RAN = set()


@pytest.fixture(scope="module")
def L():
    import orehip
    return orehip.lib()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stream():
    import orehip
    return orehip._stream()


class Launch:
    """Device inputs and sentinel-filled outputs of one case."""

    def __init__(self, L, c, cap=None, C_=None, parts=None, post=None, outs=True, ws=True):
        cap, Cc = c.cap if cap is None else cap, c.C if C_ is None else C_
        self.c, self.cap, self.Cc, self.L = c, cap, Cc, L
        self.parts = c.parts if parts is None else parts
        self.h = _dev(c.h) if C_ is None and cap == c.cap and self.parts == c.parts else torch.zeros(max(self.parts, 1) * cap * Cc, device="cuda")
        self.bias = _dev(c.bias) if c.bias is not None and C_ is None else None
        if C_ is None:
            self.w = [_dev(a) for a in (c.cls_w, c.cls_b, c.box_w, c.box_b)]
        else:
            self.w = [torch.zeros(2 * Cc, device="cuda"), torch.zeros(2, device="cuda"), torch.zeros(4 * Cc, device="cuda"), torch.zeros(4, device="cuda")]
        self.boxes = _dev(c.boxes) if cap == c.cap else torch.zeros(cap, 4, device="cuda")
        self.n_dev = torch.tensor([c.n], dtype=torch.int32, device="cuda") if c.n_on_device else None
        post = c.post if post is None else post
        self.post = _dev(np.asarray(post, np.float32)) if post is not None else None
        self.has_fin = self.post is not None and outs
        self.wsb = L.ore_roi_predict_workspace_bytes(cap)
        self.ws = torch.empty(self.wsb, dtype=torch.uint8, device="cuda")
        self.ws_bytes = self.wsb if ws else self.wsb - 1
        self.rw = (C.c_float * 4)(*RT.REG_W)
        self.fill()

    def fill(self):
        cap = self.cap
        nan = float("nan")
        self.det_boxes = torch.full((cap, 4), nan, device="cuda")
        self.det_scores = torch.full((cap,), nan, device="cuda")
        self.det_src = torch.full((cap,), SENT, dtype=torch.int64, device="cuda")
        self.det_count = torch.full((4,), SENT, dtype=torch.int32, device="cuda")
        self.fin_boxes = torch.full((cap, 4), nan, device="cuda")
        self.fin_scores = torch.full((cap,), nan, device="cuda")
        self.fin_count = torch.full((4,), SENT, dtype=torch.int32, device="cuda")
        self.ws.fill_(0xFF)
        self.rec = self.pin = None
        if self.c.record != "none":
            self.pin = torch.full((4,), SENT, dtype=torch.int32, device="cuda")
            addr = 0
            if self.c.record == "rec":
                self.rec = torch.full((cap * 28,), REC_FILL, dtype=torch.uint8, device="cuda")
                addr = self.rec.data_ptr()
            self.pin[2:4] = torch.from_numpy(np.array([addr], np.uint64).view(np.int32).copy()).cuda()
        torch.cuda.synchronize()

    def run(self):
        c, p = self.c, (lambda t: None if t is None else t.data_ptr())
        head = (p(self.h), self.Cc, p(self.w[0]), p(self.w[1]), p(self.w[2]), p(self.w[3]), p(self.boxes), p(self.n_dev), c.n, self.cap, self.rw,
                c.img[0], c.img[1], c.score_thresh, c.nms_thresh, c.topk, p(self.det_boxes), p(self.det_scores), p(self.det_src), p(self.det_count))
        fin = (p(self.post), p(self.fin_boxes) if self.has_fin else None, p(self.fin_scores) if self.has_fin else None,
               p(self.fin_count) if self.has_fin else None, p(self.pin))
        tail = (p(self.ws), self.ws_bytes, _stream())
        if self.parts >= 1:
            rc = self.L.ore_roi_predict_parts_fwd(*head, *fin, *tail, self.parts, p(self.bias))
        elif self.post is not None or self.pin is not None:
            rc = self.L.ore_roi_predict_post_fwd(*head, *fin, *tail)
        else:
            rc = self.L.ore_roi_predict_fwd(*head, *tail)
        torch.cuda.synchronize()
        return rc

    def result(self):
        o = {k: getattr(self, k).cpu().numpy() for k in ("det_boxes", "det_scores", "det_src", "det_count", "fin_boxes", "fin_scores", "fin_count")}
        o["pin"] = None if self.pin is None else self.pin.cpu().numpy()[:2]      # words 2..3 hold this launch's record address
        o["rec"] = None if self.rec is None else self.rec.cpu().numpy()
        return o


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _untouched(o, L_):
    nanb = np.float32("nan").view(np.uint32)
    assert np.all(_bits(o["fin_boxes"]) == nanb) and np.all(_bits(o["fin_scores"]) == nanb) and np.all(o["fin_count"] == SENT)


@pytest.mark.parametrize("name", RT.case_names())
def test_case_vs_twin(L, name):
    c = RT.case(name)
    exp = RT.expected(c)
    la = Launch(L, c)
    assert la.run() == 0, L.ore_last_error()
    first = la.result()
    la.fill()
    assert la.run() == 0, L.ore_last_error()
    o = la.result()
    for k, v in first.items():
        assert (v is None and o[k] is None) or _same_bits(v, o[k]), (name, k, "two launches differ")
    nanb = np.float32("nan").view(np.uint32)
    k = len(exp["scores"])
    assert o["det_count"].tolist() == [k, SENT, SENT, SENT], (name, o["det_count"], k)
    assert _same_bits(o["det_boxes"][:k], exp["boxes"]) and _same_bits(o["det_scores"][:k], exp["scores"]), name
    assert np.array_equal(o["det_src"][:k], exp["src"]), name
    assert np.all(_bits(o["det_boxes"][k:]) == nanb) and np.all(_bits(o["det_scores"][k:]) == nanb) and np.all(o["det_src"][k:] == SENT), name
    if c.post is None:
        _untouched(o, L)
        assert o["pin"] is None or o["pin"][0] == SENT
    else:
        f = len(exp["fin_scores"])
        assert o["fin_count"].tolist() == [f, SENT, SENT, SENT], (name, o["fin_count"], f)
        assert _same_bits(o["fin_boxes"][:f], exp["fin_boxes"]) and _same_bits(o["fin_scores"][:f], exp["fin_scores"]), name
        assert np.all(_bits(o["fin_boxes"][f:]) == nanb) and np.all(_bits(o["fin_scores"][f:]) == nanb), name
        if c.record != "none":
            assert o["pin"][0] == f and o["pin"][1] == SENT, (name, o["pin"])
        if c.record == "rec":
            assert np.array_equal(o["rec"], RT.fill_record(c.cap, exp["fin_boxes"], exp["fin_scores"], REC_FILL)), name
    for cls in c.classes:
        RAN.add((c.form, cls))


@pytest.mark.parametrize("name,cap,Cc,parts,post,outs,ws", RT.REFUSALS, ids=[r[0] for r in RT.REFUSALS])
def test_refusals_return_before_any_launch(L, name, cap, Cc, parts, post, outs, ws):
    base = RT.case("f64-cap64-C16")
    la = Launch(L, base, cap=cap, C_=Cc, parts=parts, post=RT.POSTS["up"] if post else None, outs=outs, ws=ws)
    rc = la.run()
    assert rc != 0 and L.ore_last_error(), name
    o = la.result()
    nanb = np.float32("nan").view(np.uint32)
    assert np.all(_bits(o["det_boxes"]) == nanb) and np.all(_bits(o["det_scores"]) == nanb) and np.all(o["det_src"] == SENT)
    assert np.all(o["det_count"] == SENT)
    _untouched(o, L)
    assert np.all(la.ws.cpu().numpy() == 0xFF)                  # not even the workspace was written


@pytest.mark.parametrize("name", ["FUSED8-post-up-rec", "FUSED64-post-nonuniform-zero", "FUSED8-thr0.6", "GENERAL-thr0.6"])
def test_binding_hands_parts_post_and_pin_over(name):
    """orehip.roi_predict(parts=, bias=, post=, pin=) reaches the same launch as the C ABI call above."""
    import orehip
    c = RT.case(name)
    exp = RT.expected(c)
    assert c.n == c.cap and not c.n_on_device
    pin = rec = None
    if c.record != "none":
        pin = torch.zeros(4, dtype=torch.int32, device="cuda")
        if c.record == "rec":
            rec = torch.full((c.cap * 28,), REC_FILL, dtype=torch.uint8, device="cuda")
            pin[2:4] = torch.from_numpy(np.array([rec.data_ptr()], np.uint64).view(np.int32).copy()).cuda()
    o = orehip.roi_predict(_dev(c.h), _dev(c.cls_w), _dev(c.cls_b), _dev(c.box_w), _dev(c.box_b), _dev(c.boxes), RT.REG_W, c.img, c.score_thresh,
                           c.nms_thresh, c.topk, parts=c.parts, bias=None if c.bias is None else _dev(c.bias),
                           post=None if c.post is None else _dev(c.post), pin=pin)
    torch.cuda.synchronize()
    k = int(o["count"].item())
    assert k == len(exp["scores"]) and _same_bits(o["boxes"][:k].cpu().numpy(), exp["boxes"]) and np.array_equal(o["src"][:k].cpu().numpy(), exp["src"])
    assert ("fin_count" in o) == (c.post is not None)
    if c.post is not None:
        f = int(o["fin_count"].item())
        assert f == len(exp["fin_scores"]) == int(pin[0].item())
        assert _same_bits(o["fin_boxes"][:f].cpu().numpy(), exp["fin_boxes"]) and _same_bits(o["fin_scores"][:f].cpu().numpy(), exp["fin_scores"])
    if rec is not None:
        assert np.array_equal(rec.cpu().numpy(), RT.fill_record(c.cap, exp["fin_boxes"], exp["fin_scores"], REC_FILL))
    with pytest.raises(orehip.OreError):
        orehip.roi_predict(_dev(c.h), _dev(c.cls_w), _dev(c.cls_b), _dev(c.box_w), _dev(c.box_b), _dev(c.boxes), RT.REG_W, c.img, 0.0, 0.5, 10,
                           parts=c.parts + 1)


# ---- the NMS behind the general path, and the row-major scan -------------------------------------------------------------------------
_TWIN = {}


def _twin_nms(key, boxes, scores, thr):
    if key not in _TWIN:
        _TWIN[key] = odec.nms(boxes, scores, thr)
    return _TWIN[key]


def _nms_call(L, boxes, scores, n, thr, n_dev=None, cap=None):
    rows = cap if n_dev is not None else n
    keep = torch.full((max(rows, 1) + 8,), SENT, dtype=torch.int64, device="cuda")
    cnt = torch.full((4,), SENT, dtype=torch.int32, device="cuda")
    wsb = L.ore_nms_workspace_bytes(rows)
    ws = torch.full((wsb,), 0xFF, dtype=torch.uint8, device="cuda")
    b, s = _dev(boxes), _dev(scores)
    if n_dev is None:
        rc = L.ore_nms_fwd(b.data_ptr(), s.data_ptr(), n, thr, keep.data_ptr(), cnt.data_ptr(), ws.data_ptr(), wsb, _stream())
    else:
        nd = torch.tensor([n_dev], dtype=torch.int32, device="cuda")
        rc = L.ore_nms_device_n_fwd(b.data_ptr(), s.data_ptr(), nd.data_ptr(), cap, thr, keep.data_ptr(), cnt.data_ptr(), ws.data_ptr(), wsb, _stream())
    torch.cuda.synchronize()
    assert rc == 0, L.ore_last_error()
    return keep.cpu().numpy(), cnt.cpu().numpy()


@pytest.mark.parametrize("cap", [1, 64, 65, 600])
def test_nms_device_count_vs_twin(L, cap):
    """Counts below, at and above the capacity; the tensors hold cap + 64 rows, a count above cap is the NMS of the first cap rows."""
    boxes, scores = RT.nms_inputs(cap + 64, 7000 + cap)
    for n_dev in (0, 1, 63, 64, 65, cap, cap + 3):
        n = min(n_dev, cap)
        for thr in (0.5, 0.9):
            want = _twin_nms(("dev", cap, n, thr), boxes[:n], scores[:n], thr)
            keep, cnt = _nms_call(L, boxes, scores, None, thr, n_dev=n_dev, cap=cap)
            assert cnt.tolist() == [len(want), SENT, SENT, SENT], (cap, n_dev, thr, cnt)
            assert np.array_equal(keep[:len(want)], want), (cap, n_dev, thr)
            assert np.all(keep[len(want):] == SENT), (cap, n_dev, thr)


@pytest.mark.parametrize("n", [3073, 4096, 4097, 8192, 8193])
def test_row_major_scan_vs_twin(L, n):
    """k_nms_mask + k_nms_scan<1|2|4> (n > 3072): two row counts per template form and the first one, keep lists bit for bit."""
    boxes, scores = RT.nms_inputs(n, 9000 + n)
    assert len(np.unique(scores)) < n - n // 6                   # ties
    for thr in (0.6, 0.9):
        want = _twin_nms(("row", n, thr), boxes, scores, thr)
        keep, cnt = _nms_call(L, boxes, scores, n, thr)
        assert 0 < len(want) < n and cnt[0] == len(want), (n, thr, cnt, len(want))
        assert np.array_equal(keep[:len(want)], want), (n, thr)
        assert np.all(keep[n:] == SENT)


@pytest.mark.parametrize("n", [512, 3073], ids=["transposed-mask", "row-major-mask"])
@pytest.mark.parametrize("thr", RT.THRESHOLDS)
def test_near_threshold_pairs_through_nms(L, thr, n):
    """The pairs within 2^-20 of the threshold (tests/test_roitail_host.py counts them) through k_nms_mask_t and k_nms_mask."""
    boxes, scores = RT.near_nms_inputs(thr, n)
    want = _twin_nms(("near", n, thr), boxes, scores, thr)
    a, b = RT.near_threshold(thr, 1)
    assert len(want) == n - int(RT.band_stats(a, b, thr)["above"].sum())
    keep, cnt = _nms_call(L, boxes, scores, n, thr)
    assert cnt[0] == len(want) and np.array_equal(keep[:len(want)], want), (thr, n)


def test_zz_every_form_ran_every_class():
    """Closing test: the (form, class) pairs of the table, each launched above."""
    want = {(c.form, k) for c in RT.cases() for k in c.classes}
    assert {f for f, _ in want} == {RT.FUSED64, RT.FUSED8, RT.GENERAL}
    assert want == {
        (f, k) for f in (RT.FUSED64, RT.FUSED8, RT.GENERAL)
        for k in ("shape", "count", "filter", "topk", "earlystop", "threshold", "near", "ties", "chain", "on_threshold", "nonfinite")
    } | {(f, k) for f in (RT.FUSED64, RT.FUSED8) for k in ("post", "record-none", "record-zero", "record-rec")} \
      | {(RT.FUSED8, "parts"), (RT.FUSED8, "cancelling"), (RT.GENERAL, "pass")}
    assert RAN == want, sorted(want ^ RAN)
