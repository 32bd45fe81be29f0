"""CPU: the second-stage tail's case table (tests/roitail_ref.py) without a GPU.

  * every case has the property it was built for, computed from the C twin's own outputs (band counts, filter outcome, block count,
    early stop, chain depth, rows exactly on the score threshold, non-finite rows);
  * the twin agrees with an independent float64 restatement of predict + NMS wherever the decisions are clear, so twin and kernel
    cannot be wrong together;
  * the numpy emulation of the tail equals the twin on every case, and each seeded fault changes at least one case: the table sees it;
  * form() is the launcher's rule, read from oreroi::roi_predict_post."""
import os
import re

import numpy as np
import pytest

import roitail_ref as RT
from conftest import PKG

F32 = np.float32
CASES = RT.cases()
BY_CLASS = {}
for _c in CASES:
    for _k in _c.classes:
        BY_CLASS.setdefault(_k, []).append(_c)


def _sorted_filtered(case):
    """The filtered rows in the tail's order (score descending, ties by row), from the twin: boxes, scores, source rows."""
    rows = RT.rows_of(case)
    fin, tw = RT.finite_rows(case, rows)
    ok = fin & (tw["raw_scores"] > F32(case.score_thresh))
    comp = np.nonzero(ok)[0]
    order = np.lexsort((comp, -tw["raw_scores"][comp].astype(np.float64)))
    return tw["raw_boxes"][comp][order], tw["raw_scores"][comp][order], comp[order]


def _full_keep(case):
    """The twin's whole survivor list (no top-k) as positions in the sorted filtered list."""
    sb, ss, src = _sorted_filtered(case)
    tw = RT.predict(RT.rows_of(case), case, topk=-1)
    pos = {int(s): i for i, s in enumerate(src)}
    return np.array([pos[int(s)] for s in tw["src"]], np.int64), len(src)


# ---- the table itself ----------------------------------------------------------------------------------------------------------------
def test_table_covers_the_axes_of_every_form():
    by_form = {f: [c for c in CASES if c.form == f] for f in (RT.FUSED64, RT.FUSED8, RT.GENERAL)}
    assert not [c.name for c in CASES if c.form == RT.REFUSED]
    f64, f8, gen = by_form[RT.FUSED64], by_form[RT.FUSED8], by_form[RT.GENERAL]
    assert {1, 2, 63, 64, 65, 320, 511, 512} <= {c.cap for c in f64} and {1, 16, 128, 208} <= {c.C for c in f64}
    assert {(c.cap, c.C) for c in f64} >= {(cap, C) for cap in (1, 2, 63, 64, 65, 320, 511, 512) for C in (1, 16, 128, 208)}
    assert {(c.cap, c.C) for c in f8} >= {(cap, C) for cap in (1, 7, 8, 9, 320, 510) for C in (16, 128, 208)}
    assert {(c.parts, c.bias is not None) for c in f8} >= {(S, b) for S in (2, 15, 16, 17, 32, 33) for b in (False, True)}
    assert {(c.cap, c.C) for c in gen} >= {(cap, C) for cap in (513, 600, 1024) for C in (1, 128, 145)}
    assert {c.n for c in gen} >= {255, 256, 257, 513}
    assert max(c.cap for c in CASES) <= 1024
    for f, cs in by_form.items():
        assert {c.nms_thresh for c in cs} >= set(RT.THRESHOLDS), f
        assert {c.topk for c in cs if "topk" in c.classes} == set(RT.TOPKS), f
        assert {(c.n_on_device, np.sign(c.n - c.cap)) for c in cs if "count" in c.classes and c.n} == \
            {(d, s) for d in (False, True) for s in (-1, 0, 1)}, f
        want = {"shape", "count", "filter", "topk", "earlystop", "threshold", "near", "ties", "chain", "on_threshold", "nonfinite"}
        assert want <= {k for c in cs for k in c.classes}, f
    for f in (RT.FUSED64, RT.FUSED8):
        posts = [c for c in by_form[f] if c.post is not None]
        assert {c.record for c in posts} == {"none", "zero", "rec"}
        assert all(c.cap % 2 == 0 for c in posts if c.record == "rec")
    assert not [c.name for c in gen if c.post is not None or c.record != "none"]
    # rows of the partials at and beyond the count are NaN: summed, never used
    for c in f8:
        assert np.isnan(c.h[:, c.n_eff:]).all()
        if "nonfinite" not in c.classes:
            assert np.isfinite(c.h[:, :c.n_eff]).all()
    assert any(c.n_eff < c.cap for c in f8)


def test_filter_outcomes_and_block_counts():
    for c in BY_CLASS["filter"]:
        _, _, src = _sorted_filtered(c)
        assert len(src) == c.prop["m"], c.name
    for f in (RT.FUSED64, RT.FUSED8, RT.GENERAL):
        ms = {c.prop["m"] for c in BY_CLASS["filter"] if c.form == f}
        assert ms == {0, 1, 64, 65, 200}, f              # nothing, one row, one full block, one row more, four blocks
    for c in BY_CLASS["topk"]:                           # the walk has more survivors than the small top-k values and fewer than the largest
        keep, m = _full_keep(c)
        assert 100 < len(keep) < 1000 and m > 128, (c.name, len(keep), m)


def test_early_stop_cases_stop_after_block_0():
    for c in BY_CLASS["earlystop"]:
        keep, m = _full_keep(c)
        assert (m + 63) // 64 >= 3, c.name
        assert int((keep < 64).sum()) >= c.topk > 0, c.name           # topk survivors are known once block 0 is resolved
        assert int((keep < 64).sum()) < 64, c.name                    # and block 0 has suppressions of its own to resolve first
        assert RT.emulate(c)["walked"] == 1


def test_clustered_rows_are_suppressed_across_blocks():
    for c in BY_CLASS["threshold"]:
        if c.nms_thresh > 0.6:
            continue
        keep, m = _full_keep(c)
        sb, _, _ = _sorted_filtered(c)
        assert len(keep) < m / 2, (c.name, len(keep), m)              # most rows are suppressed
        S = RT.sup_matrix(sb, c.nms_thresh)
        kept = np.zeros(m, bool)
        kept[keep] = True
        blk = np.arange(m) // 64
        cross = (S & kept[:, None] & (blk[:, None] < blk[None, :])).any(0) & ~kept
        assert int(cross.sum()) > m / 4, (c.name, int(cross.sum()))   # by a survivor of an EARLIER 64-row block


def test_chain_cases_need_the_stated_fixpoint_depth():
    depth = {}
    for c in BY_CLASS["chain"]:
        start, L = c.prop["chain"]
        exp = RT.expected(c)
        assert np.array_equal(exp["raw_boxes"], c.boxes[:c.n]), c.name          # the predictor hands the boxes through bit for bit
        assert np.all(np.diff(exp["raw_scores"]) < 0), c.name                    # row order = score order
        S = RT.sup_matrix(exp["raw_boxes"], c.nms_thresh)
        i = np.arange(c.n)
        assert np.array_equal(S & (i[:, None] < i[None, :]), (i[None, :] == i[:, None] + 1) & (i[:, None] >= start) & (i[None, :] < start + L))
        want = np.concatenate([i[:start], i[start:start + L:2], i[start + L:]])  # greedy keeps every other link
        assert np.array_equal(exp["src"], want), c.name
        depth[(c.form, start, L)] = RT.emulate(c)["rounds"]
    for f in (RT.FUSED64, RT.FUSED8, RT.GENERAL):
        assert depth[(f, 0, 64)] == 63                   # one block, the full depth the 64 rounds allow
        assert depth[(f, 32, 64)] == 31                  # straddles two blocks: 32 links in each
        assert depth[(f, 100, 40)] >= 27


@pytest.mark.parametrize("thr", RT.THRESHOLDS)
def test_near_threshold_family_sits_in_the_band(thr):
    a, b = RT.near_threshold(thr, 1)
    st = RT.band_stats(a, b, thr)
    n = {k: int(v.sum()) for k, v in st.items()}
    assert n["band_above"] >= 4 and n["band_below"] >= 26 and n["clear_above"] >= 24 and n["clear_below"] >= 24, n
    # different pairs never overlap
    fam = np.stack([a, b], 1).reshape(-1, 4)
    S = RT.sup_matrix(fam, 1e-6)
    i = np.arange(len(fam))
    assert not (S & (i[:, None] // 2 != i[None, :] // 2)).any()
    # the doubled family decides every pair it keeps as the undoubled one does, and keeps pairs of every kind
    a2, b2 = RT.near_threshold(thr, 2)
    assert np.all(a2 % 2 == 0) and np.all(b2 % 2 == 0) and a2.max() <= 1 << 24
    st2 = RT.band_stats(a2, b2, thr)
    half = RT.band_stats(a2 * np.array([0.5, 1, 0.5, 1], F32), b2 * np.array([0.5, 1, 0.5, 1], F32), thr)
    for k in st2:
        assert np.array_equal(st2[k], half[k]), k
    n2 = {k: int(v.sum()) for k, v in st2.items()}
    assert n2["band_above"] >= 2 and n2["band_below"] >= 20 and n2["clear_above"] >= 20 and n2["clear_below"] >= 20, n2


def test_near_threshold_cases_pass_the_predictor_bit_for_bit():
    for c in BY_CLASS["near"]:
        exp = RT.expected(c)
        assert np.array_equal(exp["raw_boxes"], c.boxes[:c.n]), c.name
        assert np.all(np.diff(exp["raw_scores"]) < 0), c.name
        a, b = c.boxes[0:c.n:2], c.boxes[1:c.n:2]
        st = RT.band_stats(a, b, c.nms_thresh)
        want = np.sort(np.concatenate([np.arange(0, c.n, 2), np.arange(1, c.n, 2)[~st["above"]]]))
        assert np.array_equal(exp["src"], want), c.name                           # the inner box goes exactly where fl(inter / uni) > thr


def test_ties_on_threshold_and_nonfinite_cases():
    for c in BY_CLASS["ties"]:
        exp = RT.expected(c)
        _, ss, src = _sorted_filtered(c)
        tied = ss[1:] == ss[:-1]
        assert int(tied.sum()) > 50, c.name
        assert np.all(src[1:][tied] > src[:-1][tied])                             # equal scores: the lower row first
        ds = exp["scores"]
        assert int((ds[1:] == ds[:-1]).sum()) > 5, c.name                         # and tied rows survive side by side into the result
    for c in BY_CLASS["on_threshold"]:
        exp = RT.expected(c)
        on = exp["raw_scores"] == F32(0.5)
        assert int(on.sum()) == c.prop["on_threshold"] == 30 and c.score_thresh == 0.5
        assert np.array_equal(exp["src"], np.nonzero(~on)[0]), c.name             # strict filter: a score ON the threshold is rejected
    for c in BY_CLASS["nonfinite"]:
        rows = RT.rows_of(c)
        fin, _ = RT.finite_rows(c, rows)
        r_inf, r_nan = c.prop["nonfinite"]
        assert np.isinf(rows[r_inf, 3]) and not fin[r_inf], c.name
        if c.parts:        # K-split form: the ReLU behind the sum is fmaxf, which turns the NaN into 0: the row is an ordinary row again
            assert rows[r_nan, 3] == 0 and fin[r_nan], c.name
        else:
            assert np.isnan(rows[r_nan, 3]) and not fin[r_nan], c.name
        assert fin.sum() == c.n_eff - (1 if c.parts else 2)
        assert fin[r_inf - 1] and fin[r_inf + 1] and fin[r_nan - 1] and fin[r_nan + 1]          # dropped between valid neighbours
        exp = RT.expected(c)
        assert r_inf not in exp["src"] and len(exp["src"]) > 100 and (c.parts or r_nan not in exp["src"])


def test_cancelling_parts_depend_on_the_order():
    for c in BY_CLASS["cancelling"]:
        ref = RT.sum_parts(c.h, c.bias)
        assert np.abs(c.h[:, :c.n_eff]).min() > 4e3 or c.parts % 2, c.name
        assert np.abs(ref).max() < 50
        for fault in ("parts_reverse", "parts_pairwise") + (("bias_last",) if c.bias is not None else ()):
            if c.parts == 2 and fault != "bias_last":
                continue                 # two partials of one magnitude sit on one fp32 grid: either order rounds the bias alike
            assert (RT.sum_parts(c.h, c.bias, fault).view(np.uint32) != ref.view(np.uint32)).mean() > 0.2, (c.name, fault)
    # and sum_parts is the plain ordered sum
    p = np.array([[[1e8]], [[1.0]], [[-1e8]], [[np.nan]]], F32)
    assert RT.sum_parts(p[:3], None)[0, 0] == 0 and RT.sum_parts(p[:3], None, "parts_reverse")[0, 0] == 0
    assert RT.sum_parts(p[[0, 2, 1]], None)[0, 0] == 1 and RT.sum_parts(p, None)[0, 0] == 0      # NaN -> 0, as fmaxf gives
    assert RT.sum_parts(p[1:2], np.array([-3.0], F32))[0, 0] == 0


def test_postprocess_cases():
    from test_nway_host import merge_classes
    seen_drop = False
    for c in BY_CLASS["post"]:
        exp = RT.expected(c)
        sx, sy, ow, oh = (float(v) for v in c.post)
        k = len(exp["scores"])
        # the same arithmetic as the N-way merge's postprocess (one class, list already in score order)
        if k and np.all(np.diff(exp["scores"].astype(np.float64)) < 0):
            b, s, _ = merge_classes([(exp["boxes"], exp["scores"])], [0], max(k, 1), (oh / sy, ow / sx), (oh, ow))
            if F32(ow / (ow / sx)) == F32(sx) and F32(oh / (oh / sy)) == F32(sy):
                assert np.array_equal(b, exp["fin_boxes"]) and np.array_equal(s, exp["fin_scores"]), c.name
        if "emptying" in c.name:
            _, keep = RT.scale_clip_drop(exp["boxes"], *c.post)
            assert 0.2 * k < keep.sum() < 0.8 * k and np.any(keep[1:] != keep[:-1]), c.name      # interleaved rows go
            assert int((keep[1:] != keep[:-1]).sum()) > 10
            seen_drop = True
        if "identity" in c.name:
            assert np.array_equal(exp["fin_boxes"], exp["boxes"]), c.name
    assert seen_drop
    buf, rb, rs, rc = RT.record_views(6)
    assert (buf == 0).all() and rb.shape == (6, 4) and rs.shape == (6,) and rc.shape == (6,) and rc.dtype == np.int64
    rb[:] = 1
    rs[:] = 2
    rc[:] = -1
    assert np.all(buf[:96].view(F32) == 1) and np.all(buf[96:120].view(F32) == 2) and np.all(buf[120:] == 255)
    with pytest.raises(AssertionError):
        RT.record_views(5)


# ---- twin against an independent float64 restatement ---------------------------------------------------------------------------------
def _predict_f64(c, rows):
    h = rows.astype(np.float64)
    lg = h @ c.cls_w.astype(np.float64).T + c.cls_b
    dl = h @ c.box_w.astype(np.float64).T + c.box_b
    score = 1.0 / (1.0 + np.exp(lg[:, 1] - lg[:, 0]))
    p = c.boxes[:len(rows)].astype(np.float64)
    w, hg = p[:, 2] - p[:, 0], p[:, 3] - p[:, 1]
    cx, cy = p[:, 0] + 0.5 * w, p[:, 1] + 0.5 * hg
    clamp = np.log(1000.0 / 16.0)
    pcx, pcy = dl[:, 0] / 10 * w + cx, dl[:, 1] / 10 * hg + cy
    pw, ph = np.exp(np.minimum(dl[:, 2] / 5, clamp)) * w, np.exp(np.minimum(dl[:, 3] / 5, clamp)) * hg
    b = np.stack([pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph], 1)
    b[:, 0::2] = np.clip(b[:, 0::2], 0, c.img[1])
    b[:, 1::2] = np.clip(b[:, 1::2], 0, c.img[0])
    return b, score


def _nms_f64(b, s, thr):
    """Greedy NMS in float64; also the distance of the closest IoU to the threshold."""
    order = np.lexsort((np.arange(len(s)), -s))
    b = b[order]
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    wh = np.clip(np.minimum(b[:, None, 2:], b[None, :, 2:]) - np.maximum(b[:, None, :2], b[None, :, :2]), 0, None)
    inter = wh[..., 0] * wh[..., 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        iou = inter / (area[:, None] + area[None, :] - inter)
    dead = np.zeros(len(s), bool)
    keep = []
    for i in range(len(s)):
        if dead[i]:
            continue
        keep.append(i)
        dead[i + 1:] |= iou[i, i + 1:] > thr
    off = iou[np.triu_indices(len(s), 1)]
    return order[keep], float(np.abs(off - thr).min()) if len(off) else 1.0


def test_twin_agrees_with_a_float64_restatement_on_clear_decisions():
    clear = 0
    for c in CASES:
        if c.classes[0] not in ("shape", "threshold", "topk", "filter", "pass", "count") or c.n_eff == 0:
            continue
        rows = RT.rows_of(c)
        b, s = _predict_f64(c, rows)
        tw = RT.expected(c)
        assert np.abs(tw["raw_scores"] - s).max() < 2e-6, c.name                   # ore_expf is within a few ulp of exp
        assert np.abs(tw["raw_boxes"] - b).max() < 2e-3, c.name
        ok = s > c.score_thresh
        idx = np.nonzero(ok)[0]
        keep, gap = _nms_f64(b[idx], s[idx], c.nms_thresh)
        ss = np.sort(s[idx])
        if gap < 1e-4 or (len(ss) > 1 and np.diff(ss).min() < 1e-6) or np.abs(s - c.score_thresh).min() < 1e-6:
            continue                                                                # a decision float64 and fp32 may take differently
        src = idx[keep]
        if c.topk >= 0:
            src = src[:c.topk]
        assert np.array_equal(src, tw["src"]), c.name
        clear += 1
    assert clear >= 40, clear


# ---- the emulation, and what the table can see ---------------------------------------------------------------------------------------
def test_emulation_equals_the_twin_on_every_case():
    for c in CASES:
        exp = dict(RT.expected(c))
        if c.record == "rec":
            exp["record"] = RT.fill_record(c.cap, exp["fin_boxes"], exp["fin_scores"], 0xA5)
        em = RT.emulate(c)
        assert RT.same(em, exp), c.name
        assert len(em["src"]) == len(exp["src"])


@pytest.mark.parametrize("fault", RT.FAULTS)
def test_every_seeded_fault_changes_a_case(fault):
    hits = []
    for c in CASES:
        if fault.startswith(("parts_", "bias_")) and not c.parts:
            continue
        if fault in ("clip_first", "rec_scores_20") and c.post is None:
            continue
        exp = dict(RT.expected(c))
        if c.record == "rec":
            exp["record"] = RT.fill_record(c.cap, exp["fin_boxes"], exp["fin_scores"], 0xA5)
        if not RT.same(RT.emulate(c, fault), exp):
            hits.append(c.name)
            if len({RT.case(h).form for h in hits}) >= 2 or len(hits) >= 12:
                break
    assert hits, fault
    want = {"filter_ge": "on-threshold", "iou_nodiv": "near", "iou_ge": "near", "fix8": "chain", "ties_desc": ""}.get(fault)
    if want:
        assert any(want in h for h in hits), (fault, hits)


# ---- the launcher's rule -------------------------------------------------------------------------------------------------------------
def test_form_is_the_launchers_rule():
    src = open(os.path.join(PKG, "csrc", "ore_roi.hip")).read()
    body = src[src.index("int oreroi::roi_predict_post("):]
    body = body[:body.index("\nstatic int roi_align_bwd_impl")]
    assert int(re.search(r"constexpr int ROI_FUSED_CAP = (\d+);", src)[1]) == RT.FUSED_CAP == 512
    m = re.search(r"if \(cap <= ROI_FUSED_CAP && \(size_t\)C \* 4 \* 71 \+ 6 \* 64 \* 4 <= 60 \* 1024\) \{", body)
    assert m, "the fused path's condition changed"
    fused_c = max(C for C in range(1, 1000) if C * 4 * 71 + 6 * 64 * 4 <= 60 * 1024)
    m = re.search(r"const size_t lds = \(\(size_t\)256 \* \(C \+ 1\) \+ 6 \* \(size_t\)C\) \* sizeof\(float\);\s*ORE_CHECK_ARG\(lds <= 150 \* 1024", body)
    assert m, "the general path's condition changed"
    general_c = max(C for C in range(1, 1000) if (256 * (C + 1) + 6 * C) * 4 <= 150 * 1024)
    assert (fused_c, general_c) == (RT.FUSED_C, RT.GENERAL_C) == (210, 145)
    assert "k_roi_predict_mb<8>" in body and "k_roi_predict_mb<64>" in body and "ore_nms_device_n_fwd(" in body and "k_roi_finalize" in body
    assert re.search(r"ORE_CHECK_ARG\(h_parts == 0,", body) and re.search(r"ORE_CHECK_ARG\(!post_dev \|\| cap <= ROI_FUSED_CAP", body)

    def rule(cap, C, parts):
        if cap <= 512 and C * 4 * 71 + 6 * 64 * 4 <= 60 * 1024:
            return RT.FUSED8 if parts > 0 else RT.FUSED64
        if parts != 0 or (256 * (C + 1) + 6 * C) * 4 > 150 * 1024:
            return RT.REFUSED
        return RT.GENERAL
    for cap in (1, 2, 63, 64, 65, 320, 510, 511, 512, 513, 600, 1024):
        for C in (1, 16, 128, 145, 146, 208, 209, 210, 211):
            for parts in (0, 1, 2, 32, 33):
                assert RT.form(cap, C, parts) == rule(cap, C, parts), (cap, C, parts)
    # the engine's own bound on the fc width is the fused one, in multiples of 16: 208 is the widest head it launches
    eng = open(os.path.join(PKG, "csrc", "ore_engine.hip")).read()
    assert "fc_dim % 16 == 0" in eng and "(size_t)fc_dim * 4 * 71 + 6 * 64 * 4 <= 60 * 1024" in eng
    assert max(C for C in range(16, 1000, 16) if C <= RT.FUSED_C) == 208
    for name, cap, C, parts, post, outs, ws in RT.REFUSALS:
        if outs and ws and not post:
            assert RT.form(cap, C, parts) == RT.REFUSED, name
