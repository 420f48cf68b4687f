"""Detection quality, host side: msocr_quad_match_host (csrc/quad_iou.h) against a Python restatement of
the matching rule of include/msocr.h, the C ABI's refusals, detectors.match_detections / detection_f1 / load_coco_quads,
Pipeline.evaluate on stand-in plugins, and the header once more in a stand-alone program under the address and undefined-behaviour
sanitizers (tests/native/quad_match_fuzz.cpp).  No GPU.

The yardstick (ref_match) is written from the header's text: validity and canonical winding in NumPy f64, the IoU from
oracle.lanms.polygon_iou, and the control flow of the reference's compute_f1 (detectors/_east/utils.py:435-474), once per threshold.
Match indices and counts are integers and the IoUs are the same f64 operations in the same order on both sides: everything is
compared for equality, the IoUs bit for bit.  tests/test_gpu_quad_match.py imports the helpers and cases of this file."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

E_ARG = -1
DEFAULT_T = np.arange(0.50, 0.95 + 1e-9, 0.05)


def _lib():
    from manuscript_ocr_amd import _native as nat
    return nat.lib()


# ------------------------------------------------------------------------------------------------ the reference
def canonical(q):
    """The header's validity and winding rule on one [4,2] f32 quad -> [4,2] f64 with positive turns, or None (invalid)."""
    v = np.asarray(q, dtype=np.float32).astype(np.float64).reshape(4, 2)
    if not np.all(np.isfinite(v)):
        return None
    c = []
    for i in range(4):
        a, b = v[(i + 1) % 4] - v[i], v[(i + 2) % 4] - v[(i + 1) % 4]
        c.append(a[0] * b[1] - a[1] * b[0])
    if all(x > 0 for x in c):
        return v
    if all(x < 0 for x in c):
        return v[[0, 3, 2, 1]]
    return None


def ref_match(pred_pages, gt_pages, thresholds):
    """-> per page (match int32 [T,n], iou f64 [T,n]) and counts int64 [N,T,3]; compute_f1's loop, line by line, per threshold."""
    from oracle import lanms
    out, counts = [], np.zeros((len(pred_pages), len(thresholds), 3), dtype=np.int64)
    for p, (preds, gts) in enumerate(zip(pred_pages, gt_pages)):
        pred_polys = [canonical(q) for q in preds]
        gt_polys = [canonical(q) for q in gts]
        cache = {}

        def iou_of(i, j):  # polygon_iou(prediction, ground truth); the value does not depend on the threshold
            if (i, j) not in cache:
                cache[(i, j)] = lanms.polygon_iou(pred_polys[i], gt_polys[j])
            return cache[(i, j)]

        match = np.full((len(thresholds), len(preds)), -9, dtype=np.int32)
        ious = np.full((len(thresholds), len(preds)), np.nan)
        for k, thresh in enumerate(thresholds):
            used = [False] * len(gt_polys)
            tp = fp = 0
            for i, pred_polygon in enumerate(pred_polys):
                if pred_polygon is None:
                    fp += 1
                    match[k, i], ious[k, i] = -2, 0.0
                    continue
                best_iou, bj = 0.0, -1
                for j, gt_polygon in enumerate(gt_polys):
                    if used[j] or gt_polygon is None:
                        continue
                    iou = iou_of(i, j)
                    if iou > best_iou:
                        best_iou, bj = iou, j
                ious[k, i] = best_iou
                if best_iou >= thresh:
                    tp += 1
                    used[bj] = True
                    match[k, i] = bj
                else:
                    fp += 1
                    match[k, i] = -1
            counts[p, k] = (tp, fp, len(gt_polys) - tp)
        out.append((match, ious))
    return out, counts


def pack(pages, pad_to=None):
    n = np.array([len(q) for q in pages], dtype=np.int32)
    m = max(int(n.max()) if len(n) else 0, pad_to or 0)
    a = np.zeros((len(pages), m, 4, 2), dtype=np.float32)
    for p, q in enumerate(pages):
        if len(q):
            a[p, : len(q)] = np.asarray(q, dtype=np.float32).reshape(-1, 4, 2)
    return a, n


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def check_against_reference(pred_pages, gt_pages, thresholds, got=None):
    """msocr_quad_match_host (or `got` = (match, iou, counts) of another implementation) == ref_match, everywhere."""
    from manuscript_ocr_amd import ops
    thresholds = np.asarray(thresholds, dtype=np.float64)
    if got is None:
        got = ops.quad_match_host(*pack(pred_pages), *pack(gt_pages), thresholds)
    match, iou, counts = got
    exp, exp_counts = ref_match(pred_pages, gt_pages, thresholds)
    assert np.array_equal(np.asarray(counts, dtype=np.int64), exp_counts), (counts, exp_counts)
    for p, (m, i) in enumerate(exp):
        n = m.shape[1]
        assert np.array_equal(match[p, :, :n], m), (p, match[p, :, :n], m)
        assert same_bits(iou[p, :, :n], i), (p, iou[p, :, :n], i)
    return exp, exp_counts


# ------------------------------------------------------------------------------------------------ quads
def rect(x0, y0, x1, y1):
    return [[x0, y0], [x1, y0], [x1, y1], [x0, y1]]


def rotated(cx, cy, w, h, deg):
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    return [[cx + c * dx - s * dy, cy + s * dx + c * dy] for dx, dy in ((-w / 2, -h / 2), (w / 2, -h / 2), (w / 2, h / 2), (-w / 2, h / 2))]


BOW_TIE = [[0, 0], [10, 10], [10, 0], [0, 10]]
CONCAVE = [[0, 0], [10, 0], [3, 3], [0, 10]]
COLLINEAR = [[0, 0], [5, 0], [10, 0], [5, 10]]
ZERO_AREA = [[4, 4], [4, 4], [4, 4], [4, 4]]
WITH_NAN = [[0, 0], [10, 0], [10, np.nan], [0, 10]]
WITH_INF = [[0, 0], [np.inf, 0], [10, 10], [0, 10]]
INVALID = {"bow-tie": BOW_TIE, "concave": CONCAVE, "collinear": COLLINEAR, "zero-area": ZERO_AREA, "nan": WITH_NAN, "inf": WITH_INF}
UNIT = rect(0, 0, 10, 10)


def random_page(seed, n=300, origin=(0.0, 0.0), drop=0.1, spurious=0.1, tilt=4.0):
    """A page of about n words on a grid: the ground truth, and predictions that are the ground truth jittered, partly dropped, partly
    replaced by spurious boxes, in shuffled order -> (pred [<=n,4,2], gt [n,4,2]) f32."""
    rng = np.random.default_rng(seed)
    cols = 20
    gt = []
    for k in range(n):
        cx = origin[0] + 40 + (k % cols) * 90 + rng.uniform(-8, 8)
        cy = origin[1] + 30 + (k // cols) * 34 + rng.uniform(-3, 3)
        gt.append(rotated(cx, cy, rng.uniform(40, 100), rng.uniform(16, 30), rng.uniform(-tilt, tilt)))
    gt = np.asarray(gt, dtype=np.float32).reshape(-1, 4, 2)
    pred = []
    for q in gt:
        if rng.uniform() < drop:
            continue
        pred.append(q + rng.normal(0, 2.0, size=(4, 2)))
    for _ in range(int(spurious * n)):
        pred.append(rotated(origin[0] + rng.uniform(0, 1900), origin[1] + rng.uniform(0, 34 * (n // cols + 1)), rng.uniform(20, 80),
                            rng.uniform(10, 30), rng.uniform(-30, 30)))
    pred = np.asarray(pred, dtype=np.float32).reshape(-1, 4, 2)[rng.permutation(len(pred))]
    if seed % 2:  # every other page: ground truth in the other winding, as annotations come
        gt = gt[:, ::-1].copy()
    return pred[:n], gt


def special_cases():
    """name -> (pred_pages, gt_pages, thresholds): the small cases of the issue, shared with the GPU file."""
    T3 = [0.3, 0.5, 0.9]
    c = {
        "no predictions": ([[]], [[UNIT, rect(20, 0, 30, 10)]], T3),
        "no ground truth": ([[UNIT, rect(20, 0, 30, 10)]], [[]], T3),
        "empty page": ([[]], [[]], T3),
        "one pair": ([[rect(0, 0, 10, 8)]], [[UNIT]], T3),
        "identical": ([[UNIT, rotated(100, 100, 50, 20, 17)]], [[UNIT, rotated(100, 100, 50, 20, 17)]], list(DEFAULT_T) + [1.0]),
        "tie": ([[UNIT]], [[rect(-5, 0, 5, 10), rect(5, 0, 15, 10)]], [0.3, 0.4]),
        "competing": ([[UNIT, rect(1, 0, 11, 10)]], [[UNIT, rect(4, 0, 14, 10)]], [0.5, 0.6]),
        "independent thresholds": ([[rect(0, 0, 10, 7.1), rect(0, 0, 10, 9.5)]], [[UNIT]], [0.5, 0.6, 0.7, 0.75, 0.9]),
        "reversed winding": ([[UNIT, rect(20, 0, 30, 10)[::-1]]], [[UNIT[::-1], rect(20, 0, 30, 10)]], T3),
        "touching": ([[UNIT]], [[rect(10, 0, 20, 10)]], T3),
        "far apart": ([[UNIT, rect(5000, 5000, 5040, 5020)]], [[rect(3000, 10, 3040, 30), rect(5001, 5001, 5041, 5021)]], T3),
        "rotated at 9000": ([[rotated(8990, 8800, 120, 30, a) for a in (0, 13, 45, 90, 133, -60)]],
                            [[rotated(8991, 8801, 118, 31, a + 2) for a in (0, 13, 45, 90, 133, -60)]], list(DEFAULT_T)),
    }
    for name, q in INVALID.items():
        c[f"invalid prediction: {name}"] = ([[q, UNIT]], [[UNIT, rect(2, 2, 9, 9)]], T3)
        c[f"invalid ground truth: {name}"] = ([[UNIT, rect(1, 1, 9, 9)]], [[q, UNIT]], T3)
    return c


CASES = special_cases()


# ------------------------------------------------------------------------------------------------ the host twin
@pytest.mark.parametrize("name", list(CASES))
def test_host_twin_special_cases(name):
    pred, gt, th = CASES[name]
    check_against_reference(pred, gt, th)


def test_expected_outcomes_of_the_named_cases():
    """The cases do what their names say, under the yardstick itself."""
    from oracle import lanms
    assert lanms.polygon_iou(UNIT, UNIT) == 1.0 and lanms.polygon_iou(UNIT, UNIT[::-1]) == 0.0
    (m, i), = ref_match(*CASES["identical"])[0]
    assert np.array_equal(m, np.tile([0, 1], (11, 1))) and np.all(i == 1.0)
    (m, i), = ref_match(*CASES["tie"])[0]
    a, b = lanms.polygon_iou(UNIT, rect(-5, 0, 5, 10)), lanms.polygon_iou(UNIT, rect(5, 0, 15, 10))
    assert a == b and 0.3 < a < 0.4 and m.tolist() == [[0], [-1]]
    (m, i), = ref_match(*CASES["competing"])[0]
    assert m.tolist() == [[0, 1], [0, -1]]
    (m, i), = ref_match(*CASES["independent thresholds"])[0]
    # 0.71 takes the ground truth up to 0.7; above, it stays free and the later prediction (0.95) takes it
    assert m.tolist() == [[0, -1], [0, -1], [0, -1], [-1, 0], [-1, 0]] and i[0, 1] == 0.0 and i[3, 0] == i[0, 0]
    (m, i), = ref_match(*CASES["reversed winding"])[0]
    assert m.tolist() == [[0, 1]] * 3 and np.all(i == 1.0)
    (m, i), = ref_match(*CASES["touching"])[0]
    assert np.all(m == -1) and np.all(i == 0.0)
    for name in INVALID:
        (m, _), = ref_match(*CASES[f"invalid prediction: {name}"])[0]
        assert m.tolist() == [[-2, 0]] * 3, name
        (m, _), = ref_match(*CASES[f"invalid ground truth: {name}"])[0]
        _, counts = ref_match(*CASES[f"invalid ground truth: {name}"])
        assert m[0].tolist() == [1, -1] and counts[0, 0].tolist() == [1, 1, 1], name  # never matched, but counted


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_host_twin_random_pages(seed):
    pred, gt = random_page(seed, 300, origin=(0.0, 0.0) if seed != 3 else (7000.0, 6000.0))
    assert len(gt) == 300 and 250 <= len(pred) <= 300
    _, counts = check_against_reference([pred], [gt], DEFAULT_T)
    assert counts[0, 0, 0] > 150 and counts[0, -1, 0] < counts[0, 0, 0], counts[0]  # the page exercises both outcomes


def test_ragged_batch_and_padding():
    pages = [random_page(10 + k, n) for k, n in enumerate((0, 7, 40))]
    pred, gt = [p for p, _ in pages], [g for _, g in pages]
    check_against_reference(pred, gt, [0.5, 0.75])
    from manuscript_ocr_amd import ops
    a = ops.quad_match_host(*pack(pred), *pack(gt), [0.5, 0.75])
    b = ops.quad_match_host(*pack(pred, 64), *pack(gt, 50), [0.5, 0.75])  # wider arrays: same results, the rest unwritten
    for p in range(3):
        n = len(pred[p])
        assert np.array_equal(a[0][p, :, :n], b[0][p, :, :n]) and same_bits(a[1][p, :, :n], b[1][p, :, :n])
        assert np.all(b[0][p, :, n:] == -3) and np.all(np.isnan(b[1][p, :, n:]))
    assert np.array_equal(a[2], b[2])


def test_shortcut_is_exact():
    """For strictly convex quads whose boxes are separated by more than the shortcut's margin, the reference's IoU is 0.0: skipping
    the clip there changes nothing."""
    from oracle import lanms
    rng = np.random.default_rng(5)
    checked = 0
    for _ in range(3000):
        scale = 10.0 ** rng.uniform(0, 4)
        a = np.asarray(rotated(rng.uniform(0, scale), rng.uniform(0, scale), rng.uniform(1, 200), rng.uniform(1, 60), rng.uniform(0, 360)))
        b = np.asarray(rotated(0, 0, rng.uniform(1, 200), rng.uniform(1, 60), rng.uniform(0, 360)))
        a = (a + rng.normal(0, 0.05, (4, 2))).astype(np.float32)
        b = (b + rng.normal(0, 0.05, (4, 2))).astype(np.float32)
        gap = 10.0 ** rng.uniform(-1.5, 2)
        if rng.uniform() < 0.5:   # b to the right of a, or below it
            b[:, 0] += a[:, 0].max() - b[:, 0].min() + np.float32(gap)
            b[:, 1] += np.float32(rng.uniform(-50, 50))
        else:
            b[:, 1] += a[:, 1].max() - b[:, 1].min() + np.float32(gap)
            b[:, 0] += np.float32(rng.uniform(-50, 50))
        ca, cb = canonical(a), canonical(b)
        if ca is None or cb is None:
            continue
        ext = max(np.abs(ca).max(), np.abs(cb).max())
        sep = max(cb[:, 0].min() - ca[:, 0].max(), cb[:, 1].min() - ca[:, 1].max())
        if sep <= 1e-6 * (1.0 + ext):
            continue
        assert lanms.polygon_iou(ca, cb) == 0.0 and lanms.polygon_iou(cb, ca) == 0.0
        checked += 1
    assert checked > 2500


# ------------------------------------------------------------------------------------------------ the C ABI
def test_symbols_in_header_bindings_and_library():
    from manuscript_ocr_amd import _native as nat
    from manuscript_ocr_amd import ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "msocr.h")).read()
    for name in ("msocr_quad_match_ws_bytes", "msocr_quad_match", "msocr_quad_match_host"):
        assert name + "(" in header and name in nat.exported_symbols() and hasattr(_lib(), name), name
    assert callable(ops.quad_match) and callable(ops.quad_match_host) and callable(ops.quad_match_workspace_bytes)


def _host_call(pred, n_pred, max_pred, gt, n_gt, max_gt, N, th, T, null=None):
    pred = np.ascontiguousarray(pred, dtype=np.float32)
    gt = np.ascontiguousarray(gt, dtype=np.float32)
    n_pred, n_gt = np.asarray(n_pred, dtype=np.int32), np.asarray(n_gt, dtype=np.int32)
    th = np.asarray(th, dtype=np.float64)
    rows = max(N, 1) * 16 * max(max_pred, 1)
    match, iou, counts = np.zeros(rows, np.int32), np.zeros(rows, np.float64), np.zeros(max(N, 1) * 16 * 3, np.int32)
    ptr = {"pred": pred.ctypes.data, "n_pred": n_pred.ctypes.data, "gt": gt.ctypes.data, "n_gt": n_gt.ctypes.data,
           "thresholds": th.ctypes.data, "match": match.ctypes.data, "iou": iou.ctypes.data, "counts": counts.ctypes.data}
    if null:
        ptr[null] = None
    return _lib().msocr_quad_match_host(ptr["pred"], ptr["n_pred"], max_pred, ptr["gt"], ptr["n_gt"], max_gt, N, ptr["thresholds"], T,
                                        ptr["match"], ptr["iou"], ptr["counts"])


def test_c_abi_refusals():
    q = np.zeros((1, 4, 4, 2), np.float32)
    q[0, :, :] = UNIT
    ok = dict(pred=q, n_pred=[4], max_pred=4, gt=q, n_gt=[4], max_gt=4, N=1, th=[0.5] * 17, T=1)
    assert _host_call(**ok) == 0
    for null in ("pred", "n_pred", "gt", "n_gt", "thresholds", "match", "iou", "counts"):
        assert _host_call(**ok, null=null) == E_ARG, null
    for T in (0, 17, -1):
        assert _host_call(**{**ok, "T": T}) == E_ARG, T
    assert _host_call(**{**ok, "T": 16}) == 0
    for bad in (0.0, -0.1, 1.5, np.nan, np.inf, -np.inf):
        assert _host_call(**{**ok, "th": [0.5, bad], "T": 2}) == E_ARG, bad
        assert _host_call(**{**ok, "th": [0.5, bad], "T": 1}) == 0, bad  # behind T: not read
    assert _host_call(**{**ok, "th": [1.0]}) == 0
    big = np.zeros((1, 16385, 4, 2), np.float32)
    assert _host_call(**{**ok, "pred": big, "max_pred": 16385}) == E_ARG
    assert _host_call(**{**ok, "gt": big, "max_gt": 16385}) == E_ARG
    assert _host_call(**{**ok, "pred": big, "max_pred": 16384, "n_pred": [0]}) == 0
    for k, v in (("n_pred", [5]), ("n_pred", [-1]), ("n_gt", [5]), ("n_gt", [-1]), ("N", -1), ("max_pred", -1), ("max_gt", -1)):
        assert _host_call(**{**ok, k: v}) == E_ARG, (k, v)
    assert _host_call(**{**ok, "N": 0}) == 0
    L = _lib()
    assert L.msocr_quad_match_ws_bytes(16, 512, 512) > 0 and L.msocr_quad_match_ws_bytes(0, 0, 0) >= 0
    for bad in ((-1, 4, 4), (1, 16385, 4), (1, 4, 16385), (1, -1, 4), (1, 4, -1)):
        assert L.msocr_quad_match_ws_bytes(*bad) == E_ARG, bad
    # the device entry point refuses the same before it touches the device: no GPU is needed to be refused
    d = ctypes.c_void_p(8)  # never dereferenced on these paths
    th = np.asarray([0.0], dtype=np.float64)
    assert L.msocr_quad_match(d, d, 4, d, d, 4, 1, th.ctypes.data, 1, d, d, d, d, None) == E_ARG
    th[0] = 0.5
    assert L.msocr_quad_match(d, d, 4, d, d, 4, 1, th.ctypes.data, 1, d, d, d, None, None) == E_ARG  # no workspace
    assert L.msocr_quad_match(d, d, 16385, d, d, 4, 1, th.ctypes.data, 1, d, d, d, d, None) == E_ARG
    assert L.msocr_quad_match(d, d, 4, d, d, 4, 0, th.ctypes.data, 1, d, d, d, d, None) == 0  # N == 0: nothing launched


# ------------------------------------------------------------------------------------------------ the Python layer
def test_detection_f1_by_hand():
    from manuscript_ocr_amd.detectors import DEFAULT_IOU_THRESHOLDS, detection_f1
    assert DEFAULT_IOU_THRESHOLDS.dtype == np.float64 and len(DEFAULT_IOU_THRESHOLDS) == 10 and DEFAULT_IOU_THRESHOLDS[0] == 0.5
    assert np.array_equal(DEFAULT_IOU_THRESHOLDS, DEFAULT_T)
    # two pages, three thresholds: sums (tp, fp, fn) = (6, 2, 4), (3, 5, 7), (0, 8, 10)
    counts = np.array([[[4, 1, 1], [2, 3, 3], [0, 5, 5]], [[2, 1, 3], [1, 2, 4], [0, 3, 5]]])
    r = detection_f1(counts, [0.5, 0.7, 0.9])
    assert r["tp"].tolist() == [6, 3, 0] and r["fp"].tolist() == [2, 5, 8] and r["fn"].tolist() == [4, 7, 10]
    assert r["precision"].tolist() == [6 / 8, 3 / 8, 0.0] and r["recall"].tolist() == [6 / 10, 3 / 10, 0.0]
    f = [2 * (6 / 8) * (6 / 10) / (6 / 8 + 6 / 10), 2 * (3 / 8) * (3 / 10) / (3 / 8 + 3 / 10), 0.0]
    assert r["f1"].tolist() == f and r["f1_at_05"] == f[0] and r["f1_avg"] == float(np.mean(f))
    z = detection_f1(np.zeros((1, 3)), [0.6])  # nothing predicted, nothing annotated: every guard
    assert z["precision"].tolist() == [0.0] and z["recall"].tolist() == [0.0] and z["f1"].tolist() == [0.0] and z["f1_at_05"] is None
    z = detection_f1(np.array([[0, 0, 5]]), [0.5])  # no predictions at all
    assert (z["precision"][0], z["recall"][0], z["f1"][0], z["f1_at_05"]) == (0.0, 0.0, 0.0, 0.0)
    with pytest.raises(ValueError):
        detection_f1(counts)  # three rows are not the ten default thresholds


def test_match_detections_host():
    from manuscript_ocr_amd.detectors import detection_f1, match_detections
    pages = [random_page(20 + k, n) for k, n in enumerate((30, 0, 12))]
    pred, gt = [p for p, _ in pages], [g for _, g in pages]
    m = match_detections(pred, gt)
    exp, counts = ref_match(pred, gt, DEFAULT_T)
    assert np.array_equal(m.counts, counts) and np.array_equal(m.thresholds, DEFAULT_T)
    for p in range(3):
        assert np.array_equal(m.match[p], exp[p][0]) and same_bits(m.iou[p], exp[p][1])
    r = detection_f1(m.counts)
    assert r["tp"].tolist() == counts.sum(axis=0)[:, 0].tolist()
    # scores: a stable descending sort decides the turns; the result stays indexed by the predictions as given
    pred2, gt2, th2 = CASES["competing"]
    plain = match_detections(pred2, gt2, th2)
    assert plain.match[0].tolist() == [[0, 1], [0, -1]]
    turned = match_detections(pred2, gt2, th2, scores=[[0.2, 0.9]])
    exp2, _ = ref_match([[pred2[0][1], pred2[0][0]]], gt2, th2)
    assert turned.match[0][:, [1, 0]].tolist() == exp2[0][0].tolist() and turned.match[0].tolist() == [[-1, 0], [-1, 0]]
    assert match_detections(pred2, gt2, th2, scores=[[0.5, 0.5]]).match[0].tolist() == plain.match[0].tolist()  # stable
    assert match_detections([], []).counts.shape == (0, 10, 3)
    for bad in ([0.0], [1.5], [], [0.5] * 17):
        with pytest.raises(ValueError):
            match_detections(pred2, gt2, bad)
    with pytest.raises(ValueError):
        match_detections(pred2, gt2 + gt2)
    with pytest.raises(ValueError):
        match_detections([np.zeros((16385, 4, 2), np.float32)], [[]])


def test_load_coco_quads(tmp_path):
    from manuscript_ocr_amd.detectors import load_coco_quads
    coco = {"images": [{"id": 7}, {"id": 9}], "annotations": [
        {"id": 1, "image_id": 7, "segmentation": [[0, 0, 10, 0, 10, 5, 0, 5]]},
        {"id": 2, "image_id": 9, "segmentation": [[1.5, 2, 3, 2, 3, 4, 1.5, 4], [9, 9, 9, 9, 9, 9, 9, 9]]},
        {"id": 3, "image_id": 7, "segmentation": [[20, 0, 30, 0, 30, 5, 20, 5]]},
        {"id": 4, "image_id": 7, "segmentation": []},
        {"id": 5, "image_id": 9}]}
    path = tmp_path / "gt.json"
    path.write_text(json.dumps(coco), encoding="utf-8")
    q = load_coco_quads(str(path))
    assert sorted(q) == [7, 9] and q[7].shape == (2, 4, 2) and q[9].shape == (1, 4, 2) and q[7].dtype == np.float32
    assert q[7][1].tolist() == [[20, 0], [30, 0], [30, 5], [20, 5]] and q[9][0].tolist() == [[1.5, 2], [3, 2], [3, 4], [1.5, 4]]
    for bad in ([0, 0, 10, 0, 10, 5], [0, 0, 10, 0, 10, 5, 0, 5, 1, 1], [0, 0, 10, 0, 10, 5, 0, "5"]):
        coco["annotations"][0]["segmentation"] = [bad]
        path.write_text(json.dumps(coco), encoding="utf-8")
        with pytest.raises(ValueError):
            load_coco_quads(str(path))


class StandInDetector:
    def __init__(self, quads):
        self.quads = quads

    def predict(self, image, vis=False, profile=False):
        from manuscript_ocr_amd.detectors._types import Block, Page, Word
        words = [Word(polygon=[[float(x), float(y)] for x, y in q], detection_confidence=0.9) for q in self.quads]
        return {"page": Page(blocks=[Block(words=words)]), "vis_image": None, "score_map": None, "geo_map": None}


class StandInRecognizer:
    """Reads a crop's grey level and looks the text up."""
    def __init__(self, texts):
        self.texts = texts

    def predict(self, images):
        return [{"text": self.texts[int(im[0, 0, 0])], "confidence": 0.5} for im in images]


def test_pipeline_evaluate_on_stand_in_plugins():
    """Four detections, five annotated words.  Detection 0 sits on annotation 0 and is read right; detection 1 overlaps annotation 1
    (IoU 36*20 / (40*20 + 4*20) = 0.818) and is read with one wrong letter; detection 2 sits on annotation 2 and is read as nothing;
    detection 3 overlaps annotation 3 too little (IoU 20*20 / (60*20) = 1/3) and annotation 4 not at all."""
    from manuscript_ocr_amd import Pipeline
    det = [rect(10, 10, 50, 30), rect(104, 10, 144, 30), rect(10, 60, 50, 80), rect(120, 60, 160, 80)]
    gt = [(rect(10, 10, 50, 30), "alpha"), (rect(100, 10, 140, 30)[::-1], "beta"), (rect(10, 60, 50, 80), "gamma"),
          (rect(100, 60, 140, 80), "delta"), (rect(200, 100, 240, 120), "omega")]
    img = np.full((140, 260, 3), 255, dtype=np.uint8)
    for k, q in enumerate(det):
        img[q[0][1]: q[2][1], q[0][0]: q[2][0]] = 10 + k
    pipe = Pipeline(detector=StandInDetector(det), recognizer=StandInRecognizer({10: "alpha", 11: "bexa", 12: "", 13: "delta"}))
    r = pipe.evaluate([img], [gt], iou=0.5)
    assert r["detection"] == {"precision": 3 / 4, "recall": 3 / 5, "f1": 2 * (3 / 4) * (3 / 5) / (3 / 4 + 3 / 5), "tp": 3, "fp": 1, "fn": 2}
    assert r["recognition"] == {"n": 3, "accuracy": 1 / 3, "cer_micro": (0 + 1 + 5) / (5 + 4 + 5), "cer_mean": (0 / 5 + 1 / 4 + 5 / 5) / 3}
    assert r["end_to_end"] == {"precision": 1 / 4, "recall": 1 / 5, "f1": 2 * (1 / 4) * (1 / 5) / (1 / 4 + 1 / 5)}
    rows = sorted((j, ref, hyp) for _i, j, _iou, ref, hyp in r["matches"][0])
    assert rows == [(0, "alpha", "alpha"), (1, "beta", "bexa"), (2, "gamma", "")]
    assert sorted(round(row[2], 6) for row in r["matches"][0]) == [round(36 * 20 / (40 * 20 + 4 * 20), 6), 1.0, 1.0]
    # at a stricter threshold the shifted word is lost; an empty reference read as something counts inf in cer_mean
    r = pipe.evaluate([img], [gt], iou=0.9)
    assert (r["detection"]["tp"], r["detection"]["fp"], r["detection"]["fn"]) == (2, 2, 3) and r["recognition"]["n"] == 2
    gt[0] = (gt[0][0], "")
    r = pipe.evaluate([img], [gt], iou=0.9)
    assert r["recognition"]["cer_mean"] == float("inf") and r["recognition"]["cer_micro"] == (5 + 5) / 5
    empty = pipe.evaluate([], [])
    assert empty["detection"]["f1"] == 0.0 and empty["recognition"] == {"n": 0, "accuracy": 0.0, "cer_micro": 0.0, "cer_mean": 0.0}
    with pytest.raises(ValueError):
        pipe.evaluate([img], [])


# ------------------------------------------------------------------------------------------------ the sanitizers
def test_header_under_the_sanitizers(tmp_path):
    """csrc/quad_iou.h (geometry and host matching) in a plain C++ program of its own (tests/native/quad_match_fuzz.cpp) with the
    address and undefined-behaviour sanitizers: garbage coordinates, counts at the bounds, every array in a heap block of its exact
    size.  Run as a child process; nothing is loaded into this one."""
    cxx = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cxx):
        pytest.skip("the ROCm clang++ is not available")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "quad_match_fuzz"
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(root, "manuscript_ocr_amd", "csrc"),
                           os.path.join(root, "tests", "native", "quad_match_fuzz.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe), "400"], capture_output=True, text=True, timeout=600, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.startswith("rounds 400 checked")
