"""msocr_quad_match on the MI355X against its host twin msocr_quad_match_host, which
tests/test_quad_match_cpu.py holds to the Python restatement of the rule.  Both sides do the same f64 operations in the same order:
match indices, counts and IoUs (bit for bit) are compared for equality.

Sizes straddle the kernels' own edges, named here as quad_match.hip names them: QM_TILE = 64 predictions x 64 ground truths per
workgroup of the pair phase (also the wave the match phase walks the predictions with), 256 = four tiles, and QM_CAND_CAP = 8
candidate slots per prediction, behind which a prediction is recomputed against the whole page."""
import numpy as np
import pytest

from test_quad_match_cpu import CASES, DEFAULT_T, pack, random_page, rect, same_bits

pytestmark = pytest.mark.gpu

QM_TILE = 64
QM_CAND_CAP = 8


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device_and_host(pred_pages, gt_pages, thresholds, pad_pred=None, pad_gt=None):
    from manuscript_ocr_amd import ops
    pred, n_pred = pack(pred_pages, pad_pred)
    gt, n_gt = pack(gt_pages, pad_gt)
    host = ops.quad_match_host(pred, n_pred, gt, n_gt, thresholds)
    dev = [t.cpu().numpy() for t in ops.quad_match(_dev(pred), _dev(n_pred), _dev(gt), _dev(n_gt), thresholds)]
    return dev, host, n_pred


def assert_same(dev, host, n_pred, what=""):
    assert np.array_equal(dev[2], host[2]), (what, dev[2], host[2])
    for p, n in enumerate(n_pred):
        assert np.array_equal(dev[0][p, :, :n], host[0][p, :, :n]), (what, p)
        assert same_bits(dev[1][p, :, :n], host[1][p, :, :n]), (what, p)


def pages_of(sizes, seed):
    """Pages with exactly (n_pred, n_gt) quads: a random page of the larger size, cut."""
    out = []
    for k, (a, b) in enumerate(sizes):
        pred, gt = random_page(seed + k, max(a, b) + 40, spurious=0.3)
        assert len(pred) >= a and len(gt) >= b
        out.append((pred[:a], gt[:b]))
    return [p for p, _ in out], [g for _, g in out]


@pytest.mark.parametrize("T", [1, 10, 16])
def test_ragged_batch(T):
    pred, gt = pages_of([(0, 5), (7, 0), (65, 130)], 100)
    th = np.linspace(0.3, 1.0, T) if T != 10 else DEFAULT_T
    dev, host, n = device_and_host(pred, gt, th)
    assert_same(dev, host, n)
    assert host[2][2, 0, 0] > 20 and host[2][0].tolist() == [[0, 0, 5]] * T and host[2][1].tolist() == [[0, 7, 0]] * T


@pytest.mark.parametrize("n", [QM_TILE - 1, QM_TILE, QM_TILE + 1, 4 * QM_TILE - 1, 4 * QM_TILE, 4 * QM_TILE + 1])
def test_tile_edges(n):
    pred, gt = random_page(200 + n, n, drop=0.0, spurious=0.0)  # every word predicted: the last tile's quads take part
    assert len(pred) == n and len(gt) == n
    dev, host, cnt = device_and_host([pred], [gt], DEFAULT_T)
    assert_same(dev, host, cnt)
    assert host[2][0, 0, 0] > 0.9 * n and host[2][0, -1, 0] < 0.5 * n and np.any(host[0][0, 0, QM_TILE * ((n - 1) // QM_TILE):] >= 0)


def test_special_cases():
    for name, (pred, gt, th) in CASES.items():
        dev, host, n = device_and_host(pred, gt, th)
        assert_same(dev, host, n, name)


def test_candidate_capacity():
    """More overlaps than QM_CAND_CAP slots: the recompute path gives the host's answer."""
    small = [rect(2 + 5 * (k % 20), 2 + 5 * (k // 20), 5 + 5 * (k % 20), 5 + 5 * (k // 20)) for k in range(200)]
    big = rect(0, 0, 102, 52)
    assert len(small) > QM_CAND_CAP
    th = [0.001, 0.002, 0.5]
    # one prediction over 200 small ground truths (IoU 9 / 5304 each: the smallest index wins), and the transposed page
    dev, host, n = device_and_host([[big]], [small], th)
    assert_same(dev, host, n, "1 x 200")
    assert host[2][0].tolist() == [[1, 0, 199], [0, 1, 200], [0, 1, 200]]
    dev, host, n = device_and_host([small], [[big]], th)
    assert_same(dev, host, n, "200 x 1")
    assert host[0][0, 0, :3].tolist() == [0, -1, -1] and host[2][0, 0].tolist() == [1, 199, 0]
    # sixty jittered copies of one word on each side: every prediction has sixty candidates, and the used set decides among them
    rng = np.random.default_rng(3)
    base = np.asarray(rect(100, 100, 180, 130), dtype=np.float32)
    pred = [base + rng.normal(0, 3, (4, 2)).astype(np.float32) for _ in range(60)]
    gt = [base + rng.normal(0, 3, (4, 2)).astype(np.float32) for _ in range(60)]
    for k in (QM_CAND_CAP - 1, QM_CAND_CAP, QM_CAND_CAP + 1, 60):  # ground truths on the page: below, at and above the cap
        dev, host, n = device_and_host([pred], [gt[:k]], DEFAULT_T)
        assert_same(dev, host, n, f"cluster {k}")
        assert host[2][0, 0, 0] == k
    # both paths on one page: a cluster above the cap among sparse words
    sparse_p, sparse_g = random_page(9, 100)
    dev, host, n = device_and_host([list(sparse_p[:50]) + pred + list(sparse_p[50:])], [list(gt) + list(sparse_g)], DEFAULT_T)
    assert_same(dev, host, n, "mixed")


def _grid(n, cols, pitch=60.0, jitter=0.0, seed=0):
    rng = np.random.default_rng(seed)
    k = np.arange(n)
    x0, y0 = (k % cols) * pitch, (k // cols) * pitch
    q = np.stack([np.stack([x0, y0], 1), np.stack([x0 + 40, y0], 1), np.stack([x0 + 40, y0 + 20], 1), np.stack([x0, y0 + 20], 1)], 1)
    return (q + rng.uniform(-jitter, jitter, q.shape)).astype(np.float32)


@pytest.mark.parametrize("transposed", [False, True])
def test_envelope_edge(transposed):
    """One page of 16384 x 1024 quads on a sparse grid (and 1024 x 16384): the largest page the entry point takes."""
    many = _grid(16384, 128)
    few = _grid(16384, 128, jitter=2.0, seed=1)[7::16]
    assert len(few) == 1024
    pred, gt = (few, many) if transposed else (many, few)
    dev, host, n = device_and_host([pred], [gt], [0.5, 0.9])
    assert_same(dev, host, n)
    assert host[2][0, 0, 0] > 900 and host[2][0, 0, 0] + host[2][0, 0, 1] == len(pred)
    if not transposed:
        assert np.all(np.flatnonzero(host[0][0, 0] >= 0) % 16 == 7)  # only the predictions under a ground truth match


def test_unwritten_bytes_stay():
    import torch
    from manuscript_ocr_amd import ops
    pred, gt = pages_of([(5, 9), (0, 3), (70, 64)], 300)
    P, n_pred = pack(pred, 100)
    G, n_gt = pack(gt, 90)
    th = [0.5, 0.7, 0.9]
    match = torch.full((3, 3, 100), -77, dtype=torch.int32, device="cuda")
    iou = torch.full((3, 3, 100), -77.0, dtype=torch.float64, device="cuda")
    counts = torch.full((3, 3, 3), -77, dtype=torch.int32, device="cuda")
    ops.quad_match(_dev(P), _dev(n_pred), _dev(G), _dev(n_gt), th, out=(match, iou, counts))
    dev = [t.cpu().numpy() for t in (match, iou, counts)]
    host = ops.quad_match_host(P, n_pred, G, n_gt, th)
    assert_same(dev, host, n_pred)
    for p, n in enumerate(n_pred):
        assert np.all(dev[0][p, :, n:] == -77) and np.all(dev[1][p, :, n:] == -77.0), p


def test_graph_replay():
    import torch
    from manuscript_ocr_amd import ops
    pred, gt = pages_of([(40, 50), (130, 120)], 400)
    P, n_pred = pack(pred)
    G, n_gt = pack(gt)
    Pd, npd, Gd, ngd = _dev(P), _dev(n_pred), _dev(G), _dev(n_gt)
    eager = [t.cpu().numpy() for t in ops.quad_match(Pd, npd, Gd, ngd, DEFAULT_T)]
    host = ops.quad_match_host(P, n_pred, G, n_gt, DEFAULT_T)
    assert_same(eager, host, n_pred)
    ws = torch.empty((ops.quad_match_workspace_bytes(2, P.shape[1], G.shape[1]),), dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.quad_match(Pd, npd, Gd, ngd, DEFAULT_T, workspace=ws)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.quad_match(Pd, npd, Gd, ngd, DEFAULT_T, workspace=ws)
    Gd.copy_(_dev(G[::-1].copy()))  # other inputs in the captured buffers: a replay must compute, not remember
    ngd.copy_(_dev(n_gt[::-1].copy()))
    graph.replay()
    swapped = [t.cpu().numpy() for t in out]
    assert_same(swapped, ops.quad_match_host(P, n_pred, G[::-1].copy(), n_gt[::-1].copy(), DEFAULT_T), n_pred)
    Gd.copy_(_dev(G))
    ngd.copy_(_dev(n_gt))
    for _ in range(2):
        graph.replay()
        assert_same([t.cpu().numpy() for t in out], host, n_pred)


def test_match_detections_on_the_device():
    from manuscript_ocr_amd.detectors import match_detections
    pred, gt = pages_of([(30, 35), (0, 4), (90, 80)], 500)
    scores = [np.random.default_rng(k).uniform(size=len(p)).round(1) for k, p in enumerate(pred)]
    a, b = match_detections(pred, gt, scores=scores), match_detections(pred, gt, scores=scores, device="cuda")
    assert np.array_equal(a.counts, b.counts)
    for p in range(3):
        assert np.array_equal(a.match[p], b.match[p]) and same_bits(a.iou[p], b.iou[p])


def test_east_evaluate():
    """EAST.evaluate on two synthetic pages with seeded weights: the detector's own boxes as ground truth score 1 everywhere;
    with every fifth box dropped and a quarter of the rest shifted by half their height (IoU 1/3 with their own box) the result
    equals the host twin's on the boxes predict_batch returns, and the drops show as false positives."""
    from manuscript_ocr_amd import synth
    from manuscript_ocr_amd.detectors import EAST, detection_f1, match_detections
    H, W = 512, 768
    det = EAST(state_dict=synth.east_state_dict(), target_size=(W, H), device="cuda")
    pages = [synth.synth_page(5, H, W)[0], synth.synth_page(6, H, W)[0]]
    boxes = [np.array([w.polygon for w in r["page"].blocks[0].words], dtype=np.float32).reshape(-1, 4, 2) for r in det.predict_batch(pages)]
    n = [len(b) for b in boxes]
    print("boxes per page:", n)
    assert min(n) >= 4 and max(n) >= 5  # seeded weights: a few merged boxes per page, enough to drop and to shift some
    same = det.evaluate(pages, boxes)
    assert same["n_images"] == 2 and same["n_pred"] == sum(n) and same["n_gt"] == sum(n) and len(same["thresholds"]) == 10
    assert np.all(same["precision"] == 1.0) and np.all(same["recall"] == 1.0) and same["f1_at_05"] == 1.0 and same["f1_avg"] == 1.0
    gt, n_drop, n_shift = [], 0, 0
    for b in boxes:
        keep = [k for k in range(len(b)) if k % 5 != 4]
        n_drop += len(b) - len(keep)
        g = b[keep].copy()
        h = g[:, :, 1].max(axis=1) - g[:, :, 1].min(axis=1)
        g[::4, :, 1] += 0.5 * h[::4, None]
        n_shift += len(g[::4])
        gt.append(g)
    th = [0.3, 0.5, 0.9]
    got = det.evaluate(pages, gt, thresholds=th, batch=1)
    exp = match_detections(boxes, gt, th, device=None)
    f1 = detection_f1(exp.counts, th)
    for key in ("tp", "fp", "fn", "precision", "recall", "f1"):
        assert np.array_equal(got[key], f1[key]), key
    for p in range(2):
        assert np.array_equal(got["matches"][p], exp.match[p]) and same_bits(got["ious"][p], exp.iou[p])
    print("tp / fp / fn:", got["tp"], got["fp"], got["fn"], "dropped", n_drop)
    assert n_drop >= 1 and got["n_gt"] == sum(n) - n_drop and np.all(got["fp"] >= n_drop) and np.all(got["tp"] + got["fn"] == got["n_gt"])
    # at 0.3 every kept box is found (a shifted one at IoU 1/3) and exactly the dropped ones are false positives; at 0.9 the shifted
    # quarter is lost as well
    assert (got["tp"][0], got["fp"][0], got["fn"][0]) == (got["n_gt"], n_drop, 0)
    assert (got["tp"][2], got["fp"][2], got["fn"][2]) == (got["n_gt"] - n_shift, n_drop + n_shift, n_shift)


def test_pipeline_evaluate_with_the_package_plugins():
    """Pipeline.evaluate on the device routes (EAST's device for the matching, TRBA's for the distances): the pipeline's own words as
    the annotation score 1 throughout; with every third annotated text changed by one character the detection figures stay and the
    recognition and end-to-end figures follow by count."""
    from manuscript_ocr_amd import Pipeline, synth
    from manuscript_ocr_amd.detectors import EAST
    from manuscript_ocr_amd.recognizers import TRBA
    H, W = 512, 768
    det = EAST(state_dict=synth.east_state_dict(), target_size=(W, H), device="cuda")
    rec = TRBA(state_dict=synth.trba_state_dict(194, 256, seed=20260128), config={"img_h": 32, "img_w": 100, "max_len": 25, "hidden_size": 256},
               device="cuda")
    pipe = Pipeline(detector=det, recognizer=rec)
    img = synth.synth_page(5, H, W)[0]
    words = [w for b in pipe.predict(img).blocks for w in b.words]
    gt = [(w.polygon, w.text or "") for w in words]
    n = len(gt)
    assert n >= 10
    r = pipe.evaluate([img], [gt])
    assert r["detection"] == {"precision": 1.0, "recall": 1.0, "f1": 1.0, "tp": n, "fp": 0, "fn": 0}
    assert r["recognition"] == {"n": n, "accuracy": 1.0, "cer_micro": 0.0, "cer_mean": 0.0}
    assert r["end_to_end"] == {"precision": 1.0, "recall": 1.0, "f1": 1.0}
    changed = [(q, t + "x" if k % 3 == 0 else t) for k, (q, t) in enumerate(gt)]  # one insertion: distance 1
    wrong = len(range(0, n, 3))
    r = pipe.evaluate([img], [changed])
    assert r["detection"]["tp"] == n and r["recognition"]["n"] == n
    assert r["recognition"]["accuracy"] == (n - wrong) / n and r["end_to_end"]["recall"] == (n - wrong) / n
    assert r["recognition"]["cer_micro"] == wrong / sum(len(t) for _q, t in changed)


def test_east_evaluate_behind_the_host_tail():
    """With the box tail left to the host (the route a page above the device tail's capacity takes), evaluate gives what the device
    tail route gives: the two tails return the same boxes."""
    from manuscript_ocr_amd import synth
    from manuscript_ocr_amd.detectors import EAST
    H, W = 512, 768
    det = EAST(state_dict=synth.east_state_dict(), target_size=(W, H), device="cuda")
    pages = [synth.synth_page(5, H, W)[0], synth.synth_page(6, H, W)[0]]
    gt = [np.array([w.polygon for w in r["page"].blocks[0].words], dtype=np.float32).reshape(-1, 4, 2)[1:] for r in det.predict_batch(pages)]
    a = det.evaluate(pages, gt, thresholds=[0.5, 0.8])
    det.device_tail = False
    b = det.evaluate(pages, gt, thresholds=[0.5, 0.8])
    assert a["tp"].tolist() == b["tp"].tolist() == [a["n_gt"]] * 2 and a["fp"].tolist() == b["fp"].tolist() == [2, 2]
    for p in range(2):
        assert np.array_equal(a["matches"][p], b["matches"][p]) and same_bits(a["ious"][p], b["ious"][p])
