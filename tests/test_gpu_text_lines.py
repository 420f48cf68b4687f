"""Text lines as a result on the device (Pipeline.group_lines; DESIGN.md sections 4.6 and 4.12): msocr_reading_order_lines against
msocr_reading_order_crops (the four common outputs, bit for bit), against the host twin msocr_reading_lines_host and against the
Python restatement `lines_of` of tests/test_text_lines_cpu.py (which that module pins to the oracle on every input), and the
Pipeline with the attribute set on its three routes.  Everything is integer or f64 arithmetic in the reference's written order:
every comparison is for equality.

Shapes: the smallest at which the kernel can go wrong.  One word and one line; the wave walks the lines in chunks of 64 (64, 65 and
129 lines); RO_T = 1024 threads own one position each up to n = 1024 (1190 boxes in 70 lines: two positions per thread and more
than one chunk of lines); one thread owns one line up to 1024 lines and RO_MAXLINES = 4096 is the capacity (4096 and 4097 lines).
"""
import numpy as np
import pytest
import torch

import test_text_lines_cpu as tl

pytestmark = pytest.mark.gpu

F32 = np.float32
ISENT, WSENT, WS_TAIL = -777, 0xA5, 4096
INF = float("inf")
CFG = {"img_h": 32, "img_w": 100, "max_len": 25, "hidden_size": 256}


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


@pytest.fixture(scope="module")
def ops(gpu):
    from manuscript_ocr_amd import ops as _ops
    return _ops


# ================================================================================================ the kernel
def polys_of(boxes_i):
    """Integer AABBs -> [n, 9] f32 quads whose corners carry fractions that truncate toward zero to those integers."""
    b = np.asarray(boxes_i, dtype=np.float64).reshape(-1, 4)
    x0, y0, x1, y1 = b.T
    fr = lambda v, f: v + np.where(v < 0, -f, f)
    q = np.stack([fr(x0, .25), fr(y0, .5), fr(x1, .75), fr(y0, .25), fr(x1, .5), fr(y1, .75), fr(x0, .5), fr(y1, .25), np.full(len(b), .9)], 1)
    return q.astype(F32)


def _iguard(*shape):
    return torch.full(shape, ISENT, dtype=torch.int32, device="cuda")


def run_lines(ops, pages, mc, page_hw, counts=None, page_base=0, tol=0.6, gap=INF, min_text=5, img_hw=(32, 100)):
    """pages: integer-AABB lists (None or [] = no boxes) -> per page (order, line, records, nlines, ncrop) as numpy, from the raw C
    call with one guard page behind every output and a guard tail behind the workspace.  Asserts on the way: nothing is written
    behind a page's counts or behind the last page; order / keep / desc / ncrop equal ops.reading_order_crops on the same input;
    ops.reading_order_lines gives the same bits; a flagged page has nlines = ncrop = -1 and untouched rows."""
    from manuscript_ocr_amd import _native as nat
    N = len(pages)
    a = np.full((N + 1, mc, 9), np.nan, dtype=F32)  # rows past a page's count and the page behind the last: never to be read
    for i, p in enumerate(pages):
        if p is not None and len(p):
            a[i, :len(p)] = polys_of(p)
    boxes = torch.from_numpy(a).cuda()
    cnt_l = [0 if p is None else len(p) for p in pages] if counts is None else list(counts)
    cnt = torch.tensor(cnt_l + [ISENT], dtype=torch.int32).cuda()
    L = nat.lib()
    rows = L.msocr_reading_order_line_rows(mc)
    assert rows == min(mc, 4096)
    nbytes = L.msocr_reading_order_workspace_bytes(N, mc)
    ws = torch.full((nbytes + WS_TAIL,), WSENT, dtype=torch.uint8, device="cuda")
    order, keep, desc, ncrop = _iguard(N + 1, mc), _iguard(N + 1, mc), _iguard(N + 1, mc, 8), _iguard(N + 1)
    line, lines, nlines = _iguard(N + 1, mc), _iguard(N + 1, rows, 6), _iguard(N + 1)
    rc = L.msocr_reading_order_lines(boxes.data_ptr(), cnt.data_ptr(), N, mc, page_hw[0], page_hw[1], min_text, img_hw[0], img_hw[1], tol, gap,
                                     page_base, order.data_ptr(), keep.data_ptr(), desc.data_ptr(), ncrop.data_ptr(), line.data_ptr(),
                                     lines.data_ptr(), nlines.data_ptr(), ws.data_ptr(), ops._stream())
    assert rc == 0
    torch.cuda.synchronize()
    o, k, d, c, ln, rec, nl = (t.cpu().numpy() for t in (order, keep, desc, ncrop, line, lines, nlines))
    for t in (o, k, d, c, ln, rec, nl):
        assert (t[N] == ISENT).all(), "written behind the last page"
    assert bool((ws[nbytes:] == WSENT).all()), "written behind msocr_reading_order_workspace_bytes"
    ro = ops.reading_order_crops(boxes[:N], cnt[:N], page_hw, min_text, img_hw[0], img_hw[1], page_base=page_base, y_tol_ratio=tol, x_gap_ratio=gap)
    ro2, rl2 = ops.reading_order_lines(boxes[:N], cnt[:N], page_hw, min_text, img_hw[0], img_hw[1], page_base=page_base, y_tol_ratio=tol,
                                       x_gap_ratio=gap)
    assert isinstance(ro2, ops.ReadingOrder) and isinstance(rl2, ops.ReadingLines) and rl2.lines.shape == (N, rows, 6)
    ro, ro2, rl2 = [t.cpu().numpy() for t in ro], [t.cpu().numpy() for t in ro2], [t.cpu().numpy() for t in rl2]
    assert np.array_equal(c[:N], ro[3]) and np.array_equal(c[:N], ro2[3]) and np.array_equal(nl[:N], rl2[2])
    res = []
    for n in range(N):
        nc, nln = int(c[n]), int(nl[n])
        assert (nc == -1) == (nln == -1), (n, nc, nln)
        if nc < 0:
            assert nc == nln == -1 and (ln[n] == ISENT).all() and (rec[n] == ISENT).all(), ("flagged page", n)
            res.append((None, None, None, nln, nc))
            continue
        m = max(cnt_l[n], 0)
        assert 0 <= nc <= m and 0 <= nln <= min(m, rows) and (nln > 0) == (m > 0)
        # desc is staged at the words' positions before it is compacted: defined up to nc, untouched from m on
        for got, ref, ref2, used, end in ((o, ro[0], ro2[0], m, m), (k, ro[1], ro2[1], m, m), (d, ro[2], ro2[2], nc, m), (ln, None, rl2[0], m, m),
                                          (rec, None, rl2[1], nln, nln)):
            assert (got[n, end:] == ISENT).all(), ("rows past the page's counts written", n)
            assert ref is None or np.array_equal(got[n, :used], ref[n, :used]), ("differs from reading_order_crops", n)
            assert np.array_equal(got[n, :used], ref2[n, :used]), ("ops.reading_order_lines differs from the raw call", n)
        res.append((o[n, :m].copy(), ln[n, :m].copy(), rec[n, :nln].copy(), nln, nc))
    return res


def check_page(ops, boxes, reference=True, tol=0.6, gap=INF, hw=(3000, 1200)):
    """One page alone: device == host twin (== `expected` of the restatement, with `reference`).  Returns the records."""
    eo, el, er = tl.check_twin(boxes, tol, gap, reference=reference)
    o, ln, rec, nln, nc = run_lines(ops, [boxes], len(boxes) + 3, hw, tol=tol, gap=gap)[0]
    assert nln == len(er) and np.array_equal(o, eo) and np.array_equal(ln, el) and np.array_equal(rec, er)
    return rec


@pytest.fixture(scope="module")
def text_page():
    """1190 boxes in 70 lines of 17 with its expectation from the restatement, computed once (0.7 s) and left unchanged."""
    boxes = tl.text_page()
    exp = tl.expected(boxes)
    for t in exp:
        t.setflags(write=False)
    return boxes, exp


def test_lines_smallest_pages(ops):
    rec = check_page(ops, [[30, 40, 90, 70]])
    assert rec.tolist() == [[0, 1, 30, 40, 90, 70]]
    rec = check_page(ops, [[130, 42, 190, 72], [30, 40, 90, 70]])
    assert rec.tolist() == [[0, 2, 30, 40, 190, 72]]
    rec = check_page(ops, tl.duplicate_page())
    assert rec.tolist() == [[0, 3, 10, 12, 180, 42], [3, 2, 12, 80, 170, 112]]


def test_lines_golden_cases(ops):
    """The reference-generated boxes: intersections, shrinking and duplicates included; 0 to 66 boxes, 0 to 14 lines."""
    n_lines = [len(check_page(ops, boxes)) if boxes else run_lines(ops, [boxes], 5, (3000, 1200))[0][3] for boxes in tl.golden_cases()]
    assert len(n_lines) == 9 and min(n_lines) == 0 and max(n_lines) == 14, n_lines


@pytest.mark.parametrize("L", [64, 65, 129])
def test_lines_wave_chunks(ops, L):
    """L single-word lines, shuffled: the line walk tests 64 lines per step, the L-th line opens chunk (L - 1) // 64."""
    rng = np.random.default_rng([tl.SEED, 51, L])
    ys = rng.permutation(L)
    boxes = [[int(10 + rng.integers(0, 300)), int(30 * y + 5), int(400 + rng.integers(0, 300)), int(30 * y + 25)] for y in ys]
    rec = check_page(ops, boxes, hw=(30 * L + 40, 800))
    assert len(rec) == L and (rec[:, 1] == 1).all() and rec[:, 0].tolist() == list(range(L))


def test_lines_text_page(ops, text_page):
    """n = 1190 > RO_T: two positions per thread, 70 lines in two chunks of the walk, lines of 17 words to unite."""
    boxes, (eo, el, er) = text_page
    assert len(boxes) == 1190 and len(er) == 70 and (er[:, 1] == 17).all()
    to, tline, trec = tl.check_twin(boxes, reference=False)
    assert np.array_equal(to, eo) and np.array_equal(tline, el) and np.array_equal(trec, er)
    o, ln, rec, nln, nc = run_lines(ops, [boxes], 1200, (3000, 1200))[0]
    assert nln == 70 and nc == 1190 and np.array_equal(o, eo) and np.array_equal(ln, el) and np.array_equal(rec, er)


def test_lines_tie_on_mean_cy(ops):
    """Two lines with the same mean centre y: creation order decides, in the rank as in lstart.  Once with a finite x gap (words of
    one row too far apart), once with zero-height boxes (avg_h = 0: NaN gap, every box its own line, rows shared)."""
    rec = check_page(ops, tl.tie_page(), gap=tl.TIE_GAP)
    assert rec.tolist() == [[0, 2, 0, 0, 100, 20], [2, 1, 500, 0, 550, 20], [3, 1, 5, 60, 45, 80]]
    flat = [[40, 50, 90, 50], [300, 50, 380, 50], [10, 20, 60, 20], [200, 50, 260, 50], [100, 20, 130, 20]]
    rec = check_page(ops, flat)
    assert rec[:, :2].tolist() == [[k, 1] for k in range(5)] and rec[:, 2].tolist() == [10, 100, 40, 300, 200], "ties: cy-sorted input order"


def test_lines_pages_of_one_launch(ops, text_page):
    """Pages of 0, 1190, 3 and 65 boxes and a skipped page (count -1) in one launch, page_base = 7: outputs strided by max_cand and
    by rows, the empty page has no line, the skipped page is flagged and untouched."""
    big, (eo, el, er) = text_page
    rng = np.random.default_rng([tl.SEED, 52])
    three = [[200, 10, 260, 40], [20, 12, 80, 42], [30, 90, 100, 120]]
    ys = rng.permutation(65)
    many = [[int(10 + rng.integers(0, 50)), int(30 * y + 5), int(200 + rng.integers(0, 50)), int(30 * y + 25)] for y in ys]
    pages = [[], big, three, many, None]
    res = run_lines(ops, pages, 1200, (3000, 1200), counts=[0, 1190, 3, 65, -1], page_base=7)
    assert res[0][3:] == (0, 0) and len(res[0][0]) == 0
    assert res[4][3:] == (-1, -1)
    assert np.array_equal(res[1][0], eo) and np.array_equal(res[1][1], el) and np.array_equal(res[1][2], er)
    for n in (2, 3):
        to, tline, trec = tl.check_twin(pages[n])
        assert np.array_equal(res[n][0], to) and np.array_equal(res[n][1], tline) and np.array_equal(res[n][2], trec), n
    assert res[2][2].tolist() == [[0, 2, 20, 10, 260, 42], [2, 1, 30, 90, 100, 120]] and res[3][3] == 65


def test_lines_capacity(ops):
    """RO_MAXLINES = 4096 lines are taken (rows = 4096 records, four lines per thread), 4097 flag the page in both counts.  Against
    the host twin only: the Python restatement would take minutes here."""
    boxes = [[10, 12 * i, 60, 12 * i + 8] for i in range(4097)]
    rng = np.random.default_rng([tl.SEED, 53])
    over = [boxes[i] for i in rng.permutation(4097)]
    fits = [boxes[i] for i in rng.permutation(4096)]
    to, tline, trec = tl.check_twin(fits, reference=False)
    assert len(trec) == 4096 and np.array_equal(trec[:, 3], 12 * np.arange(4096))
    res = run_lines(ops, [over, fits], 4100, (50000, 200))
    assert res[0][3:] == (-1, -1)
    o, ln, rec, nln, nc = res[1]
    assert nln == 4096 and nc == 4096 and np.array_equal(o, to) and np.array_equal(ln, tline) and np.array_equal(rec, trec)


def test_lines_entry_point_refuses_missing_outputs(ops):
    from manuscript_ocr_amd import _native as nat
    b, c = torch.zeros((1, 4, 9), device="cuda"), torch.zeros((1,), dtype=torch.int32, device="cuda")
    o, k, d, nc, ln, rec, nl = _iguard(1, 4), _iguard(1, 4), _iguard(1, 4, 8), _iguard(1), _iguard(1, 4), _iguard(1, 4, 6), _iguard(1)
    ws = torch.empty((nat.lib().msocr_reading_order_workspace_bytes(1, 4),), dtype=torch.uint8, device="cuda")
    for miss in range(3):
        outs = [ln.data_ptr(), rec.data_ptr(), nl.data_ptr()]
        outs[miss] = None
        assert nat.lib().msocr_reading_order_lines(b.data_ptr(), c.data_ptr(), 1, 4, 100, 100, 5, 32, 100, 0.6, INF, 0, o.data_ptr(), k.data_ptr(),
                                                   d.data_ptr(), nc.data_ptr(), *outs, ws.data_ptr(), ops._stream()) == -1


# ================================================================================================ the Pipeline
PH, PW = 224, 320


@pytest.fixture(scope="module")
def rec(gpu):
    from manuscript_ocr_amd import synth
    from manuscript_ocr_amd.recognizers import TRBA
    return TRBA(state_dict=synth.trba_state_dict_confident(194, 256, seed=3), config=CFG, device="cuda")


@pytest.fixture(scope="module")
def east_sd(gpu):
    from manuscript_ocr_amd import synth
    return synth.east_state_dict()


def _pages_and_maps(tilted):
    """Two pages at the smallest size the pipeline tests use, with injected maps: word rectangles, or the same words tilted."""
    from manuscript_ocr_amd import synth
    pgs, maps = [], []
    for seed in (41, 42):
        pg, rects = synth.synth_page(seed, PH, PW, line_pitch=44, word_h=22, margin=14)
        pgs.append(pg)
        if tilted:
            maps.append(synth.synth_quad_maps(synth.synth_tilted_quads(rects, seed, max_deg=6.0), (PH, PW), (PH // 4, PW // 4), seed))
        else:
            maps.append(synth.synth_maps(rects, (PH, PW), (PH // 4, PW // 4), seed))
    mo = (torch.from_numpy(np.stack([m[0] for m in maps])).cuda(), torch.from_numpy(np.stack([m[1] for m in maps])).cuda())
    return pgs, mo


def _words(page):
    return [(w.polygon, w.detection_confidence, w.text, w.recognition_confidence) for b in page.blocks for w in b.words]


def _chars(page):
    return [[(c.char, c.confidence, c.x) for c in getattr(w, "chars", [])] for b in page.blocks for w in b.words]


def _layout(page):
    """The line spans and boxes of a grouped page."""
    return [(len(b.words), b.bbox) for b in page.blocks]


def _union(words):
    pts = np.array([w.polygon for w in words], dtype=np.float64).astype(np.int32).reshape(-1, 2)
    return (int(pts[:, 0].min()), int(pts[:, 1].min()), int(pts[:, 0].max()), int(pts[:, 1].max()))


def _generic(pipe, det, pgs, mo, monkeypatch):
    """The generic route: predict() page by page with native_fast_path = False; the detector's own predict_batch gets the page's
    injected maps."""
    real_pb, k = det.predict_batch, iter(range(len(pgs)))

    def with_maps(images, **kw):
        i = next(k)
        return real_pb(images, _maps_override=(mo[0][i:i + 1], mo[1][i:i + 1]), **kw)

    monkeypatch.setattr(det, "predict_batch", with_maps)
    pipe.native_fast_path = False
    pages = [pipe.predict(p) for p in pgs]
    pipe.native_fast_path = True
    monkeypatch.setattr(det, "predict_batch", real_pb)
    return pages


def _setup(rec, east_sd, mode):
    from manuscript_ocr_amd import Pipeline
    from manuscript_ocr_amd.detectors import EAST
    tilted = mode == "rectify_crops"
    det = EAST(state_dict=east_sd, target_size=(PW, PH), device="cuda", axis_aligned_output=not tilted)
    pipe = Pipeline(det, rec)
    pipe.char_details, pipe.rectify_crops = mode == "char_details", tilted
    return pipe, det, _pages_and_maps(tilted)


def _routes(pipe, det, pgs, mo, monkeypatch):
    """The grouped pages of the three routes, and of the device route with one page flagged (its group then takes the host route)."""
    from manuscript_ocr_amd import ops
    out = {"device": pipe.predict_batch(pgs, _maps_override=mo)}
    pipe.device_order = False
    out["host"] = pipe.predict_batch(pgs, _maps_override=mo)
    pipe.device_order = True
    real, calls = ops.reading_order_lines, []

    def flagged(*args, **kw):
        ro, rl = real(*args, **kw)
        calls.append(1)
        bad = torch.tensor([-1] + [0] * (len(ro.ncrop) - 1), dtype=torch.int32, device=ro.ncrop.device)
        return ro._replace(ncrop=torch.where(bad < 0, bad, ro.ncrop)), rl._replace(nlines=torch.where(bad < 0, bad, rl.nlines))

    monkeypatch.setattr(ops, "reading_order_lines", flagged)
    out["flagged"] = pipe.predict_batch(pgs, _maps_override=mo)
    monkeypatch.setattr(ops, "reading_order_lines", real)
    assert calls == [1], "the device route goes through ops.reading_order_lines"
    out["generic"] = _generic(pipe, det, pgs, mo, monkeypatch)
    return out


MODES = ["plain", "char_details", "rectify_crops"]


@pytest.mark.parametrize("mode", MODES)
def test_pipeline_group_lines_on_every_route(gpu, rec, east_sd, monkeypatch, mode):
    """group_lines = True: the device route, device_order = False, a flagged page and native_fast_path = False return the same
    lines — the same spans and boxes over the same polygons — and on every route the flattening equals that route's run without
    the switch, words and symbols.  The device route, the host route and the flagged page also agree in every word (polygon,
    confidences, text).  Alone, with char_details (the lines hold the CharWords) and with rectify_crops on tilted quads.  The
    words of the generic route against the device route's: the next test."""
    from manuscript_ocr_amd.detectors._types import Block, CharWord, TextLine
    tilted = mode == "rectify_crops"
    pipe, det, (pgs, mo) = _setup(rec, east_sd, mode)
    off = pipe.predict_batch(pgs, _maps_override=mo)
    off_generic = _generic(pipe, det, pgs, mo, monkeypatch)
    assert all(len(p.blocks) == 1 and type(p.blocks[0]) is Block for p in off + off_generic)
    assert sum(w.text is not None for p in off for w in p.blocks[0].words) >= 8
    pipe.group_lines = True
    out = _routes(pipe, det, pgs, mo, monkeypatch)
    dev = out["device"]
    geometry = lambda p: [(w[0], w[1], w[2] is None) for w in _words(p)]
    for name, pages in out.items():
        assert len(pages) == 2
        for p in pages:
            assert len(p.blocks) >= 3 and all(type(b) is TextLine and len(b.words) >= 1 for b in p.blocks), name
            assert all(b.bbox == _union(b.words) for b in p.blocks), name
        assert [_layout(p) for p in pages] == [_layout(p) for p in dev], name
        assert [geometry(p) for p in pages] == [geometry(p) for p in off], name
    assert max(len(b.words) for p in dev for b in p.blocks) >= 2
    if tilted:
        assert any(abs(w.polygon[1][1] - w.polygon[0][1]) > 2.0 for p in dev for b in p.blocks for w in b.words)
    for name in ("device", "host", "flagged"):
        assert [_words(p) for p in out[name]] == [_words(p) for p in off], name
        assert [_chars(p) for p in out[name]] == [_chars(p) for p in off], name
    assert [_words(p) for p in out["generic"]] == [_words(p) for p in off_generic], "generic route, with and without the switch"
    if mode == "char_details":
        named = [w for p in dev for b in p.blocks for w in b.words if w.text is not None]
        assert len(named) >= 8 and all(isinstance(w, CharWord) and "".join(c.char for c in w.chars) == w.text for w in named)
    rows = pipe.get_text(dev[0]).split("\n")
    assert rows == [" ".join(w.text for w in sorted(b.words, key=lambda w: min(p[0] for p in w.polygon)) if w.text)
                    for b in dev[0].blocks if any(w.text for w in b.words)] and len(rows) >= 3
    # off again: the first run, exactly
    pipe.group_lines = False
    again = pipe.predict_batch(pgs, _maps_override=mo)
    assert [type(b) for p in again for b in p.blocks] == [Block, Block] and [_words(p) for p in again] == [_words(p) for p in off]


@pytest.mark.parametrize("mode", MODES)
def test_pipeline_group_lines_generic_route_words_equal_device_route(gpu, rec, east_sd, monkeypatch, mode):
    """group_lines = True: flattened, the pages of native_fast_path = False hold the same words as the device route's — polygon,
    confidences and text, compared for equality — and as the run without the switch.  With rectify_crops this rests on the generic
    route handing this package's recogniser the device route's canvases (Pipeline._extract_word_image)."""
    pipe, det, (pgs, mo) = _setup(rec, east_sd, mode)
    off = pipe.predict_batch(pgs, _maps_override=mo)
    pipe.group_lines = True
    dev = pipe.predict_batch(pgs, _maps_override=mo)
    generic = _generic(pipe, det, pgs, mo, monkeypatch)
    diff = [(a[2], b[2], a[3], b[3]) for p, q in zip(generic, dev) for a, b in zip(_words(p), _words(q)) if a != b]
    print(f"group_lines {mode}: generic route against device route, {len(diff)} of {sum(len(_words(p)) for p in dev)} words differ {diff[:4]}")
    assert [_layout(p) for p in generic] == [_layout(p) for p in dev]
    assert [_words(p) for p in dev] == [_words(p) for p in off]
    assert [_words(p) for p in generic] == [_words(p) for p in dev]
