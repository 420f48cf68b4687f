"""Skew-aware reading order on the device (Pipeline.deskew): msocr_reading_order_deskew against the host
twins msocr_page_skew_host + msocr_deskew_boxes_host + msocr_reading_lines_host and the restatement of tests/test_deskew_cpu.py,
against msocr_reading_order_lines where no rotation is applied (bit for bit), and the Pipeline with the attribute set on its routes.
Everything is integer or f64 arithmetic in one written order: every comparison is for equality.

Shapes: the smallest at which the kernel can go wrong.  n = 1, 7 and 8 (the word threshold); 64 and 65 (one wave of the reduction
and the first lane of the second); 1024 and 1025 (RO_T = 1024 threads own one box each, then two); the 1190-word text page turned
by 3 degrees; 1024 words 280 000 px wide (the int64 sums pass 2^32); 4096 and 4097 lines (the capacity: the second page is flagged).
"""
import math

import numpy as np
import pytest
import torch

import test_deskew_cpu as dk
import test_gpu_text_lines as gt

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
def _guard(shape, dtype=torch.int32):
    return torch.full(shape, ISENT, dtype=dtype, device="cuda")


def expected_page(ops, quads, page_hw, page, min_text=5, img_hw=(32, 100)):
    """One page through the twins: (order, line, records, keep, desc, skew, cs); skew, cs and the ordering boxes are pinned to the
    restatement on the way."""
    q = np.asarray(quads, dtype=F32).reshape(-1, 4, 2)
    skew, cs, _boxes = dk.check_twins(q, page_hw)
    order, line, recs, _s = dk.deskewed_lines(q, page_hw)
    own = dk.trunc_boxes(q)[order].astype(np.int64)
    big = ((own[:, 2] - own[:, 0]) >= min_text) & ((own[:, 3] - own[:, 1]) >= min_text)
    desc, kept = ops.crop_descriptors(own[big], [page] * int(big.sum()), page_hw, *img_hw)
    keep = np.zeros(len(q), dtype=np.int32)
    keep[np.flatnonzero(big)[kept]] = 1
    return order, line, recs, keep, desc, skew, cs


def run_deskew(ops, pages, mc, page_hw, counts=None, page_base=0, with_lines=True, min_text=5, img_hw=(32, 100)):
    """pages: per page quads [n,4,2] (None or empty = no boxes) -> per page (order, line, records, nlines, ncrop, skew, cs) as
    numpy, from the raw C call with one guard page behind every output and a guard tail behind the workspace.  Asserts on the way:
    nothing is written behind a page's counts or behind the last page; a flagged page has nlines = ncrop = -1 and untouched rows,
    skew and cs included; every other page equals the twins in every output; ops.reading_order_deskew gives the same bits; a page
    whose rotation is not applied equals msocr_reading_order_lines."""
    from manuscript_ocr_amd import _native as nat
    N = len(pages)
    a = np.full((N + 1, mc, 9), np.nan, dtype=F32)  # rows past a page's count and the page behind the last: never to be read
    for i, p in enumerate(pages):
        if p is not None and len(p):
            a[i, :len(p), :8] = np.asarray(p, dtype=F32).reshape(-1, 8)
            a[i, :len(p), 8] = 0.9
    boxes = torch.from_numpy(a).cuda()
    cnt_l = [0 if p is None else len(p) for p in pages] if counts is None else list(counts)
    cnt = torch.tensor(cnt_l + [ISENT], dtype=torch.int32).cuda()
    L = nat.lib()
    rows = L.msocr_reading_order_line_rows(mc)
    nbytes = L.msocr_reading_order_deskew_workspace_bytes(N, mc)
    assert nbytes == L.msocr_reading_order_workspace_bytes(N, mc) + N * 16 * min(mc, 16384)
    ws = torch.full((nbytes + WS_TAIL,), WSENT, dtype=torch.uint8, device="cuda")
    order, keep, desc, ncrop = _guard((N + 1, mc)), _guard((N + 1, mc)), _guard((N + 1, mc, 8)), _guard((N + 1,))
    line, lines, nlines = _guard((N + 1, mc)), _guard((N + 1, rows, 6)), _guard((N + 1,))
    skew, cs = _guard((N + 1, 4), torch.int64), _guard((N + 1, 2), torch.float64)
    louts = [line.data_ptr(), lines.data_ptr(), nlines.data_ptr()] if with_lines else [None, None, None]
    rc = L.msocr_reading_order_deskew(boxes.data_ptr(), cnt.data_ptr(), N, mc, page_hw[0], page_hw[1], min_text, img_hw[0], img_hw[1], 0.6, INF,
                                      page_base, order.data_ptr(), keep.data_ptr(), desc.data_ptr(), ncrop.data_ptr(), *louts,
                                      skew.data_ptr(), cs.data_ptr(), ws.data_ptr(), ops._stream())
    assert rc == 0
    torch.cuda.synchronize()
    o, k, d, c, ln, rec, nl, sk, csn = (t.cpu().numpy() for t in (order, keep, desc, ncrop, line, lines, nlines, skew, cs))
    for t in (o, k, d, c, ln, rec, nl, sk, csn):
        assert (t[N] == ISENT).all(), "written behind the last page"
    assert bool((ws[nbytes:] == WSENT).all()), "written behind msocr_reading_order_deskew_workspace_bytes"
    if not with_lines:
        assert (ln == ISENT).all() and (rec == ISENT).all() and (nl == ISENT).all()
    ro2, rl2, sk2 = ops.reading_order_deskew(boxes[:N], cnt[:N], page_hw, min_text, img_hw[0], img_hw[1], page_base=page_base, lines=with_lines)
    assert isinstance(ro2, ops.ReadingOrder) and isinstance(sk2, ops.PageSkew) and (rl2 is None) == (not with_lines)
    ro2, sk2 = [t.cpu().numpy() for t in ro2], [t.cpu().numpy() for t in sk2]
    rl2 = [t.cpu().numpy() for t in rl2] if with_lines else None
    plain = None
    if with_lines:
        plain = [t.cpu().numpy() for pair in ops.reading_order_lines(boxes[:N], cnt[:N], page_hw, min_text, img_hw[0], img_hw[1], page_base=page_base)
                 for t in pair]
    assert np.array_equal(c[:N], ro2[3])
    res = []
    for n in range(N):
        nc = int(c[n])
        if nc < 0:
            assert nc == -1 and (sk[n] == ISENT).all() and (csn[n] == ISENT).all(), ("flagged page: skew / cs written", n)
            assert (ln[n] == ISENT).all() and (rec[n] == ISENT).all() and (not with_lines or nl[n] == -1), ("flagged page", n)
            res.append((None, None, None, -1, -1, None, None))
            continue
        m = max(cnt_l[n], 0)
        eo, el, er, ek, ed, es, ec = expected_page(ops, np.zeros((0, 4, 2)) if m == 0 else pages[n], page_hw, page_base + n, min_text, img_hw)
        assert nc == len(ed) and np.array_equal(sk[n], es) and np.array_equal(csn[n], ec), (n, sk[n], es)
        assert np.array_equal(sk2[0][n], es) and np.array_equal(sk2[1][n], ec)
        for got, exp, got2, used, end in ((o, eo, ro2[0], m, m), (k, ek, ro2[1], m, m), (d, ed, ro2[2], nc, m)):
            assert (got[n, end:] == ISENT).all(), ("rows past the page's counts written", n)
            assert np.array_equal(got[n, :used], exp), ("differs from the twins", n)
            assert np.array_equal(got2[n, :used], exp), ("ops.reading_order_deskew differs from the raw call", n)
        nln = -2
        if with_lines:
            nln = int(nl[n])
            assert nln == len(er) and nln == int(rl2[2][n]) and (ln[n, m:] == ISENT).all() and (rec[n, nln:] == ISENT).all()
            assert np.array_equal(ln[n, :m], el) and np.array_equal(rec[n, :nln], er), ("lines differ from the twins", n)
            assert np.array_equal(rl2[0][n, :m], el) and np.array_equal(rl2[1][n, :nln], er)
            if not es[3]:  # no rotation: msocr_reading_order_lines, bit for bit
                po, pk, pd, pc, pl, pr, pn = plain
                assert pc[n] == nc and pn[n] == nln and np.array_equal(po[n, :m], o[n, :m]) and np.array_equal(pk[n, :m], k[n, :m])
                assert np.array_equal(pd[n, :nc], d[n, :nc]) and np.array_equal(pl[n, :m], ln[n, :m]) and np.array_equal(pr[n, :nln], rec[n, :nln])
        res.append((o[n, :m].copy(), ln[n, :m].copy(), rec[n, :max(nln, 0)].copy(), nln, nc, sk[n].copy(), csn[n].copy()))
    return res


def n_words(n, deg, page_hw=(1400, 2000), seed=0):
    """n words of 40 x 20 at pitch 56 x 36, up to 32 per line, turned rigidly by deg."""
    cols = min(n, 32)
    q, _t = dk.grid_page(-(-n // cols), cols, deg, page_hw, word_wh=(40.0, 20.0), pitch=(56.0, 36.0), seed=seed, shuffle=False)
    return q[:n][np.random.default_rng([dk.SEED, n, seed]).permutation(n)]


@pytest.mark.parametrize("n", [1, 7, 8, 64, 65, 1024, 1025])
def test_deskew_kernel_sizes(ops, n):
    hw = (1400, 2000)
    q = n_words(n, 3.0, hw, seed=n)
    o, ln, rec, nln, nc, skew, cs = run_deskew(ops, [q], n + 3, hw)[0]
    assert skew[2] == n and skew[3] == (1 if n >= 8 else 0) and nc == n
    if n >= 64:
        assert nln == -(-n // 32) and (rec[:-1, 1] == 32).all(), "the lines of the deskewed frame are the grid's rows"
    run_deskew(ops, [q], n + 3, hw, with_lines=False)


def test_deskew_kernel_text_page(ops):
    """n = 1190 > RO_T turned by 3 degrees: 70 lines of 17 in the deskewed frame, none of them in the page frame."""
    hw = (3000, 1200)
    q = dk.text_page_quads(3.0, hw)
    o, ln, rec, nln, nc, skew, cs = run_deskew(ops, [q], 1200, hw)[0]
    assert len(q) == 1190 and skew[2] == 1190 and skew[3] == 1 and nln == 70 and (rec[:, 1] == 17).all()
    plain = ops.reading_lines_host(dk.trunc_boxes(q))
    assert len(plain[2]) != 70 and not np.array_equal(plain[0], o)


def test_deskew_kernel_sums_past_two_to_the_32(ops):
    q = dk.wide_page()
    o, ln, rec, nln, nc, skew, cs = run_deskew(ops, [q], 1024, dk.WIDE_HW)[0]
    assert skew[0] > 2 ** 32 and skew[2] == 1024 and skew[3] == 1 and nln == 1024 and (rec[:, 1] == 1).all()


def test_deskew_kernel_pages_of_one_launch(ops):
    """Pages of 0, 1190, 3 and 65 boxes and a skipped page (count -1) in one launch, page_base = 7."""
    hw = (3000, 1200)
    pages = [None, dk.text_page_quads(3.0, hw), n_words(3, 3.0, hw), n_words(65, -4.0, hw, seed=2), None]
    res = run_deskew(ops, pages, 1200, hw, counts=[0, 1190, 3, 65, -1], page_base=7)
    assert res[0][3:5] == (0, 0) and res[0][5].tolist() == [0, 0, 0, 0] and res[0][6].tolist() == [1.0, 0.0]
    assert res[4][3:5] == (-1, -1)
    assert res[1][3] == 70 and res[1][5][3] == 1 and res[2][5][3] == 0 and res[3][5][3] == 1 and res[3][5][1] < 0
    run_deskew(ops, pages, 1200, hw, counts=[0, 1190, 3, 65, -1], page_base=7, with_lines=False)


def test_deskew_kernel_line_capacity(ops):
    """4096 single-word lines of a skewed page are taken, 4097 flag the page: its skew and cs rows stay untouched."""
    col = np.stack([np.array([[10.0, 12.0 * i], [60.0, 12.0 * i + 3], [60.0, 12.0 * i + 11], [10.0, 12.0 * i + 8]]) for i in range(4097)]).astype(F32)
    rng = np.random.default_rng([dk.SEED, 53])
    over, fits = col[rng.permutation(4097)], col[rng.permutation(4096)]
    res = run_deskew(ops, [over, fits], 4100, (50000, 200))
    assert res[0][3:5] == (-1, -1)
    assert res[1][3] == 4096 and res[1][4] == 4096 and res[1][5][3] == 1


def test_deskew_kernel_upright_pages_equal_reading_order_lines(ops):
    """Exact rectangles: applied = 0, and the seven outputs of msocr_reading_order_lines bit for bit (run_deskew asserts it)."""
    def rects_of(boxes):
        b = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
        return (np.stack([b[:, [0, 1]], b[:, [2, 1]], b[:, [2, 3]], b[:, [0, 3]]], axis=1) + 0.25).astype(F32)

    pages = [rects_of(gt.tl.text_page()), rects_of(gt.tl.duplicate_page()), rects_of(gt.tl.envelope_pages()["page_edges"])]
    res = run_deskew(ops, pages, 1200, (600, 900))
    assert [int(r[5][3]) for r in res] == [0, 0, 0] and [int(r[5][1]) for r in res] == [0, 0, 0] and res[0][3] == 70


def test_deskew_entry_point_refuses_missing_outputs(ops):
    from manuscript_ocr_amd import _native as nat
    L = nat.lib()
    b, c = torch.zeros((1, 4, 9), device="cuda"), torch.zeros((1,), dtype=torch.int32, device="cuda")
    o, k, d, nc, ln, rec, nl = _guard((1, 4)), _guard((1, 4)), _guard((1, 4, 8)), _guard((1,)), _guard((1, 4)), _guard((1, 4, 6)), _guard((1,))
    sk, cs = _guard((1, 4), torch.int64), _guard((1, 2), torch.float64)
    ws = torch.empty((L.msocr_reading_order_deskew_workspace_bytes(1, 4),), dtype=torch.uint8, device="cuda")
    call = lambda louts, souts: L.msocr_reading_order_deskew(b.data_ptr(), c.data_ptr(), 1, 4, 100, 100, 5, 32, 100, 0.6, INF, 0, o.data_ptr(),
                                                             k.data_ptr(), d.data_ptr(), nc.data_ptr(), *louts, *souts, ws.data_ptr(), ops._stream())
    full, sfull = [ln.data_ptr(), rec.data_ptr(), nl.data_ptr()], [sk.data_ptr(), cs.data_ptr()]
    for miss in range(3):
        louts = list(full)
        louts[miss] = None
        assert call(louts, sfull) == -1
    assert call(full, [None, cs.data_ptr()]) == -1 and call(full, [sk.data_ptr(), None]) == -1
    assert call(full, sfull) == 0 and call([None] * 3, sfull) == 0
    torch.cuda.synchronize()


# ================================================================================================ the Pipeline
PH, PW, DEG = 352, 1024, 5.0


@pytest.fixture(scope="module")
def rec(gpu):
    from manuscript_ocr_amd import synth
    from manuscript_ocr_amd.recognizers import TRBA
    return TRBA(state_dict=synth.trba_state_dict_confident(194, 256, seed=3), config=CFG, device="cuda")


@pytest.fixture(scope="module")
def east_sd(gpu):
    from manuscript_ocr_amd import synth
    return synth.east_state_dict()


def _pages_and_maps():
    """Two pages 1024 px wide whose words are turned rigidly by 5 degrees about the page centre: a line drifts by 80 px from end to
    end against a line pitch of 44, so the page-frame rule interleaves neighbouring lines."""
    from manuscript_ocr_amd import synth
    pgs, maps = [], []
    for seed in (41, 42):
        pg, rects = synth.synth_page(seed, PH, PW, line_pitch=44, word_h=22, margin=60)
        r = np.asarray(rects, dtype=np.float64)
        quads = dk.turn(np.stack([r[:, [0, 1]], r[:, [2, 1]], r[:, [2, 3]], r[:, [0, 3]]], axis=1), DEG, (0.5 * PW, 0.5 * PH))
        pgs.append(pg)
        maps.append(synth.synth_quad_maps(quads, (PH, PW), (PH // 4, PW // 4), seed))
    mo = (torch.from_numpy(np.stack([m[0] for m in maps])).cuda(), torch.from_numpy(np.stack([m[1] for m in maps])).cuda())
    return pgs, mo


def _routes(pipe, det, pgs, mo, monkeypatch):
    from manuscript_ocr_amd import ops
    out = {"device": pipe.predict_batch(pgs, _maps_override=mo)}
    pipe.device_order = False
    out["host"] = pipe.predict_batch(pgs, _maps_override=mo)
    pipe.device_order = True
    real, calls = ops.reading_order_deskew, []

    def flagged(*args, **kw):
        ro, rl, sk = real(*args, **kw)
        calls.append(1)
        bad = torch.tensor([-1] + [0] * (len(ro.ncrop) - 1), dtype=torch.int32, device=ro.ncrop.device)
        return ro._replace(ncrop=torch.where(bad < 0, bad, ro.ncrop)), rl, sk

    monkeypatch.setattr(ops, "reading_order_deskew", flagged)
    out["flagged"] = pipe.predict_batch(pgs, _maps_override=mo)
    monkeypatch.setattr(ops, "reading_order_deskew", real)
    assert calls == [1], "the device route goes through ops.reading_order_deskew"
    out["generic"] = gt._generic(pipe, det, pgs, mo, monkeypatch)
    return out


@pytest.mark.parametrize("mode", ["plain", "group_lines", "rectify_crops+char_details"])
def test_pipeline_deskew_on_every_route(gpu, rec, east_sd, monkeypatch, mode):
    from manuscript_ocr_amd import Pipeline
    from manuscript_ocr_amd.detectors import EAST
    from manuscript_ocr_amd.detectors._types import Page, SkewPage, TextLine
    det = EAST(state_dict=east_sd, target_size=(PW, PH), device="cuda", axis_aligned_output=False)
    pipe = Pipeline(det, rec)
    pipe.group_lines = mode == "group_lines"
    pipe.rectify_crops = pipe.char_details = mode == "rectify_crops+char_details"
    pgs, mo = _pages_and_maps()
    off = pipe.predict_batch(pgs, _maps_override=mo)
    off_generic = gt._generic(pipe, det, pgs, mo, monkeypatch)
    assert all(type(p) is Page for p in off + off_generic)
    assert sum(w.text is not None for p in off for b in p.blocks for w in b.words) >= 16
    pipe.deskew = True
    out = _routes(pipe, det, pgs, mo, monkeypatch)
    dev = out["device"]
    polys = lambda pages: [[w.polygon for b in p.blocks for w in b.words] for p in pages]
    assert all(a != b for a, b in zip(polys(dev), polys(off))), "the plain order of these pages differs from the deskewed one"
    for p in dev:
        assert type(p) is SkewPage and abs(p.skew_deg - DEG) < 1.0, p.skew_deg
        # line-major in the deskewed frame: turned back, the centres descend line by line and run left to right inside a line
        c = dk.turn(np.array([np.mean(w.polygon, axis=0) for b in p.blocks for w in b.words]), -p.skew_deg, (0.5 * PW, 0.5 * PH))
        brk = np.flatnonzero(np.diff(c[:, 0]) < 0)
        assert len(brk) >= 3 and (np.diff(c[:, 1])[brk] > 22).all() and (np.abs(np.delete(np.diff(c[:, 1]), brk)) < 12).all()
    for name, pages in out.items():
        assert [type(p) for p in pages] == [SkewPage, SkewPage], name
        assert polys(pages) == polys(dev), name
        assert [gt._layout(p) if pipe.group_lines else len(p.blocks) for p in pages] == [gt._layout(p) if pipe.group_lines else 1 for p in dev], name
        assert [p.skew_deg for p in pages] == [p.skew_deg for p in dev], name
        ref = off_generic if name == "generic" else off
        key = lambda pages: [sorted(map(repr, gt._words(p))) for p in pages]
        assert key(pages) == key(ref), (name, "the words of the run without the switch, permuted")
        if pipe.char_details and name != "generic":
            chars = lambda pages: [sorted(map(repr, zip(gt._words(p), gt._chars(p)))) for p in pages]
            assert chars(pages) == chars(off), name
    for name in ("host", "flagged"):
        assert [gt._words(p) for p in out[name]] == [gt._words(p) for p in dev], name
    if pipe.group_lines:
        for p in dev:
            assert len(p.blocks) >= 3 and all(type(b) is TextLine and b.bbox == gt._union(b.words) for b in p.blocks)
            assert max(len(b.words) for b in p.blocks) >= 3
    pipe.deskew = False
    again = pipe.predict_batch(pgs, _maps_override=mo)
    assert all(type(p) is Page for p in again) and [gt._words(p) for p in again] == [gt._words(p) for p in off]
    assert [gt._chars(p) for p in again] == [gt._chars(p) for p in off]
    assert [gt._layout(p) if pipe.group_lines else 0 for p in again] == [gt._layout(p) if pipe.group_lines else 0 for p in off]
