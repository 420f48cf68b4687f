"""Column-aware reading order on the device (Pipeline.columns): msocr_reading_order_regions against the host
twin msocr_reading_regions_host (which tests/test_regions_cpu.py holds to the restatement of the definition), against
msocr_reading_order_lines / msocr_reading_order_deskew where the page ends as one region (bit for bit), and the Pipeline with the
attribute set on its routes.  Everything is integer or f64 arithmetic in one written order: every comparison is for equality.

Shapes: the smallest at which the kernel can go wrong.  n = 1 and 2; 63, 64 and 65 (one wave of the reductions and the first lane of
the second); 1024 and 1025 (RO_T = 1024 threads own one word each, then two); the threshold edges; 256 and 257 regions and 4096 and
4097 lines (the capacities); five pages of one launch; one page of 16384 words, the kernel's word capacity.
"""
import numpy as np
import pytest
import torch

import test_deskew_cpu as dk
import test_gpu_text_lines as gt
import test_regions_cpu as rc

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


def _own_records(recs, own_at_pos):
    out = recs.copy()
    for r in out:
        seg = own_at_pos[r[0]:r[0] + r[1]]
        r[2:4], r[4:6] = seg[:, :2].min(axis=0), seg[:, 2:].max(axis=0)
    return out


def expected_page(ops, quads, page_hw, page, deskew, ratios, min_text=5, img_hw=(32, 100)):
    """One page through the twins: (order, line, line records, region, region records, keep, desc, skew, cs)."""
    q = np.asarray(quads, dtype=F32).reshape(-1, 4, 2)
    own = dk.trunc_boxes(q)
    skew, cs = ops.page_skew_host(q) if deskew else (None, None)
    seen = ops.deskew_boxes_host(q, page_hw, skew, cs) if deskew else own
    order, line, lrecs, region, rrecs = ops.reading_regions_host(seen, 0.6, INF, *ratios)
    at_pos = own[order].astype(np.int64)
    big = ((at_pos[:, 2] - at_pos[:, 0]) >= min_text) & ((at_pos[:, 3] - at_pos[:, 1]) >= min_text)
    desc, kept = ops.crop_descriptors(at_pos[big], [page] * int(big.sum()), page_hw, *img_hw)
    keep = np.zeros(len(q), dtype=np.int32)
    keep[np.flatnonzero(big)[kept]] = 1
    return order, line, _own_records(lrecs, own[order]), region, _own_records(rrecs, own[order]), keep, desc, skew, cs


def run_regions(ops, pages, mc, page_hw, counts=None, page_base=0, with_lines=True, deskew=False, ratios=rc.DEFAULTS, quads=False,
                min_text=5, img_hw=(32, 100)):
    """pages: per page integer boxes [n,4] (quads=True: quads [n,4,2]; None or empty = no boxes) -> per page (order, line, line
    records, region, region records, nlines, nregions, ncrop) as numpy, from the raw C call with one guard page behind every output
    and a guard tail behind the workspace.  Asserts on the way: nothing is written behind a page's counts or behind the last page; a
    flagged page has nlines = nregions = ncrop = -1 and untouched rows; every other page equals the twins in every output;
    ops.reading_order_regions gives the same bits; a page of one region equals msocr_reading_order_lines (deskew:
    msocr_reading_order_deskew) bit for bit."""
    from manuscript_ocr_amd import _native as nat
    N = len(pages)
    a = np.full((N + 1, mc, 9), np.nan, dtype=F32)  # rows past a page's count and the page behind the last: never to be read
    for i, p in enumerate(pages):
        if p is not None and len(p):
            a[i, :len(p)] = gt.polys_of(p) if not quads else np.concatenate([np.asarray(p, dtype=F32).reshape(-1, 8), np.full((len(p), 1), 0.9, F32)], 1)
    boxes = torch.from_numpy(a).cuda()
    cnt_l = [0 if p is None else len(p) for p in pages] if counts is None else list(counts)
    cnt = torch.tensor(cnt_l + [ISENT], dtype=torch.int32).cuda()
    L = nat.lib()
    rows, rrows = L.msocr_reading_order_line_rows(mc), L.msocr_reading_order_region_rows(mc)
    assert rrows == min(mc, 256)
    nbytes = L.msocr_reading_order_regions_workspace_bytes(N, mc)
    ws = torch.full((nbytes + WS_TAIL,), WSENT, dtype=torch.uint8, device="cuda")
    order, keep, desc, ncrop = _guard((N + 1, mc)), _guard((N + 1, mc)), _guard((N + 1, mc, 8)), _guard((N + 1,))
    line, lines, nlines = _guard((N + 1, mc)), _guard((N + 1, rows, 6)), _guard((N + 1,))
    region, regions, nregions = _guard((N + 1, mc)), _guard((N + 1, rrows, 6)), _guard((N + 1,))
    skew, cs = _guard((N + 1, 4), torch.int64), _guard((N + 1, 2), torch.float64)
    louts = [line.data_ptr(), lines.data_ptr(), nlines.data_ptr()] if with_lines else [None, None, None]
    souts = [skew.data_ptr(), cs.data_ptr()] if deskew else [None, None]
    ret = L.msocr_reading_order_regions(boxes.data_ptr(), cnt.data_ptr(), N, mc, page_hw[0], page_hw[1], min_text, img_hw[0], img_hw[1], 0.6, INF,
                                        page_base, *ratios, 1 if deskew else 0, order.data_ptr(), keep.data_ptr(), desc.data_ptr(),
                                        ncrop.data_ptr(), *louts, *souts, region.data_ptr(), regions.data_ptr(), nregions.data_ptr(),
                                        ws.data_ptr(), ops._stream())
    assert ret == 0
    torch.cuda.synchronize()
    o, k, d, c, ln, rec, nl, rg, rrec, nr, sk, csn = (t.cpu().numpy() for t in (order, keep, desc, ncrop, line, lines, nlines, region, regions,
                                                                                 nregions, skew, cs))
    for t in (o, k, d, c, ln, rec, nl, rg, rrec, nr, sk, csn):
        assert (t[N] == ISENT).all(), "written behind the last page"
    assert bool((ws[nbytes:] == WSENT).all()), "written behind msocr_reading_order_regions_workspace_bytes"
    if not with_lines:
        assert (ln == ISENT).all() and (rec == ISENT).all() and (nl == ISENT).all()
    if not deskew:
        assert (sk == ISENT).all() and (csn == ISENT).all()
    ro2, rl2, sk2, rg2 = ops.reading_order_regions(boxes[:N], cnt[:N], page_hw, min_text, img_hw[0], img_hw[1], page_base, 0.6, INF, *ratios,
                                                   lines=with_lines, deskew=deskew)
    assert isinstance(ro2, ops.ReadingOrder) and isinstance(rg2, ops.ReadingRegions) and (rl2 is None) == (not with_lines) and (sk2 is None) == (not deskew)
    ro2, rg2 = [t.cpu().numpy() for t in ro2], [t.cpu().numpy() for t in rg2]
    rl2 = [t.cpu().numpy() for t in rl2] if with_lines else None
    plain = None
    if with_lines and deskew:
        pro, prl, _psk = ops.reading_order_deskew(boxes[:N], cnt[:N], page_hw, min_text, img_hw[0], img_hw[1], page_base=page_base)
        plain = [t.cpu().numpy() for t in pro + prl]
    elif with_lines:
        plain = [t.cpu().numpy() for pair in ops.reading_order_lines(boxes[:N], cnt[:N], page_hw, min_text, img_hw[0], img_hw[1], page_base=page_base)
                 for t in pair]
    assert np.array_equal(c[:N], ro2[3]) and np.array_equal(nr[:N], rg2[2])
    res = []
    for n in range(N):
        nc, nrg = int(c[n]), int(nr[n])
        assert (nc == -1) == (nrg == -1), (n, nc, nrg)
        if nc < 0:
            assert (rg[n] == ISENT).all() and (rrec[n] == ISENT).all() and (sk[n] == ISENT).all() and (csn[n] == ISENT).all(), ("flagged page", n)
            assert (ln[n] == ISENT).all() and (rec[n] == ISENT).all() and (not with_lines or nl[n] == -1), ("flagged page", n)
            res.append((None, None, None, None, None, -1, -1, -1))
            continue
        m = max(cnt_l[n], 0)
        src = np.zeros((0, 4, 2)) if m == 0 else (a[n, :m, :8].reshape(-1, 4, 2))
        eo, el, er, eg, egr, ek, ed, es, ec = expected_page(ops, src, page_hw, page_base + n, deskew, ratios, min_text, img_hw)
        assert nc == len(ed) and nrg == len(egr), (n, nc, len(ed), nrg, len(egr))
        if deskew:
            assert np.array_equal(sk[n], es) and np.array_equal(csn[n], ec), (n, sk[n], es)
        for got, exp, got2, used, end in ((o, eo, ro2[0], m, m), (k, ek, ro2[1], m, m), (d, ed, ro2[2], nc, m), (rg, eg, rg2[0], m, m),
                                          (rrec, egr, rg2[1], nrg, nrg)):
            assert (got[n, end:] == ISENT).all(), ("rows past the page's counts written", n)
            assert np.array_equal(got[n, :used], exp), ("differs from the twins", n)
            assert np.array_equal(got2[n, :used], exp), ("ops.reading_order_regions differs from the raw call", n)
        nln = -2
        if with_lines:
            nln = int(nl[n])
            assert nln == len(er) and nln == int(rl2[2][n]) and (ln[n, m:] == ISENT).all() and (rec[n, nln:] == ISENT).all()
            assert np.array_equal(ln[n, :m], el) and np.array_equal(rec[n, :nln], er), ("lines differ from the twins", n)
            assert np.array_equal(rl2[0][n, :m], el) and np.array_equal(rl2[1][n, :nln], er)
            if nrg <= 1:  # one region: the kernel without the cut, bit for bit
                po, pk, pd, pc, pl, pr, pn = plain
                assert pc[n] == nc and pn[n] == nln and np.array_equal(po[n, :m], o[n, :m]) and np.array_equal(pk[n, :m], k[n, :m])
                assert np.array_equal(pd[n, :nc], d[n, :nc]) and np.array_equal(pl[n, :m], ln[n, :m]) and np.array_equal(pr[n, :nln], rec[n, :nln])
        res.append((o[n, :m].copy(), ln[n, :m].copy(), rec[n, :max(nln, 0)].copy(), rg[n, :m].copy(), rrec[n, :nrg].copy(), nln, nrg, nc))
    return res


def two_columns(n, seed=0):
    """The first n words, column-major, of a two-column page of 4 words a line, in shuffled detector order."""
    b, _t = rc.layout_page(cols=2, lines=-(-n // 8), per_line=4, stagger=18, seed=seed, shuffle=False)
    return b[:n][np.random.default_rng([rc.SEED, n, seed]).permutation(n)]


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1024, 1025])
def test_regions_kernel_sizes(ops, n):
    b = two_columns(n, seed=n)
    hw = (int(b[:, 3].max()) + 50, 600)
    o, ln, rec, rg, rrec, nln, nrg, nc = run_regions(ops, [b], n + 3, hw)[0]
    assert nc == n and nrg == (2 if n >= 63 else 1) and int(rrec[:, 1].sum()) == n
    if n >= 63:
        assert rrec[0, 4] < rrec[1, 2], "the left column is read first"
    run_regions(ops, [b], n + 3, hw, with_lines=False)


@pytest.mark.parametrize("name", list(rc.edge_pages()))
def test_regions_kernel_threshold_edges(ops, name):
    boxes, nreg = rc.edge_pages()[name]
    assert run_regions(ops, [boxes], 8, (400, 400))[0][6] == nreg


def test_regions_kernel_depth_limit(ops):
    pages = [np.asarray(rc.nested_page(d)) for d in (5, 6, 7)]
    lo = min(int(p[:, :2].min()) for p in pages)
    pages = [p - lo + 5 for p in pages]
    res = run_regions(ops, pages, max(len(p) for p in pages) + 1, (1200, 1200))
    assert [r[6] for r in res] == [7, 8, 7]


def isolated_grid(n):
    """n words 40 x 20 at pitch 100 x 60, 16 to a row, column-major: every word is cut off on all sides (gx = 40, gy = 30)."""
    i = np.arange(n)
    return np.stack([10 + 100 * (i // 16), 10 + 60 * (i % 16), 50 + 100 * (i // 16), 30 + 60 * (i % 16)], 1)


def test_regions_kernel_region_capacity(ops):
    rng = np.random.default_rng([rc.SEED, 256])
    res = run_regions(ops, [isolated_grid(257)[rng.permutation(257)], isolated_grid(256)[rng.permutation(256)]], 300, (1100, 1800))
    assert res[0][5:] == (-1, -1, -1)
    assert res[1][6] == 256 and res[1][5] == 256 and res[1][7] == 256 and (res[1][4][:, 1] == 1).all()


def test_regions_kernel_line_capacity(ops):
    """4096 single-word lines over two regions are taken, 4097 flag the page."""
    def cols(n_left, n_right):
        k = np.arange(max(n_left, n_right))
        left = np.stack([10 + 0 * k, 5 + 25 * k, 60 + 0 * k, 25 + 25 * k], 1)[:n_left]
        right = np.stack([200 + 0 * k, 5 + 25 * k, 250 + 0 * k, 25 + 25 * k], 1)[:n_right]
        both = np.concatenate([left, right])
        return both[np.random.default_rng([rc.SEED, n_left, n_right]).permutation(len(both))]

    res = run_regions(ops, [cols(2048, 2049), cols(2048, 2048)], 4100, (52000, 300))
    assert res[0][5:] == (-1, -1, -1)
    assert res[1][5:] == (4096, 2, 4096) and res[1][4][:, 1].tolist() == [2048, 2048]


def test_regions_kernel_pages_of_one_launch(ops):
    """An empty page, a four-column page, a skipped page (count -1), a one-region page and a headed page in one launch, page_base = 7."""
    four, t4 = rc.layout_page(**rc.LAYOUTS["a four-column spread"])
    head, th = rc.layout_page(**rc.LAYOUTS["a heading over two columns with a footer"])
    pages = [None, four, None, np.asarray(rc.tl.text_page(lines=20, per_line=10)), head]
    counts = [0, len(four), -1, 200, len(head)]
    res = run_regions(ops, pages, 240, (900, 1300), counts=counts, page_base=7)
    assert res[0][5:] == (0, 0, 0) and res[2][5:] == (-1, -1, -1)
    assert res[1][6] == 4 and np.array_equal(res[1][0], t4) and res[3][6] == 1 and res[3][5] == 20
    assert res[4][6] == 4 and np.array_equal(res[4][0], th)
    run_regions(ops, pages, 240, (900, 1300), counts=counts, page_base=7, with_lines=False)


def test_regions_kernel_one_region_pages_equal_the_kernel_without_the_cut(ops):
    """One-region pages against msocr_reading_order_lines, and with deskew = 1 against msocr_reading_order_deskew (run_regions asserts
    both); a turned two-column page is cut in the deskewed frame."""
    pages = [np.asarray(rc.tl.text_page()), np.asarray(rc.tl.duplicate_page()), np.asarray(rc.tl.envelope_pages()["page_edges"])]
    res = run_regions(ops, pages, 1200, (3000, 1200), ratios=(INF, INF, 3.0))
    assert [r[6] for r in res] == [1, 1, 1] and res[0][5] == 70
    assert run_regions(ops, pages[:1], 1200, (3000, 1200))[0][6] == 1, "the text page ends as one region with the default ratios too"
    hw = (3000, 1200)
    res = run_regions(ops, [dk.text_page_quads(3.0, hw)], 1200, hw, deskew=True, quads=True)
    assert res[0][6] == 1 and res[0][5] == 70
    b, truth = rc.layout_page(cols=2, lines=20, per_line=4, gutter=64, seed=3)
    q = dk.turn(rc._rects(b), 3.0, (350.0, 450.0)).astype(F32)
    res = run_regions(ops, [q], len(q) + 3, (900, 700), deskew=True, quads=True)
    assert res[0][6] == 2 and np.array_equal(res[0][0], truth)
    run_regions(ops, [q], len(q) + 3, (900, 700), deskew=True, quads=True, with_lines=False)
    assert not np.array_equal(run_regions(ops, [q], len(q) + 3, (900, 700), quads=True)[0][0], truth), "in the page frame the band is closed"


def test_regions_kernel_largest_page(ops):
    """16384 words, the kernel's word capacity, in two columns of 2048 lines: every pair sweep of the cut at its full length."""
    n = 16384
    b = two_columns(n, seed=1)
    o, ln, rec, rg, rrec, nln, nrg, nc = run_regions(ops, [b], n, (int(b[:, 3].max()) + 50, 600))[0]
    assert nc == n and nrg == 2 and nln == 4096 and rrec[:, 1].tolist() == [8192, 8192]


def test_regions_entry_point_refusals(ops):
    from manuscript_ocr_amd import _native as nat
    L = nat.lib()
    b, c = torch.zeros((1, 4, 9), device="cuda"), torch.zeros((1,), dtype=torch.int32, device="cuda")
    o, k, d, nc, ln, rec, nl = _guard((1, 4)), _guard((1, 4)), _guard((1, 4, 8)), _guard((1,)), _guard((1, 4)), _guard((1, 4, 6)), _guard((1,))
    rg, rrec, nr = _guard((1, 4)), _guard((1, 4, 6)), _guard((1,))
    sk, cs = _guard((1, 4), torch.int64), _guard((1, 2), torch.float64)
    ws = torch.empty((L.msocr_reading_order_regions_workspace_bytes(1, 4),), dtype=torch.uint8, device="cuda")
    call = lambda ratios, deskew, louts, souts, routs: L.msocr_reading_order_regions(
        b.data_ptr(), c.data_ptr(), 1, 4, 100, 100, 5, 32, 100, 0.6, INF, 0, *ratios, deskew, o.data_ptr(), k.data_ptr(), d.data_ptr(), nc.data_ptr(),
        *louts, *souts, *routs, ws.data_ptr(), ops._stream())
    lfull, sfull, rfull = [ln.data_ptr(), rec.data_ptr(), nl.data_ptr()], [sk.data_ptr(), cs.data_ptr()], [rg.data_ptr(), rrec.data_ptr(), nr.data_ptr()]
    for miss in range(3):
        louts, routs = list(lfull), list(rfull)
        louts[miss], routs[miss] = None, None
        assert call(rc.DEFAULTS, 0, louts, sfull, rfull) == -1 and call(rc.DEFAULTS, 0, lfull, sfull, routs) == -1
    assert call(rc.DEFAULTS, 1, lfull, [None, cs.data_ptr()], rfull) == -1 and call(rc.DEFAULTS, 1, lfull, [sk.data_ptr(), None], rfull) == -1
    assert call(rc.DEFAULTS, 2, lfull, sfull, rfull) == -1
    for kk in range(3):
        for bad in (float("nan"), -0.5):
            ratios = list(rc.DEFAULTS)
            ratios[kk] = bad
            assert call(ratios, 0, lfull, sfull, rfull) == -1
    assert call(rc.DEFAULTS, 0, lfull, [None, None], rfull) == 0 and call((INF, INF, INF), 1, [None] * 3, sfull, rfull) == 0
    torch.cuda.synchronize()
    assert int(nr.cpu()[0]) == 0


# ================================================================================================ the Pipeline
PH, PW, DEG, BAND = 352, 1024, 5.0, 60


@pytest.fixture(scope="module")
def rec(gpu):
    from manuscript_ocr_amd import synth
    from manuscript_ocr_amd.recognizers import TRBA
    return TRBA(state_dict=synth.trba_state_dict_confident(194, 256, seed=3), config=CFG, device="cuda")


@pytest.fixture(scope="module")
def east_sd(gpu):
    from manuscript_ocr_amd import synth
    return synth.east_state_dict()


def _pages_and_maps(turned):
    """Two pages 1024 px wide whose words leave a band of 120 px free down the middle: two columns.  turned: the words turned
    rigidly by 5 degrees about the page centre."""
    from manuscript_ocr_amd import synth
    pgs, maps = [], []
    for seed in (41, 42):
        pg, rects = synth.synth_page(seed, PH, PW, line_pitch=44, word_h=22, margin=30)
        r = np.asarray(rects, dtype=np.float64)
        r = r[(r[:, 2] < 0.5 * PW - BAND) | (r[:, 0] > 0.5 * PW + BAND)]
        assert (r[:, 2] < 0.5 * PW).sum() >= 6 and (r[:, 0] > 0.5 * PW).sum() >= 6
        quads = np.stack([r[:, [0, 1]], r[:, [2, 1]], r[:, [2, 3]], r[:, [0, 3]]], axis=1)
        pgs.append(pg)
        if turned:
            maps.append(synth.synth_quad_maps(dk.turn(quads, DEG, (0.5 * PW, 0.5 * PH)), (PH, PW), (PH // 4, PW // 4), seed))
        else:
            maps.append(synth.synth_maps(r.tolist(), (PH, PW), (PH // 4, PW // 4), seed))
    mo = (torch.from_numpy(np.stack([m[0] for m in maps])).cuda(), torch.from_numpy(np.stack([m[1] for m in maps])).cuda())
    return pgs, mo


def _routes(pipe, det, pgs, mo, monkeypatch):
    from manuscript_ocr_amd import ops
    out = {"device": pipe.predict_batch(pgs, _maps_override=mo)}
    pipe.device_order = False
    out["host"] = pipe.predict_batch(pgs, _maps_override=mo)
    pipe.device_order = True
    real, calls = ops.reading_order_regions, []

    def flagged(*args, **kw):
        ro, rl, sk, rg = real(*args, **kw)
        calls.append(1)
        bad = torch.tensor([-1] + [0] * (len(ro.ncrop) - 1), dtype=torch.int32, device=ro.ncrop.device)
        return ro._replace(ncrop=torch.where(bad < 0, bad, ro.ncrop)), rl, sk, rg

    monkeypatch.setattr(ops, "reading_order_regions", flagged)
    out["flagged"] = pipe.predict_batch(pgs, _maps_override=mo)
    monkeypatch.setattr(ops, "reading_order_regions", real)
    assert calls == [1], "the device route goes through ops.reading_order_regions"
    out["generic"] = gt._generic(pipe, det, pgs, mo, monkeypatch)
    return out


@pytest.mark.parametrize("mode", ["plain", "group_lines", "deskew+rectify_crops+char_details", "n_best"])
def test_pipeline_columns_on_every_route(gpu, rec, east_sd, monkeypatch, mode):
    from manuscript_ocr_amd import Pipeline
    from manuscript_ocr_amd.detectors import EAST
    from manuscript_ocr_amd.detectors._types import Page, Region, RegionLine, SkewPage
    full = mode == "deskew+rectify_crops+char_details"
    det = EAST(state_dict=east_sd, target_size=(PW, PH), device="cuda", axis_aligned_output=not full)
    pipe = Pipeline(det, rec)
    pipe.group_lines = mode == "group_lines"
    pipe.deskew = pipe.rectify_crops = pipe.char_details = full
    pipe.n_best = 2 if mode == "n_best" else 0
    pgs, mo = _pages_and_maps(full)
    off = pipe.predict_batch(pgs, _maps_override=mo)
    off_generic = gt._generic(pipe, det, pgs, mo, monkeypatch)
    assert sum(w.text is not None for p in off for b in p.blocks for w in b.words) >= 16
    pipe.columns = True
    out = _routes(pipe, det, pgs, mo, monkeypatch)
    dev = out["device"]
    polys = lambda pages: [[w.polygon for b in p.blocks for w in b.words] for p in pages]
    assert all(a != b for a, b in zip(polys(dev), polys(off))), "the plain order of these pages reads across the band"
    block_type, page_type = (RegionLine if pipe.group_lines else Region), (SkewPage if full else Page)
    for p in dev:
        cx = [np.mean([pt[0] for pt in w.polygon]) for b in p.blocks for w in b.words]
        left = [x < 0.5 * PW for x in cx]
        assert left == sorted(left, reverse=True) and 6 <= sum(left) <= len(left) - 6, "column by column: the left column first"
        regions = [b.region if pipe.group_lines else b.index for b in p.blocks]
        assert regions[0] == 0 and regions == sorted(regions) and len(set(regions)) >= 2 and set(regions) == set(range(max(regions) + 1))
    for name, pages in out.items():
        assert [type(p) for p in pages] == [page_type, page_type], name
        assert all(type(b) is block_type for p in pages for b in p.blocks), name
        assert polys(pages) == polys(dev), name
        assert [gt._layout(p) for p in pages] == [gt._layout(p) for p in dev], name
        assert all(b.bbox == gt._union(b.words) for p in pages for b in p.blocks), name
        ref = off_generic if name == "generic" else off
        key = lambda pages: [sorted(map(repr, gt._words(p))) for p in pages]
        assert key(pages) == key(ref), (name, "the words of the run without the switch, permuted")
        if pipe.char_details and name != "generic":
            chars = lambda pages: [sorted(map(repr, zip(gt._words(p), gt._chars(p)))) for p in pages]
            assert chars(pages) == chars(off), name
    for name in ("host", "flagged"):
        assert [gt._words(p) for p in out[name]] == [gt._words(p) for p in dev], name
    if pipe.n_best:  # what sits behind the order still reaches the words inside the regions
        from manuscript_ocr_amd.detectors._types import AltWord
        alts = lambda pages: [[(w.text, [a.text for a in w.alternatives]) for b in p.blocks for w in b.words if w.text is not None] for p in pages]
        assert all(type(w) is AltWord and w.alternatives[0].text == w.text for p in dev for b in p.blocks for w in b.words if w.text is not None)
        assert alts(out["host"]) == alts(dev) and alts(out["flagged"]) == alts(dev)
    pipe.columns = False
    again = pipe.predict_batch(pgs, _maps_override=mo)
    assert [type(p) for p in again] == [type(p) for p in off] and [gt._words(p) for p in again] == [gt._words(p) for p in off]
    assert [gt._chars(p) for p in again] == [gt._chars(p) for p in off]
    assert [[type(b) for b in p.blocks] for p in again] == [[type(b) for b in p.blocks] for p in off]
