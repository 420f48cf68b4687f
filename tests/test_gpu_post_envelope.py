"""The page post-processing kernels against plain references over their envelope: east_decode_kernel, lanms_zero_kernel,
lanms_rank_x0_kernel, east_lanms_kernel, lanms_iou_bits_kernel, lanms_greedy_bits_kernel (csrc/east_post.hip), east_box_tail_kernel
(csrc/east_tail.hip) and reading_order_kernel (csrc/reading_order.hip).  Their contract is bit identity with the reference's NumPy /
Python code, so every comparison is bit for bit (floats as uint32, ints with array_equal); what can go wrong is a regime switch, a
capacity edge, a tie rule or a buffer layout, and every case names the regime it reaches and asserts the quantity that selects it
(candidate count, nm, W, pairs, lines) FROM THE REFERENCE SIDE before it compares.

References, in the order of preference:
  (a) the oracle: oracle.east_post.decode_quads_from_maps, oracle.lanms.locality_aware_nms (stable (key, index) sorts, returns nm),
      the oracle tail expand_boxes -> scale_boxes_to_original -> remove_fully_contained_boxes -> remove_area_anomalies ->
      convert_to_axis_aligned, oracle.pipeline_glue.sort_boxes_reading_order_with_resolutions + the first-equal-word re-match, and
      ops.crop_descriptors (NumPy) for the descriptors;
  (b) construction: disjoint quads (LANMS keeps all, in descending score order; the tail keeps all but the planted inserts and the
      earlier box of every planted duplicate, in index order, and with IDENT parameters returns the input rows themselves), all-on
      maps (count == cells), word grids (reading order row-major);
  (c) the host twins msocr_east_box_tail_host and msocr_reading_order_host, only beside (b) on pages too large for (a) (the oracle
      tail takes 28 s for 2049 boxes, the Python reading order 83 s for 4096 lines); tests/test_host_cpu.py pins both twins to (a) on
      the same page generators (tail_content_pages, tail_kept_page, tail_grid_page, ro_content_pages, clique_page, word_grid).
The decode drop rule has no reference behaviour (NaN polygons): its expectation is the oracle's decode of the cleaned maps minus the
cells the rule names, and the rule (|v| < 1e7 fails for the centre score or one of the centre's eight offsets) is evaluated on the maps.

Regimes and the constants that create them:
  decode   1024-thread chunks of cells (1023 / 1024 / 1025 / 2049 cells, q = 1, 2 with odd Wq, 4), 16 waves of 64 per chunk (all-on
           maps), `> thr` strict in f32, any pixel of the q x q cell, overflow flag iff total > max_cand, drop rule at 1e7.
  LANMS    scan segments S = ceil(n / 8) (n 7 / 8 / 9); RS_TILE = 256 * RS_Q = 2048 rank tiles (n 2047 / 2048 / 2049); W = ceil(nm / 32)
           suppression words, 64 lanes (nm 31 / 32 / 33, 2048 / 2049); NMS_BITCAP = 8192 and bitcap = max_cand rounded up to 32 (nm 8192
           bit matrix / 8193 in-kernel loop at max_cand 8200; max_cand 100 / 1000 / 2303 / 2304 with a full page); bit 31 of a count;
           the nm header, bit matrix and rank accumulator of a reused workspace.
  tail     TAIL_LDSM = 2048 (M 2048 LDS / 2049 workspace), keep words per lane at W = 64 / 65 / 129 / 512, TAIL_CAPM = 16384 (16385: -1),
           cap = max_cand rounded up to 32 against M == max_cand and max_cand + 1, stable area ties, NumPy pairwise sums (8, 128).
  order    output stride max_cand against workspace stride cap = min(max_cand, RO_CAP = 16384) (max_cand 131 / 16400), per = ceil(n /
           1024) of the block scan (n 1023 / 1024 / 1025), RO_MAXLINES = 4096 (4097: -1), pair buffer P = 8 cap + 4096 (5696 / 5697 at
           cap 200), 50 sweeps, truncation toward zero, NaN gap at avg_h == 0, last-shrunk / first-equal re-match, negative-stop slices.

Guards: every output (cand, counts, boxes, nbox, out, n_out, order, keep, desc, ncrop) is allocated with one page more than the launch
has and filled with a sentinel; the page behind the last, the rows past every page's count and WS_TAIL bytes behind
msocr_*_workspace_bytes must keep it.  Inputs past a page's count hold NaN.  Every launch goes through the C ABI on the guarded buffers
and, where via_ops, again through ops.east_decode / east_lanms / east_box_tail / reading_order_crops (same bits required); multi-page
launches run twice.

Regime quantities the cases assert from the reference side (each case prints its own with -s): decode counts equal the constructed
ones (every cell of 514 .. 2049, or 30 % of them; the drop rule removes 42 / 45 cells at q = 1 / 2); LANMS nm == n on every disjoint
page (31 .. 8193) and nm < n on every run page, equal_scores nm 90 kept 60, iou_equals_thr nm 24 kept 24; the tail keeps 113 of 120
boxes of the duplicates page and 40 of 120 chain boxes, K of K + 3 reach the statistics at the pairwise blocks, the grid pages lose
6 / 4 / 12 / 18 boxes at M 2048 / 2049 / 4128 / 16384; reading order: 5696 / 5697 pairs, 4096 / 4097 lines, 0 pairs on the word grids.

Finding: east_box_tail_kernel compared M with cap, which rounds max_cand up to a multiple of 32, so a page of max_cand + 1 .. cap
boxes was processed across the page boundary instead of refused (-1), against the contract in include/msocr.h; the kernel now also
refuses M > max_cand (test_tail_full_page_and_one_box_too_many[100]).

Mutants that the cases are built to catch (value-only, every index stays in bounds; applied to a scratch copy of the sources):
  decode `> thr` -> `>=`: eqthr cases; `< 1e7` -> `<=`: test_decode_drop_rule_boundaries; `total > max_cand` -> `>=`:
  test_decode_overflow_flag_at_max_cand.  LANMS index tie of the x0 keys reversed: equal_x0, signed_zero_x0, duplicates; index tie of
  the score sort reversed: equal_scores; merge test `> thr` -> `>=`: iou_equals_thr.  Tail area tie `j < i` -> `j > i`: duplicates,
  equal_areas, the grid pages; the M > max_cand test removed: test_tail_full_page_and_one_box_too_many[100].  Reading order
  `total > P` -> `>=`: test_reading_order_pair_buffer_capacity; `L >= RO_MAXLINES` -> `L >= RO_MAXLINES - 1`:
  test_reading_order_line_and_box_capacity; truncation -> floor in ro_shrink: fifty_sweeps, negative_fractions.
  `nm <= bitcap` -> `<` and `M <= TAIL_LDSM` -> `<` are equivalent mutants: both sides of either switch compute the same result, the
  cases at 8192 / 8193 and 2048 / 2049 check that they do.

"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEED = 20261017
F32 = np.float32
FSENT, ISENT, WSENT, WS_TAIL = 7.25, -777, 0xA5, 4096
FSENT_BITS = np.array([FSENT], dtype=F32).view(np.uint32)[0]
THR = float(F32(0.6))      # the decode threshold as the f32 the C ABI receives
IOU = 0.2
E_ARG = -1


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from manuscript_ocr_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def nat(ops):
    from manuscript_ocr_amd import _native
    return _native


# ================================================================================================ guards and comparisons
def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _fguard(N, mc, w):
    """N pages and one more behind them, all sentinel."""
    return torch.full((N + 1, mc, w), FSENT, dtype=torch.float32, device="cuda")


def _iguard(*shape):
    return torch.full(shape, ISENT, dtype=torch.int32, device="cuda")


def _f_untouched(a):
    return bool((_bits(a) == FSENT_BITS).all())


def _workspace(nbytes):
    return torch.full((nbytes + WS_TAIL,), WSENT, dtype=torch.uint8, device="cuda")


def _ws_tail_ok(ws, nbytes):
    return ws.numel() == nbytes + WS_TAIL and bool((ws[nbytes:] == WSENT).all())


def _pages_f(pages, mc, w=9):
    """Device input [N + 1, mc, w]: rows past a page's count and the page behind the last hold NaN (never to be read)."""
    a = np.full((len(pages) + 1, mc, w), np.nan, dtype=F32)
    for i, p in enumerate(pages):
        if p is not None and len(p):
            a[i, :len(p)] = p
    return torch.from_numpy(a).cuda()


# ================================================================================================ decode
def _decode(ops, nat, score, geo, q, mc, thr=THR, scale=4.0):
    """score [N,H,W], geo [N,H,W,8] (numpy f32) -> (rows per page, raw counts).  Guarded launch through the C ABI, then the same
    launch through ops.east_decode, which must give the same bits."""
    N, H, W = score.shape
    s, g = torch.from_numpy(score).cuda(), torch.from_numpy(geo).cuda()
    cand, cnt = _fguard(N, mc, 9), _iguard(N + 1)
    rc = nat.lib().msocr_east_decode(s.data_ptr(), g.data_ptr(), N, H, W, thr, scale, q, cand.data_ptr(), cnt.data_ptr(), mc, ops._stream())
    assert rc == 0
    torch.cuda.synchronize()
    c, k = cand.cpu().numpy(), cnt.cpu().numpy()
    assert k[N] == ISENT and _f_untouched(c[N]), "decode wrote behind the last page"
    rows = []
    for n in range(N):
        m = int(k[n]) & 0x7FFFFFFF
        assert m <= mc and _f_untouched(c[n, m:]), ("decode wrote rows past its count", n, m)
        rows.append(c[n, :m].copy())
    c2, k2 = ops.east_decode(s, g, thr, scale, q, mc)
    c2, k2 = c2.cpu().numpy(), k2.cpu().numpy()
    assert np.array_equal(k2, k[:N]) and all(_same(c2[n, :len(rows[n])], rows[n]) for n in range(N)), "ops.east_decode differs"
    return rows, k[:N]


def _decode_ref(score, geo, q, thr=THR, scale=4.0):
    """One page: the oracle's decode of the cleaned maps, minus the cells the drop rule names (centre score or one of the eight
    centre offsets NaN, infinite or of magnitude >= 1e7) -> (rows, number of cells dropped).  A cell is on as in the oracle:
    a pixel > thr (f32), so NaN and -inf switch nothing on and +inf does."""
    from oracle import east_post as P
    with np.errstate(invalid="ignore"):
        bad_s, bad_g = ~(np.abs(score) < F32(1e7)), ~(np.abs(geo) < F32(1e7))
        on = score > F32(thr)
    cs, cg = score.copy(), geo.copy()
    cs[bad_s] = np.where(on[bad_s], F32(1.0), F32(0.0))
    cg[bad_g] = 0
    rows = P.decode_quads_from_maps(cs, cg, F32(thr), scale, q)
    ys, xs = np.where(cs > F32(thr))
    if len(ys) == 0:
        return rows, 0
    if q > 1:
        u = np.unique(np.column_stack([(ys // q) * q + q // 2, (xs // q) * q + q // 2]), axis=0)
        ys, xs = u[:, 0], u[:, 1]
    assert len(ys) == len(rows)
    drop = bad_s[ys, xs] | bad_g[ys, xs].any(axis=1)
    return rows[~drop], int(drop.sum())


def _cells(rng, Hq, Wq, frac):
    n = Hq * Wq
    pick = rng.permutation(n)[:max(1, int(frac * n))]
    return pick // Wq, pick % Wq


def _maps(rng, H, W, q, kind):
    """-> score, geo, expected count (from the construction)."""
    Hq, Wq = H // q, W // q
    geo = rng.uniform(-30, 30, (H, W, 8)).astype(F32)
    off = rng.uniform(0.0, 0.55, (H, W)).astype(F32)
    if kind == "allon":
        return rng.uniform(0.7, 1.0, (H, W)).astype(F32), geo, Hq * Wq
    if kind == "empty":
        return off, geo, 0
    cy, cx = _cells(rng, Hq, Wq, 0.3)
    if kind == "sparse":       # one random pixel of every chosen cell passes
        off[cy * q + rng.integers(0, q, len(cy)), cx * q + rng.integers(0, q, len(cy))] = rng.uniform(0.61, 1.0, len(cy)).astype(F32)
        return off, geo, len(cy)
    if kind == "offcentre":    # only a pixel that is NOT the centre passes (q > 1); the row carries the centre's score <= thr
        dy, dx = rng.integers(0, q, len(cy)), rng.integers(0, q, len(cy))
        if q > 1:
            centre = (dy == q // 2) & (dx == q // 2)
            dx[centre] = q // 2 - 1
        off[cy * q + dy, cx * q + dx] = F32(0.9)
        return off, geo, len(cy)
    assert kind == "eqthr"     # whole cells exactly at thr stay off, a pixel one ulp above switches its cell on
    half = len(cy) // 2
    for y, x in zip(cy[:half], cx[:half]):
        off[y * q:(y + 1) * q, x * q:(x + 1) * q] = F32(THR)
    dy, dx = rng.integers(0, q, len(cy) - half), rng.integers(0, q, len(cy) - half)
    off[cy[half:] * q + dy, cx[half:] * q + dx] = np.nextafter(F32(THR), F32(1))
    return off, geo, len(cy) - half


# (H, W, q): cells = 1023, 1024, 1025 and 2049 around the 1024-thread chunk (and its 64-lane waves); q = 2 with odd Wq; q = 4
DECODE_SHAPES = [(31, 33, 1), (32, 32, 1), (25, 41, 1), (3, 683, 1), (50, 82, 2), (6, 1366, 2), (132, 124, 4), (8, 1028, 4)]


@pytest.mark.parametrize("kind", ["allon", "sparse", "offcentre", "eqthr"])
@pytest.mark.parametrize("shape", DECODE_SHAPES, ids=lambda s: "%dx%dq%d" % s)
def test_decode_cells_chunks_and_threshold(ops, nat, shape, kind):
    """east_decode_kernel: 1 .. 3 chunks of 1024 cells, the last one partial; all-on maps put a candidate in every lane of
    every wave (count == cells, rows in cell order); off-centre and == thr maps pin the any-pixel rule and the strict compare."""
    H, W, q = shape
    rng = np.random.default_rng([SEED, H, W, q, len(kind)])
    score, geo, want = _maps(rng, H, W, q, kind)
    ncell = (H // q) * (W // q)
    exp, dropped = _decode_ref(score, geo, q)
    assert len(exp) == want and dropped == 0, "regime: the reference's candidate count is the constructed one"
    if kind == "offcentre" and q > 1:
        assert (exp[:, 8] <= F32(THR)).all()
    rows, k = _decode(ops, nat, score[None], geo[None], q, ncell + 3)
    print(f"decode {shape} {kind}: cells {ncell} count {int(k[0])}")
    assert int(k[0]) == want and _same(rows[0], exp)


@pytest.mark.parametrize("kind", ["allon", "sparse"])
def test_decode_overflow_flag_at_max_cand(ops, nat, kind):
    """total == max_cand is no overflow; total == max_cand + 1 sets bit 31 and keeps the first max_cand rows."""
    H, W, q = 25, 41, 1
    rng = np.random.default_rng([SEED, 7, len(kind)])
    score, geo, total = _maps(rng, H, W, q, kind)
    exp, _ = _decode_ref(score, geo, q)
    assert len(exp) == total and total > 64
    for mc in (total - 1, total, total + 1):
        rows, k = _decode(ops, nat, score[None], geo[None], q, mc)
        c = int(k[0])
        print(f"decode overflow {kind}: total {total} max_cand {mc} count {c:#x}")
        assert (c < 0) == (mc == total - 1), (mc, total, c)
        assert (c & 0x7FFFFFFF) == min(mc, total) and _same(rows[0], exp[:mc])


def test_decode_three_pages_one_empty(ops, nat):
    H, W, q = 50, 82, 2
    rng = np.random.default_rng([SEED, 11])
    pages = [_maps(rng, H, W, q, kind) for kind in ("allon", "empty", "sparse")]
    score, geo = np.stack([p[0] for p in pages]), np.stack([p[1] for p in pages])
    exps = [_decode_ref(p[0], p[1], q)[0] for p in pages]
    assert [len(e) for e in exps] == [p[2] for p in pages] and len(exps[1]) == 0
    for rep in range(2):
        rows, k = _decode(ops, nat, score, geo, q, 1025)
        assert [int(v) for v in k] == [len(e) for e in exps]
        assert all(_same(r, e) for r, e in zip(rows, exps))


@pytest.mark.parametrize("q", [1, 2])
def test_decode_drop_rule_boundaries(ops, nat, q):
    """NaN, +-inf, +-1e7 at a centre score or in one geo lane drop the cell; nextafter(1e7, 0) does not; the same values in a
    pixel that is not the centre change nothing but the cell's on / off state as `> thr` defines it."""
    H, W = 50, 82
    rng = np.random.default_rng([SEED, 13, q])
    score, geo, _ = _maps(rng, H, W, q, "allon")
    Hq, Wq = H // q, W // q
    cy, cx = _cells(rng, Hq, Wq, 0.2)
    ctr = q // 2 if q > 1 else 0
    vals = [np.nan, np.inf, -np.inf, 1e7, -1e7, np.nextafter(F32(1e7), F32(0)), -np.nextafter(F32(1e7), F32(0))]
    k = 0
    for v in vals:                       # centre score
        score[cy[k] * q + ctr, cx[k] * q + ctr] = v
        k += 1
    for lane in range(8):                # single geo lanes of the centre pixel
        for v in vals:
            geo[cy[k] * q + ctr, cx[k] * q + ctr, lane] = v
            k += 1
    assert k <= len(cy)
    if q > 1:                            # non-centre pixels: values there are never copied, and a NaN there is not "> thr"
        for v in vals:
            score[cy[k] * q, cx[k] * q] = v
            geo[cy[k] * q, cx[k] * q, 3] = v
            k += 1
        y, x = cy[k], cx[k]              # a cell whose only candidates for "on" are NaN and -inf: off
        score[y * q:(y + 1) * q, x * q:(x + 1) * q] = F32(0.1)
        score[y * q, x * q], score[y * q, x * q + 1] = np.nan, -np.inf
        y, x = cy[k + 1], cx[k + 1]      # +inf off-centre switches the cell on; its centre is sane
        score[y * q:(y + 1) * q, x * q:(x + 1) * q] = F32(0.1)
        score[y * q, x * q] = np.inf
    exp, dropped = _decode_ref(score, geo, q)
    # every geo lane: NaN, +-inf, +-1e7 drop the cell (8 x 5).  Centre score: the same five where another pixel keeps the cell on
    # (q = 2); for q = 1 the centre is the only pixel, so +inf and 1e7 drop it and NaN, -inf, -1e7, -9999999 leave it off
    off = 4 if q == 1 else 1
    assert dropped == (2 if q == 1 else 5) + 8 * 5, dropped
    assert len(exp) == Hq * Wq - dropped - off
    rows, kk = _decode(ops, nat, score[None], geo[None], q, Hq * Wq)
    print(f"decode drop rule q={q}: cells {Hq * Wq} dropped {dropped} count {int(kk[0])}")
    assert int(kk[0]) == len(exp) and _same(rows[0], exp)


def test_decode_rejects_maps_not_divisible_by_quant(ops, nat):
    s, g = torch.zeros(1, 5, 8, device="cuda"), torch.zeros(1, 5, 8, 8, device="cuda")
    cand, cnt = _fguard(1, 4, 9), _iguard(2)
    for H, W, q in ((5, 8, 2), (4, 7, 2), (5, 8, 4)):
        assert nat.lib().msocr_east_decode(s.data_ptr(), g.data_ptr(), 1, H, W, THR, 4.0, q, cand.data_ptr(), cnt.data_ptr(), 4, ops._stream()) == E_ARG
    with pytest.raises(nat.NativeError):
        ops.east_decode(s, g, THR, 4.0, 2, 4)
    torch.cuda.synchronize()
    assert _f_untouched(cand.cpu().numpy()) and bool((cnt == ISENT).all())


# ================================================================================================ LANMS
def _lanms(ops, nat, pages, mc, counts=None, ws=None, via_ops=True):
    """pages: list of [n, 9] f32 arrays -> (rows per page, workspace).  Guarded launch through the C ABI on `ws` (a fresh
    sentinel-tailed one when None); via_ops repeats it through ops.east_lanms on a second workspace."""
    N = len(pages)
    cand = _pages_f(pages, mc)
    cnt_l = [len(p) for p in pages] if counts is None else list(counts)
    cnt = torch.tensor(cnt_l + [ISENT], dtype=torch.int64).to(torch.int32).cuda()
    nbytes = nat.lib().msocr_lanms_workspace_bytes(N, mc)
    ws = _workspace(nbytes) if ws is None else ws
    boxes, nbox = _fguard(N, mc, 9), _iguard(N + 1)
    rc = nat.lib().msocr_east_lanms(cand.data_ptr(), cnt.data_ptr(), N, mc, IOU, boxes.data_ptr(), nbox.data_ptr(), ws.data_ptr(), ops._stream())
    assert rc == 0
    torch.cuda.synchronize()
    b, k = boxes.cpu().numpy(), nbox.cpu().numpy()
    assert k[N] == ISENT and _f_untouched(b[N]), "LANMS wrote behind the last page"
    assert _ws_tail_ok(ws, nbytes), "LANMS wrote behind msocr_lanms_workspace_bytes"
    rows = []
    for n in range(N):
        m = int(k[n])
        assert 0 <= m <= (cnt_l[n] & 0x7FFFFFFF) and _f_untouched(b[n, m:]), ("LANMS wrote rows past nbox", n, m)
        rows.append(b[n, :m].copy())
    if via_ops:
        ws2 = _workspace(nbytes)
        b2, k2 = ops.east_lanms(cand[:N], cnt[:N], IOU, workspace=ws2)
        b2, k2 = b2.cpu().numpy(), k2.cpu().numpy()
        assert _ws_tail_ok(ws2, nbytes)
        assert np.array_equal(k2, k[:N]) and all(_same(b2[n, :len(rows[n])], rows[n]) for n in range(N)), "ops.east_lanms differs"
    return rows, ws


def _lanms_ref(inp):
    from oracle import lanms as L
    return L.locality_aware_nms(inp, IOU, return_merged_count=True)


def merge_runs(rng, n, n_base, max_run):
    """Exactly n candidates in runs of near-identical quads that merge in phase 1 (the generator of
    test_lanms_speculative_scan_long_and_short_runs), shuffled."""
    rows, x = [], 10.0
    while len(rows) < n:
        for _ in range(n_base):
            w, h = rng.uniform(40, 200), rng.uniform(12, 40)
            y = rng.uniform(10, 1500)
            base = np.array([x, y, x + w, y, x + w, y + h, x, y + h])
            for _ in range(int(rng.integers(1, max_run + 1))):
                rows.append(np.concatenate([base + rng.normal(0, 0.4, 8), [rng.uniform(0.05, 1.0)]]))
            x += rng.uniform(0.3, 1.2) * w
    inp = np.asarray(rows[:n], dtype=F32)
    return inp[rng.permutation(n)]


def disjoint_polys(rng, n):
    """n pairwise disjoint quads (nothing merges, nothing is suppressed: nm == n and the output is the input in descending
    score order), distinct scores, shuffled."""
    cols = int(np.ceil(np.sqrt(n)))
    i = np.arange(n)
    x = 10 + 40.0 * (i % cols) + rng.uniform(0, 8, n)
    y = 10 + 30.0 * (i // cols) + rng.uniform(0, 8, n)
    w, h = rng.uniform(12, 24, n), rng.uniform(6, 14, n)
    sc = (rng.permutation(n) + 1.0) / (n + 1.0)
    inp = np.stack([x, y, x + w, y, x + w, y + h, x, y + h, sc], axis=1).astype(F32)
    assert len(np.unique(inp[:, 8])) == n
    return inp[rng.permutation(n)]


def _by_score(inp):
    return inp[np.argsort(-inp[:, 8].astype(np.float64), kind="stable")]


@pytest.mark.parametrize("layout", ["runs", "disjoint"])
@pytest.mark.parametrize("n", [1, 7, 8, 9, 767, 768, 769, 2047, 2048, 2049, 6144, 6145])
def test_lanms_segment_and_rank_tile_edges(ops, nat, n, layout):
    """n < 8: one scan segment, 8 / 9: two; 2048 / 2049: one / two tiles of lanms_rank_x0_kernel (RS_TILE = 256 * RS_Q = 2048),
    grid (1, 1) / (2, 2) per page.  768 / 769: the compaction's chunk per thread goes 1 -> 2 (LANMS_PAGE_T = 768 threads);
    6144 / 6145: the segment count saturates at 768 and the segment length goes 8 -> 9."""
    rng = np.random.default_rng([SEED, 21, n, len(layout)])
    inp = merge_runs(rng, n, 4, 12) if layout == "runs" else disjoint_polys(rng, n)
    exp, nm = _lanms_ref(inp)
    assert nm == n if layout == "disjoint" else (nm < n or n == 1), "regime: merged count"
    if layout == "disjoint":
        assert _same(exp, _by_score(inp))
    mc = n + 5
    rows, _ = _lanms(ops, nat, [inp], mc)
    print(f"lanms n={n} {layout}: max_cand {mc} nm {nm} kept {len(exp)}")
    assert _same(rows[0], exp)


_BIG = {}


def _big_disjoint():
    """8193 disjoint quads whose last one is disjoint from all others, so the 8192-page's result is the 8193-page's without
    that row: one oracle run (4 s) serves both and the mixed launch."""
    if not _BIG:
        inp = disjoint_polys(np.random.default_rng([SEED, 22]), 8193)
        exp, nm = _lanms_ref(inp)
        assert nm == 8193 and _same(exp, _by_score(inp))
        _BIG["8193"] = (inp, exp)
        _BIG["8192"] = (inp[:8192], _by_score(inp[:8192]))
    return _BIG


@pytest.mark.parametrize("nm", [31, 32, 33, 2048, 2049, 8192, 8193])
def test_lanms_suppression_path_edges_disjoint(ops, nat, nm):
    """nm == n on disjoint quads.  W = ceil(nm / 32): 1 -> 2 words at 32 / 33, 64 -> 65 at 2048 / 2049 (a lane of the greedy
    wave gains its second suppression word); nm == bitcap = 8192 is the last bit-matrix page, 8193 runs the in-kernel loop
    (max_cand 8200)."""
    if nm >= 8192:
        inp, exp = _big_disjoint()[str(nm)]
        mc = 8200
    else:
        inp = disjoint_polys(np.random.default_rng([SEED, 23, nm]), nm)
        exp, got_nm = _lanms_ref(inp)
        assert got_nm == nm
        mc = nm + 7
    assert len(exp) == nm and _same(exp, _by_score(inp))
    rows, _ = _lanms(ops, nat, [inp], mc, via_ops=nm < 8192)
    bitcap = (min(mc, 8192) + 31) // 32 * 32
    print(f"lanms disjoint nm={nm}: max_cand {mc} bitcap {bitcap} W {(nm + 31) // 32} path {'bits' if nm <= bitcap else 'in-kernel'}")
    assert _same(rows[0], exp)


@pytest.mark.parametrize("mc", [100, 1000, 2303, 2304])
def test_lanms_max_cand_not_a_multiple_of_32(ops, nat, mc):
    """bitcap = max_cand rounded up to 32 (128, 1024, 2304) is the row stride of the bit matrix and sizes the workspace; a full
    page (n == nm == max_cand, for 2304 also == bitcap) beside a merging page."""
    rng = np.random.default_rng([SEED, 24, mc])
    full, runs = disjoint_polys(rng, mc), merge_runs(rng, mc // 2, 3, 9)
    (e0, nm0), (e1, nm1) = _lanms_ref(full), _lanms_ref(runs)
    assert nm0 == mc and nm1 < mc // 2
    for rep in range(2):
        rows, _ = _lanms(ops, nat, [full, runs], mc, via_ops=rep == 0)
        assert _same(rows[0], e0) and _same(rows[1], e1)
    print(f"lanms max_cand {mc}: bitcap {(mc + 31) // 32 * 32} nm {nm0}, {nm1}")


def _rect(x0, y0, x1, y1, sc):
    return [x0, y0, x1, y0, x1, y1, x0, y1, sc]


def lanms_tie_pages(rng):
    """name -> [n, 9] f32.  Every page's result depends on how a tie is broken; the oracle breaks it by index."""
    pages = {}
    # equal x0: a column of boxes that overlap their neighbours (IoU 6 / 26 > 0.2), in shuffled index order: which ones merge
    # into which, and with what weights, follows the index order
    col = [_rect(100.0, 10.0 * k, 100.0 + rng.uniform(40, 60), 10.0 * k + 16.0, rng.uniform(0.3, 1.0)) for k in range(40)]
    pages["equal_x0"] = np.asarray(col, dtype=F32)[rng.permutation(40)]
    z = [_rect(-0.0 if k % 2 else 0.0, 10.0 * k, 50.0 + k, 10.0 * k + 16.0, rng.uniform(0.3, 1.0)) for k in range(24)]
    z = np.asarray(z, dtype=F32)[rng.permutation(24)]
    assert np.signbit(z[:, 0]).sum() == 12 and np.signbit(z[:, 6]).sum() == 12
    pages["signed_zero_x0"] = z
    # equal scores in the second sort: A and B overlap (IoU 1 / 3) but a far box F sorts between them by x0, so they survive
    # phase 1 as two polygons of equal score; the earlier one in the stable order suppresses the other
    eq = []
    for k in range(30):
        y, s = 40.0 * k, float(F32(rng.uniform(0.3, 0.9)))
        eq += [_rect(100.0, y, 160.0, y + 20.0, s), _rect(110.0, y + 5000.0, 150.0, y + 5020.0, s if k % 2 else 0.95),
               _rect(130.0, y, 190.0, y + 20.0, s)]
    pages["equal_scores"] = np.asarray(eq, dtype=F32)[rng.permutation(len(eq))]
    # exact duplicates (IoU 1) in pairs and triples, and a duplicate with reversed winding
    d = merge_runs(rng, 30, 30, 1)
    d = np.concatenate([d, d[:10], d[:4]])
    d[30:, 8] = rng.uniform(0.1, 1.0, 14).astype(F32)
    rev = d[10:20].copy()
    rev[:, :8] = rev[:, [0, 1, 6, 7, 4, 5, 2, 3]]
    d = np.concatenate([d, rev])
    pages["duplicates"] = d[rng.permutation(len(d))]
    # IoU == thr exactly: 256 / 1280 is the double nearest 0.2, and `>` is strict: neither merged nor suppressed
    t = []
    for k in range(12):
        y = 40.0 * k
        t += [_rect(0.0, y, 48.0, y + 16.0, rng.uniform(0.3, 1.0)), _rect(32.0, y, 80.0, y + 16.0, rng.uniform(0.3, 1.0))]
    pages["iou_equals_thr"] = np.asarray(t, dtype=F32)
    return pages


def test_lanms_ties_duplicates_and_exact_threshold(ops, nat):
    pages = lanms_tie_pages(np.random.default_rng([SEED, 25]))
    names = list(pages)
    refs = {k: _lanms_ref(pages[k]) for k in names}
    assert refs["iou_equals_thr"][1] == 24 and len(refs["iou_equals_thr"][0]) == 24, "IoU == thr must not merge or suppress"
    assert refs["equal_scores"][1] == 90 and len(refs["equal_scores"][0]) == 60, "A and B survive phase 1, one of them phase 2"
    assert refs["duplicates"][1] < len(pages["duplicates"])
    rows, _ = _lanms(ops, nat, [pages[k] for k in names], 131)
    wrong = []
    for k, r in zip(names, rows):
        print(f"lanms ties {k}: n {len(pages[k])} nm {refs[k][1]} kept {len(refs[k][0])}")
        if not _same(r, refs[k][0]):
            wrong.append(k)
    assert not wrong, wrong


def test_lanms_mixed_launch_and_stale_workspace(ops, nat):
    """One launch (max_cand 8200, bitcap 8192) of a small bit-matrix page, an in-kernel page (nm 8193), an empty page, a page
    whose count carries bit 31, and the largest bit-matrix page (nm 8192); then the same workspace again with the pages permuted so
    that every slot inherits another regime's header, bit matrix and rank accumulator; then once more.  Every page equals the oracle."""
    rng = np.random.default_rng([SEED, 26])
    big = _big_disjoint()
    a, d = merge_runs(rng, 600, 5, 20), merge_runs(rng, 300, 4, 10)
    pages = {"A": a, "B": big["8193"][0], "C": np.zeros((0, 9), F32), "D": d, "E": big["8192"][0]}
    counts = {"A": 600, "B": 8193, "C": 0, "D": 300 - (1 << 31), "E": 8192}
    exp = {"A": _lanms_ref(a), "B": (big["8193"][1], 8193), "C": (np.zeros((0, 9), F32), 0), "D": _lanms_ref(d), "E": (big["8192"][1], 8192)}
    assert exp["A"][1] <= 8192 and exp["D"][1] <= 8192, "A, D and E take the bit matrix, B the in-kernel loop"
    mc, ws = 8200, None
    for order in ("ABCDE", "BAECD", "BAECD"):
        rows, ws = _lanms(ops, nat, [pages[k] for k in order], mc, counts=[counts[k] for k in order], ws=ws, via_ops=False)
        for k, r in zip(order, rows):
            assert _same(r, exp[k][0]), (order, k)
    for k in "ACD":   # single-page launches (B and E alone: test_lanms_suppression_path_edges_disjoint)
        rows, _ = _lanms(ops, nat, [pages[k]], mc, counts=[counts[k]], via_ops=False)
        assert _same(rows[0], exp[k][0]), k
    print("lanms mixed launch: nm " + ", ".join(f"{k} {exp[k][1]}" for k in "ABCDE"))


# ================================================================================================ box tail
# (expand_w, expand_h, orig (h, w), target (w, h), axis_aligned, anomalies, sigma, min_count)
IDENT = (0.0, 0.0, (1000, 1000), (1000, 1000), False, False, 5.0, 30)    # output rows == kept input rows, bit for bit
PROD = (0.9, 0.9, (1250, 1500), (1000, 1000), True, True, 5.0, 30)
SUMS = (0.0, 0.0, (1250, 1500), (1000, 1000), True, True, 1.0, 5)        # anomalies on, threshold inside the area range


def _tail_args(prm):
    ew, eh, ohw, twh, aa, anom, sigma, minc = prm
    return (float(ew), float(eh), ohw[1] / twh[0], ohw[0] / twh[1], int(aa), int(anom), float(sigma), int(minc))


def tail_ref(q, prm, stages=False):
    """The oracle chain; stages=True also returns the count after the containment filter."""
    from oracle import east_post as P
    ew, eh, ohw, twh, aa, anom, sigma, minc = prm
    e = P.scale_boxes_to_original(P.expand_boxes(q.copy(), ew, eh), ohw, twh)
    e = P.remove_fully_contained_boxes(e)
    n1 = len(e)
    e = P.remove_area_anomalies(e, anom, sigma, minc)
    e = P.convert_to_axis_aligned(e) if aa else e
    return (e, n1) if stages else e


def tail_host(nat, q, prm):
    """msocr_east_box_tail_host, pinned to the oracle on these page classes by tests/test_host_cpu.py."""
    q = np.ascontiguousarray(q, dtype=F32)
    out, n = np.empty((max(len(q), 1), 9), F32), ctypes.c_int32(0)
    rc = nat.lib().msocr_east_box_tail_host(q.ctypes.data, len(q), *_tail_args(prm), out.ctypes.data, ctypes.byref(n))
    assert rc == 0
    return out[:n.value].copy()


def _tail(ops, nat, pages, mc, prm, counts=None, via_ops=True):
    N = len(pages)
    boxes = _pages_f(pages, mc)
    cnt_l = [len(p) for p in pages] if counts is None else list(counts)
    cnt = torch.tensor(cnt_l + [ISENT], dtype=torch.int32).cuda()
    nbytes = nat.lib().msocr_east_box_tail_workspace_bytes(N, mc)
    ws = _workspace(nbytes)
    out, n_out = _fguard(N, mc, 9), _iguard(N + 1)
    rc = nat.lib().msocr_east_box_tail(boxes.data_ptr(), cnt.data_ptr(), N, mc, *_tail_args(prm), out.data_ptr(), n_out.data_ptr(),
                                       ws.data_ptr(), ops._stream())
    assert rc == 0
    torch.cuda.synchronize()
    o, k = out.cpu().numpy(), n_out.cpu().numpy()
    assert k[N] == ISENT and _f_untouched(o[N]), "box tail wrote behind the last page"
    assert _ws_tail_ok(ws, nbytes), "box tail wrote behind msocr_east_box_tail_workspace_bytes"
    rows = []
    for n in range(N):
        m = int(k[n])
        assert -1 <= m <= mc and _f_untouched(o[n, max(m, 0):]), ("box tail wrote rows past its count", n, m)
        rows.append(None if m < 0 else o[n, :m].copy())
    if via_ops:
        ws2 = _workspace(nbytes)
        a = _tail_args(prm)
        o2, k2 = ops.east_box_tail(boxes[:N], cnt[:N], *a, workspace=ws2)
        o2, k2 = o2.cpu().numpy(), k2.cpu().numpy()
        assert _ws_tail_ok(ws2, nbytes) and np.array_equal(k2, k[:N])
        assert all(r is None or _same(o2[n, :len(r)], r) for n, r in enumerate(rows)), "ops.east_box_tail differs"
    return rows


def rotated_quads(rng, M):
    cx, cy = rng.random(M) * 1800, rng.random(M) * 1400
    w, h = rng.random(M) * 150 + 2, rng.random(M) * 40 + 2
    ang = (rng.random(M) - 0.5) * 0.4
    pts = np.stack([np.stack([-w / 2, -h / 2], 1), np.stack([w / 2, -h / 2], 1), np.stack([w / 2, h / 2], 1), np.stack([-w / 2, h / 2], 1)], 1)
    c, s_ = np.cos(ang), np.sin(ang)
    R = np.stack([np.stack([c, -s_], 1), np.stack([s_, c], 1)], 1)
    pts = np.einsum("mij,mkj->mki", R, pts) + np.stack([cx, cy], 1)[:, None, :]
    return np.concatenate([pts.reshape(M, 8), rng.random((M, 1))], 1).astype(F32)


def tail_content_pages(rng):
    """name -> [M, 9] f32, M <= 200: the tie and nesting cases of the containment filter."""
    pages = {}
    q = rotated_quads(rng, 120)
    for k, off in ((0, 1), (5, 31), (9, 32), (14, 33), (20, 64), (50, 2), (51, 2)):      # exact duplicates, both index orders
        q[k + off, :8] = q[k, :8]
    pages["duplicates"] = q
    # equal areas (200): four shapes on a grid; every third cell also holds a nested 8 x 4, every fifth a 10 x 10 that shares a
    # corner and two edges with its host (on-edge vertices count as inside), every seventh a same-size twin
    rows, shapes = [], [(20, 10), (10, 20), (40, 5), (25, 8)]
    for k in range(60):
        x, y = 60.0 * (k % 10), 40.0 * (k // 10)
        w, h = shapes[k % 4]
        rows.append(_rect(x, y, x + w, y + h, rng.random()))
        if k % 3 == 0:
            rows.append(_rect(x + 1, y + 1, x + 9, y + 5, rng.random()))
        if k % 5 == 0 and w >= 10 and h >= 10:
            rows.append(_rect(x, y, x + 10, y + 10, rng.random()))
        if k % 7 == 0:
            rows.append(_rect(x, y, x + w, y + h, rng.random()))
    e = np.asarray(rows, dtype=F32)
    pages["equal_areas"] = e[rng.permutation(len(e))]
    # chains A in B in C: 40 disjoint outer quads (some rotated), each with two scaled copies inside
    outer = rotated_quads(rng, 40)
    ctr = np.stack([200.0 * (np.arange(40) % 8) + 100, 120.0 * (np.arange(40) // 8) + 60], 1)
    pts = outer[:, :8].reshape(40, 4, 2)
    pts = pts - pts.mean(axis=1, keepdims=True)
    pts = pts / np.abs(pts).max(axis=(1, 2), keepdims=True) * 45.0
    ch = []
    for s in (1.0, 0.6, 0.3):
        ch.append(np.concatenate([(pts * s + ctr[:, None, :]).reshape(40, 8), rng.random((40, 1))], 1))
    c = np.concatenate(ch).astype(F32)
    pages["chains"] = c[rng.permutation(len(c))]
    return pages


def tail_kept_page(rng, K):
    """K disjoint rectangles of random size plus three nested ones the filter removes: K boxes reach the anomaly statistics."""
    rows = []
    for k in range(K):
        x, y = 70.0 * (k % 12), 40.0 * (k // 12)
        rows.append(_rect(x, y, x + rng.uniform(10, 50), y + rng.uniform(5, 25), rng.random()))
    for k in (0, K // 2, K - 1):
        x, y = 70.0 * (k % 12), 40.0 * (k // 12)
        rows.append(_rect(x + 2, y + 1, x + 6, y + 3, rng.random()))
    q = np.asarray(rows, dtype=F32)
    return q[rng.permutation(len(q))]


def test_tail_ties_and_nesting_vs_oracle(ops, nat):
    pages = tail_content_pages(np.random.default_rng([SEED, 31]))
    names = list(pages)
    for prm in (IDENT, PROD):
        refs = [tail_ref(pages[k], prm, stages=True) for k in names]
        if prm is IDENT:
            assert refs[names.index("chains")][1] == 40, "only the outer quad of each chain survives"
            assert refs[0][1] == 120 - 7, "one of every duplicate pair survives"
        rows = _tail(ops, nat, [pages[k] for k in names], 200, prm)
        wrong = []
        for k, r, (e, n1) in zip(names, rows, refs):
            print(f"tail {k} {'ident' if prm is IDENT else 'prod'}: M {len(pages[k])} kept {n1} out {len(e)}")
            if not _same(r, e):
                wrong.append(k)
        assert not wrong, wrong


@pytest.mark.parametrize("K", [7, 8, 9, 128, 129, 136])
def test_tail_anomaly_sums_at_numpy_pairwise_blocks(ops, nat, K):
    """np.mean / np.std of K f32 areas: sequential below 8, eight interleaved partial sums up to 128, recursive halves (rounded
    to a multiple of 8) above: K = 129 splits 64 + 65, 136 splits 64 + 72."""
    q = tail_kept_page(np.random.default_rng([SEED, 32, K]), K)
    e, n1 = tail_ref(q, SUMS, stages=True)
    assert n1 == K and 0 < len(e) <= K, "regime: K boxes reach the statistics"
    rows = _tail(ops, nat, [q], K + 3, SUMS)
    print(f"tail sums K={K}: out {len(e)}")
    assert _same(rows[0], e)


@pytest.mark.parametrize("mc", [96, 100])
def test_tail_full_page_and_one_box_too_many(ops, nat, mc):
    """M == max_cand fills the page (cap = 96 / 128 rounds max_cand up to a multiple of 32); M == max_cand + 1 is refused with -1
    and nothing written, although for max_cand 100 it is below the rounded capacity."""
    q = rotated_quads(np.random.default_rng([SEED, 33, mc]), mc)
    e = tail_ref(q, PROD)
    rows = _tail(ops, nat, [q, q, q], mc, PROD, counts=[mc, mc + 1, mc])
    assert rows[1] is None, "M == max_cand + 1 must give -1"
    assert _same(rows[0], e) and _same(rows[2], e)


def tail_grid_page(M):
    """M small disjoint rectangles (12 x 8 on a 20 x 14 grid, 128 per row) in index order, in which some boxes are replaced:
    nested inserts (box i lies inside box j) and exact duplicates (box j repeats box i, i < j; the stable order removes i), with i
    and j in different 32-box words: the first, second and last words, and those around word 64 and word 128, where a lane of the
    greedy wave gains its second and third keep word.  -> (quads, sorted kept indices), known by construction."""
    i = np.arange(M)
    x, y = 20.0 * (i % 128), 14.0 * (i // 128)
    sc = ((i * 7919) % 10007 + 1) / 10008.0
    q = np.stack([x, y, x + 12, y, x + 12, y + 8, x, y + 8, sc], axis=1).astype(F32)
    W = (M + 31) // 32
    words = sorted({w for w in (0, 1, 31, 63, 64, 65, 127, 128, 129, 255, 256, 511, W - 2, W - 1) if 0 <= w < W})
    slot = lambda w, r: 32 * w + r if 32 * w + r < M else None
    gone = set()
    for k in range(len(words) // 2):
        lo, hi = words[k], words[-1 - k]
        for ins, host in ((slot(lo, 0), slot(hi, 0)), (slot(hi, 1), slot(lo, 1))):      # insert low / host high, and the reverse
            if ins is not None and host is not None:
                q[ins, :8] = _rect(x[host] + 3, y[host] + 2, x[host] + 7, y[host] + 5, 0)[:8]
                gone.add(ins)
        a, b = slot(lo, 2), slot(hi, 2)                                                 # duplicates
        if a is not None and b is not None:
            q[b, :8] = q[a, :8]
            gone.add(a)
    kept = np.array([k for k in range(M) if k not in gone])
    return q, kept


@pytest.mark.parametrize("M", [2048, 2049, 4128])
def test_tail_lds_and_workspace_pages_by_construction(ops, nat, M):
    """M <= TAIL_LDSM = 2048 keeps the per-box arrays in LDS, 2049 moves them to the workspace; W = 64 / 65 / 129 keep words."""
    q, kept = tail_grid_page(M)
    assert 0 < M - len(kept) and (M + 31) // 32 in (64, 65, 129)
    rows = _tail(ops, nat, [q], M + 1, IDENT)
    assert _same(rows[0], q[kept]), "kept set known by construction"
    assert _same(tail_host(nat, q, IDENT), q[kept])
    rows = _tail(ops, nat, [q], M + 1, PROD, via_ops=False)
    assert _same(rows[0], tail_host(nat, q, PROD))
    print(f"tail grid M={M}: W {(M + 31) // 32} removed {M - len(kept)}")


def test_tail_capacity_16384_and_mixed_launch(ops, nat):
    """TAIL_CAPM = 16384 boxes is the last page the device takes (max_cand 16400, cap 16384, W 512), 16385 gives -1; and one launch
    of an LDS page, a workspace page and a refused page."""
    q, kept = tail_grid_page(16384)
    rows = _tail(ops, nat, [q, None], 16400, IDENT, counts=[16384, 16385], via_ops=False)
    assert rows[1] is None and _same(rows[0], q[kept])
    assert _same(tail_host(nat, q, IDENT), q[kept])
    small = tail_content_pages(np.random.default_rng([SEED, 31]))["equal_areas"]
    g, gk = tail_grid_page(2049)
    for rep in range(2):
        rows = _tail(ops, nat, [small, g, None, small], 2304, IDENT, counts=[len(small), 2049, 2305, len(small)], via_ops=False)
        assert rows[2] is None and _same(rows[1], g[gk]) and _same(rows[0], tail_ref(small, IDENT)) and _same(rows[3], rows[0])
    print(f"tail capacity: removed {16384 - len(kept)} of 16384")


# ================================================================================================ reading order
def polys_of(boxes_i):
    """Integer AABBs -> [n, 9] f32 quads whose vertices carry fractional parts that truncate toward zero to those integers
    (negative coordinates get negative fractions)."""
    b = np.asarray(boxes_i, dtype=np.float64).reshape(-1, 4)
    x0, y0, x1, y1 = b.T
    fr = lambda v, f: v + np.where(v < 0, -f, f)
    q = np.stack([fr(x0, .25), fr(y0, .5), fr(x1, .75), fr(y0, .25), fr(x1, .5), fr(y1, .75), fr(x0, .5), fr(y1, .25), np.full(len(b), .9)], 1)
    return q.astype(F32)


def _ro(ops, nat, pages, mc, page_hw, counts=None, img_hw=(32, 100), min_text=5, page_base=0, via_ops=True):
    """pages: list of integer-AABB lists (or None) -> per page (order, keep, desc, ncrop), numpy."""
    N = len(pages)
    boxes = _pages_f([None if p is None or len(p) == 0 else polys_of(p) for p in pages], mc)
    cnt_l = [0 if p is None else len(p) for p in pages] if counts is None else list(counts)
    cnt = torch.tensor(cnt_l + [ISENT], dtype=torch.int32).cuda()
    nbytes = nat.lib().msocr_reading_order_workspace_bytes(N, mc)
    ws = _workspace(nbytes)
    order, keep, desc, ncrop = _iguard(N + 1, mc), _iguard(N + 1, mc), _iguard(N + 1, mc, 8), _iguard(N + 1)
    rc = nat.lib().msocr_reading_order_crops(boxes.data_ptr(), cnt.data_ptr(), N, mc, page_hw[0], page_hw[1], min_text, img_hw[0], img_hw[1],
                                             0.6, float("inf"), page_base, order.data_ptr(), keep.data_ptr(), desc.data_ptr(),
                                             ncrop.data_ptr(), ws.data_ptr(), ops._stream())
    assert rc == 0
    torch.cuda.synchronize()
    o, k, d, c = order.cpu().numpy(), keep.cpu().numpy(), desc.cpu().numpy(), ncrop.cpu().numpy()
    assert c[N] == ISENT and (o[N] == ISENT).all() and (k[N] == ISENT).all() and (d[N] == ISENT).all(), "reading order wrote behind the last page"
    assert _ws_tail_ok(ws, nbytes), "reading order wrote behind msocr_reading_order_workspace_bytes"
    res = []
    for n in range(N):
        nc, m = int(c[n]), (max(cnt_l[n], 0) if int(c[n]) >= 0 else 0)
        assert -1 <= nc <= m
        assert (o[n, m:] == ISENT).all() and (k[n, m:] == ISENT).all() and (d[n, m:] == ISENT).all(), ("rows past the page's count written", n)
        res.append((o[n, :m].copy(), k[n, :m].copy(), d[n, :max(nc, 0)].copy(), nc))
    if via_ops:
        ws2 = _workspace(nbytes)
        o2, k2, d2, c2 = ops.reading_order_crops(boxes[:N], cnt[:N], page_hw, min_text, img_hw[0], img_hw[1], page_base=page_base, workspace=ws2)
        o2, k2, d2, c2 = o2.cpu().numpy(), k2.cpu().numpy(), d2.cpu().numpy(), c2.cpu().numpy()
        assert _ws_tail_ok(ws2, nbytes) and np.array_equal(c2, c[:N])
        for n, (a, b, e, nc) in enumerate(res):
            assert np.array_equal(o2[n, :len(a)], a) and np.array_equal(k2[n, :len(b)], b) and np.array_equal(d2[n, :len(e)], e), "ops differs"
    return res


def ro_python_order(boxes_i):
    """Reference (a): the oracle's sort_boxes_reading_order_with_resolutions and the first-equal-word re-match."""
    from oracle import pipeline_glue as G
    boxes = [tuple(int(v) for v in b) for b in boxes_i]
    first = {}
    for k, b in enumerate(boxes):
        first.setdefault(b, k)
    return [first[b] for b in G.sort_boxes_reading_order_with_resolutions(boxes)]


def _ro_expect(ops, boxes_i, order, page_hw, page_id, img_hw=(32, 100), min_text=5):
    """order (from a reference) -> (order, keep, desc) through the size filter and ops.crop_descriptors."""
    b = np.asarray(boxes_i, dtype=np.int64).reshape(-1, 4)[np.asarray(order, dtype=np.int64)]
    big = ((b[:, 2] - b[:, 0]) >= min_text) & ((b[:, 3] - b[:, 1]) >= min_text)
    d, kk = ops.crop_descriptors(b[big], np.full(int(big.sum()), page_id), page_hw, img_hw[0], img_hw[1])
    keep = np.zeros(len(b), dtype=np.int32)
    keep[np.flatnonzero(big)[kk]] = 1
    return np.asarray(order, dtype=np.int32), keep, d


def _ro_check(got, exp, what):
    (o, k, d, nc), (eo, ek, ed) = got, exp
    assert nc == len(ed), (what, nc, len(ed))
    assert np.array_equal(o, eo), (what, "order")
    assert np.array_equal(k, ek), (what, "keep")
    assert np.array_equal(d, ed), (what, "descriptors")


def _aabbs_from_polys(boxes_i):
    """The device's own first step restated by the oracle: np.array(polygon, int32) truncation of the f32 quads, min / max."""
    from oracle import pipeline_glue as G
    return [tuple(int(v) for v in G.word_box(p[:8].reshape(4, 2))) for p in polys_of(boxes_i)]


def ro_host_order(boxes_i):
    """msocr_reading_order_host, pinned to the Python glue by tests/test_host_cpu.py."""
    from manuscript_ocr_amd._pipeline import _reading_order
    return _reading_order(np.asarray(boxes_i, dtype=np.int32).reshape(-1, 4))


def pair_count(boxes_i):
    b = np.asarray(boxes_i, dtype=np.int64).reshape(-1, 4)
    hit = ~((b[:, None, 2] <= b[None, :, 0]) | (b[None, :, 2] <= b[:, None, 0]) | (b[:, None, 3] <= b[None, :, 1]) | (b[None, :, 3] <= b[:, None, 1]))
    return int(np.triu(hit, 1).sum())


def random_boxes(rng, n, H=600, W=900):
    x0, y0 = rng.integers(0, W, size=n), rng.integers(0, H, size=n)
    w, h = rng.integers(0, 120, size=n), rng.integers(0, 40, size=n)
    b = np.stack([x0, y0, x0 + w, y0 + h], 1)
    if n > 8:
        b[n // 2], b[n - 1] = b[0], b[1]
    return b.tolist()


def ro_content_pages(rng):
    """name -> (integer AABBs, min_text).  At most 300 boxes each."""
    pages = {}
    # intersecting boxes that end at x1 = y1 = -1: int(-1 - 0.1 * (-1 - x0)) truncates toward zero back to -1, so they never
    # shrink apart and all 50 sweeps run
    neg = []
    for k in range(20):
        x, y = -40 * k - 12, -30 * (k % 5) - 9
        neg += [[x, y, -1, -1], [x - 3, y - 2, -1, -1]]
    pages["fifty_sweeps"] = (neg + random_boxes(rng, 40), 5)
    pages["negative_fractions"] = ([[-int(a) - 3, -int(b) - 2, int(c), int(d)] for a, b, c, d in rng.integers(0, 60, size=(60, 4))]
                                   + [[-90, -50, -30, -20], [-9, -9, 0, 0], [-1, -1, 1, 1]], 5)
    pages["zero_height"] = ([[int(x), int(y), int(x) + int(w), int(y)] for x, y, w in rng.integers(0, 400, size=(80, 3))], 0)
    # two different boxes with the same corner shrink to the same box in one step (100 -> 90, 101 -> int(90.9) = 90) and stay
    # equal: the dict keeps the later original, the re-match takes the first word equal to it
    dup = []
    for k in range(12):
        x, y = 150 * (k % 4) + 7, 90 * (k // 4) + 3
        dup += [[x, y, x + 100, y + 50], [x, y, x + 101, y + 51]]
    pages["duplicate_shrunk"] = (dup + random_boxes(rng, 30), 5)
    H, W = 600, 900
    pages["page_edges"] = ([[-20, 100, 30, 140], [W - 25, 200, W + 40, 240], [300, -15, 380, 25], [400, H - 10, 470, H + 30], [-30, -20, 50, 40],
                            [W - 10, H - 10, W + 10, H + 10], [-80, 50, -10, 90], [100, -70, 160, -8], [-60, -50, -10, -5], [W + 5, 10, W + 60, 50],
                            [10, H + 3, 70, H + 40], [-5, -5, W + 5, H + 5], [-W - 50, 300, -W - 5, 340], [500, -H - 40, 560, -H - 2]]
                           + random_boxes(rng, 25), 5)
    pages["min_text_size"] = ([[10 + 40 * k, 10, 10 + 40 * k + w, 10 + h] for k, (w, h) in
                               enumerate([(5, 5), (4, 5), (5, 4), (4, 4), (6, 5), (5, 30), (30, 5), (30, 4), (4, 30)])] + random_boxes(rng, 20), 5)
    return pages


def clique_page(extra_pairs):
    """107 boxes that all intersect one another (5671 pairs) and `extra_pairs` far-away pairs."""
    b = [[2 * i, 2 * i, 600 + 2 * i, 400 + 2 * i] for i in range(107)]
    for k in range(extra_pairs):
        x = 3000 + 100 * k
        b += [[x, 0, x + 50, 30], [x + 20, 10, x + 70, 40]]
    return b


def word_grid(lines, per_line, n, rng):
    """The first n words of `lines` x `per_line` words (50 x 20 at pitch 80 x 30, no two intersect), shuffled -> (boxes, the
    reading order by construction: row-major)."""
    i = np.arange(lines * per_line)[:n]
    r, c = i // per_line, i % per_line
    b = np.stack([10 + 80 * c, 5 + 30 * r, 60 + 80 * c, 25 + 30 * r], 1)
    perm = rng.permutation(n)
    b = b[perm]
    return b.tolist(), np.lexsort((b[:, 0], b[:, 1])).tolist()


@pytest.mark.parametrize("mc", [131, 16400])
def test_reading_order_pages_of_one_launch(ops, nat, mc):
    """Outputs are strided by max_cand, the workspace by cap = min(max_cand, RO_CAP = 16384): 131 / 131 and 16400 / 16384."""
    rng = np.random.default_rng([SEED, 41])
    pages = [random_boxes(rng, 100), [], None, random_boxes(rng, 37), random_boxes(rng, 131)]
    counts = [100, 0, -1, 37, 131]
    hw = (600, 900)
    exp = [None if p is None else _ro_expect(ops, p, ro_python_order(p), hw, 3 + n) for n, p in enumerate(pages)]
    for p in pages:
        if p:
            assert _aabbs_from_polys(p) == [tuple(b) for b in p]
    for rep in range(2):
        res = _ro(ops, nat, pages, mc, hw, counts=counts, page_base=3, via_ops=rep == 0)
        assert res[2][3] == -1 and res[1][3] == 0
        for n in (0, 1, 3, 4):
            _ro_check(res[n], exp[n], (mc, n))
    for n in (0, 3, 4):   # every page alone
        got = _ro(ops, nat, [pages[n]], mc, hw, page_base=3 + n, via_ops=False)[0]
        _ro_check(got, exp[n], (mc, n, "alone"))


@pytest.mark.parametrize("n", [1023, 1024, 1025])
def test_reading_order_block_scan_edges(ops, nat, n):
    """ro_block_scan gives each of its 1024 threads per = ceil(n / 1024) elements: 1 up to 1024, 2 from 1025."""
    b, order = word_grid(-(-n // 5), 5, n, np.random.default_rng([SEED, 42, n]))
    assert pair_count(b) == 0 and ro_host_order(b) == order, "row-major by construction, and the host twin agrees"
    hw = (30 * 210, 420)
    got = _ro(ops, nat, [b], n + 3, hw)[0]
    _ro_check(got, _ro_expect(ops, b, order, hw, 0), n)
    print(f"reading order n={n}: lines {-(-n // 5)} pairs 0 crops {got[3]}")


def test_reading_order_line_and_box_capacity(ops, nat):
    """RO_MAXLINES = 4096 lines of 4 words = RO_CAP = 16384 boxes is taken; 4097 lines and 16385 boxes give -1."""
    rng = np.random.default_rng([SEED, 43])
    b, order = word_grid(4096, 4, 16384, rng)
    b1, _ = word_grid(4097, 1, 4097, rng)
    assert len({bb[1] for bb in b}) == 4096 and len({bb[1] for bb in b1}) == 4097, "regime: line count by construction"
    assert ro_host_order(b) == order
    hw = (30 * 4100, 340)
    res = _ro(ops, nat, [b, b1, None], 16400, hw, counts=[16384, 4097, 16385], via_ops=False)
    assert res[1][3] == -1 and res[2][3] == -1
    _ro_check(res[0], _ro_expect(ops, b, order, hw, 0), "4096 x 4")


def test_reading_order_pair_buffer_capacity(ops, nat):
    """cap = max_cand = 200: P = 8 * 200 + 4096 = 5696 intersecting pairs fill the pair buffer, 5697 give -1."""
    fits, over = clique_page(25), clique_page(26)
    assert pair_count(fits) == 8 * 200 + 4096 and pair_count(over) == 8 * 200 + 4097, "regime: pairs at the start of sweep 0"
    hw = (500, 6000)
    exp = _ro_expect(ops, fits, ro_python_order(fits), hw, 0)
    for rep in range(2):
        res = _ro(ops, nat, [fits, over], 200, hw, via_ops=rep == 0)
        assert res[1][3] == -1
        _ro_check(res[0], exp, "pair cap")


def test_reading_order_content_vs_python(ops, nat):
    from oracle import pipeline_glue as G
    pages = ro_content_pages(np.random.default_rng([SEED, 44]))
    hw = (600, 900)
    neg = [tuple(b) for b in pages["fifty_sweeps"][0]]
    after = G.resolve_intersections(neg)
    assert pair_count(after) >= 20, "regime: still intersecting after the 50th sweep"
    assert len({tuple(b) for b in G.resolve_intersections([tuple(b) for b in pages["duplicate_shrunk"][0]])}) < len(pages["duplicate_shrunk"][0])
    wrong = []
    for name, (b, min_text) in pages.items():
        assert len(b) <= 300 and _aabbs_from_polys(b) == [tuple(bb) for bb in b], name
        order = ro_python_order(b)
        if name == "duplicate_shrunk":
            assert len(set(order)) < len(order), "a later original replaces an earlier one"
        got = _ro(ops, nat, [b], 300, hw, min_text=min_text)[0]
        print(f"reading order {name}: n {len(b)} pairs {pair_count(b)} crops {got[3]}")
        try:
            _ro_check(got, _ro_expect(ops, b, order, hw, 0, min_text=min_text), name)
        except AssertionError as e:
            wrong.append(str(e))
    assert not wrong, wrong
