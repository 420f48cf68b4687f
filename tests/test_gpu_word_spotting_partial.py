"""Partial word spotting on the MI355X (include/msocr.h, "word spotting", "Subsequence distance"):
msocr_dtw_subsequence against the f64 yardsticks of tests/test_word_spotting_partial_cpu.py computed from the same raw frames, its
launch geometry, a WordIndex through Pipeline queried with partial=True, and msocr_dtw_distances against the bits it gave before
its product loop was factored out for both kernels (tests/golden/word_spotting_dtw_parent.npz).

The bound of d, derived and not fitted, the way tests/test_gpu_word_spotting.py derives the global distance's.  Both sides start from
the same raw f32 frames.
  * A local cost errs by at most (3 H + 8) 2^-24: H 2^-24 for any f32 summation order of a unit dot product, (H + 4) 2^-24 per
    normalised operand (that derivation, unchanged: the product loop is the same code).
  * A path from row 0 to row Lq - 1 inside Lq x Ln visits at most Lq + Ln - 1 cells, so its sum errs by at most
    (Lq + Ln - 1) (3 H + 8) 2^-24, and d divides by Lq, not by Lq + Ln: the costs' share is below (3 H + 8) 2^-24 (Lq + Ln) / Lq.
    The minimum over paths, start columns and end columns of perturbed sums moves by no more than the largest perturbation of
    a path.
  * The table's own f32 additions: at most Lq + Ln - 1 on a path, each rounding a value <= 2 (Lq + Ln) relatively by 2^-24;
    divided by Lq that is at most 2 (Lq + Ln) 2^-24 (Lq + Ln) / Lq.  The subtraction 1 - acc and the division add a few 2^-24 of
    d <= 2 (Lq + Ln) / Lq, which the global bound's "+ 16" covers after the same scaling.
  |d_dev - d_f64| <= (3 H + 2 (Lq + Ln) + 16) 2^-24 (Lq + Ln) / Lq = bound_sub(H, Lq, Ln): the global bound times (Lq + Ln) / Lq.
The span, by the validity criterion: 0 <= s < e <= Ln, and the best f64 path pinned to start at (0, s) and end at (Lq - 1, e - 1)
costs, per query frame, at most d_f64 + 2 bound_sub: the device's own path is within bound_sub of its f32 value d_dev, which is
within bound_sub of d_f64.  Spans on random frames are never compared for equality (near-ties may fall differently); on exact costs
(orthogonal one-hot frames: every cost is exactly 0 or 1 on every route) d and the span are EQUAL.

Every check prints the largest error / bound it saw (-s); DESIGN.md section 4.28 records them.  Nothing is timed here."""
import os

import numpy as np
import pytest
import torch

from test_word_spotting_cpu import full_gate, random_words, same_bits, yard_unit
from test_word_spotting_partial_cpu import (bound_sub, check_all, check_stem_index, exact_arrays, nan_behind,
                                            partial_in_blocks_and_in_one, stem_index, yard_cost, yard_pinned, yard_sub, yard_sub_all,
                                            yard_sub_results)

pytestmark = pytest.mark.gpu

CFG = {"img_h": 32, "img_w": 100, "max_len": 25, "hidden_size": 256}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "word_spotting_dtw_parent.npz")


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from manuscript_ocr_amd import _native as nat
    nat.lib()
    return torch.device("cuda")


def tile():
    from manuscript_ocr_amd import ops
    return ops.SPOT_TILE


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def device_sub(fq, ql, lo, hi, fc, cl):
    """raw frames -> (d [Q, N], span [Q, N, 2]) of the device route, as arrays"""
    from manuscript_ocr_amd import ops
    qlen, clen = dev(ql, np.int32), dev(cl, np.int32)
    uq, uc = ops.frame_normalize(dev(fq), qlen), ops.frame_normalize(dev(fc), clen)
    d, span = ops.dtw_subsequence(uq, qlen, dev(lo, np.int32), dev(hi, np.int32), uc, clen)
    torch.cuda.synchronize()
    return d.cpu().numpy(), span.cpu().numpy()


def partial_gate(ql, T, r=2.0):
    """the gate of WordIndex.spot(partial=True): ceil(L / r) .. T"""
    ql = np.asarray(ql)
    return np.maximum(-(-ql // int(r)), 1).astype(np.int32), np.full(len(ql), T, dtype=np.int32)


# ------------------------------------------------------------------------------------------------ case 1: the case grid
def grid_case(T, H):
    """lengths 1, 2, T - 1, T on both sides (so Lq > Ln is among the pairs) and ragged lengths inside one tile, 3 tiles + 7 words,
    NaN behind every length, every length admitted"""
    rng = np.random.default_rng(2000 * T + H)
    edge = sorted({1, min(2, T), max(T - 1, 1), T})
    N = 3 * tile() + 7
    fq, ql = random_words(rng, len(edge), T, H, edge)
    fc, cl = random_words(rng, N, T, H, (edge + list(rng.integers(1, T + 1, N)))[:N])
    nan_behind(fq, ql), nan_behind(fc, cl)
    return (fq, ql, *full_gate(len(ql), T), fc, cl)


def count_case(Q, N, T, H):
    """counts around the tile, ragged lengths, the partial route's gate"""
    rng = np.random.default_rng(100000 + 1000 * Q + 10 * N + T)
    fq, ql = random_words(rng, Q, T, H)
    fc, cl = random_words(rng, N, T, H)
    ql[0], cl[-1] = T, T
    nan_behind(fq, ql), nan_behind(fc, cl)
    return (fq, ql, *partial_gate(ql, T), fc, cl)


GRID = [(T, H) for T in (1, 2, 33, 64) for H in (64, 256, 512)]
COUNTS = [(Q, N, T, H) for (T, H) in ((33, 256), (64, 64)) for Q in (1, 3, 65) for N in (1, 3, 4, 5, 19)]


@pytest.mark.parametrize("T,H", GRID)
def test_sub_grid_of_shapes(cuda, T, H):
    case = grid_case(T, H)
    got = device_sub(*case)
    check_all(*got, *case, f"T {T} H {H}")
    assert (case[1][:, None] > case[5][None, :]).any() or T == 1      # Lq > Ln is among the pairs


@pytest.mark.parametrize("T,H", [(33, 256), (64, 64)])
@pytest.mark.parametrize("Q", [1, 3, 65])
def test_sub_counts_around_the_tile(cuda, Q, T, H):
    for N in (1, 3, 4, 5, 19):
        case = count_case(Q, N, T, H)
        check_all(*device_sub(*case), *case, f"Q {Q} N {N} T {T} H {H}")


# ------------------------------------------------------------------------------------------------ case 2: exactness
def test_sub_exact_cases_on_one_hot_frames(cuda):
    """the one-hot cases of tests/test_word_spotting_partial_cpu.py on the device: every pairing of their queries and words equals
    the yardstick, d and span (the hand-worked values among them: the CPU test holds the yardstick to those)"""
    for H in (64, 256):
        cases, fq, ql, fc, cl = exact_arrays(H=H)
        T = fq.shape[1]
        d, span = device_sub(fq, ql, *full_gate(len(ql), T), fc, cl)
        want, wspan = yard_sub_results(*yard_sub_all(yard_unit(fq, ql), ql, yard_unit(fc, cl), cl), ql, cl)
        assert same_bits(d, want.astype(np.float32)) and np.array_equal(span, wspan)
        for k, (name, _q, _w, want_d, want_span) in enumerate(cases):
            assert d[k, k] == np.float32(want_d) and tuple(span[k, k].tolist()) == want_span, name


def planted(rng, T, H, L, at, Ln):
    """a random query of L frames and a word of Ln random frames that holds it at columns at .. at + L - 1"""
    fq, ql = random_words(rng, 1, T, H, [L])
    fc, cl = random_words(rng, 1, T, H, [Ln])
    fc[0, at:at + L] = fq[0, :L]
    return fq[0], fc[0]


def test_sub_planted_copies(cuda):
    """Copies of a random query between random junk frames at H = 64: the copy's diagonal costs ~1e-7 a frame and every other
    alignment ~1 a frame, so the span is exact, and d <= bound.  At T = 64 the copy lies at columns 20 .. 50 and its path crosses
    the edge between two 32 x 32 blocks of the cost tile; a query of 40 frames at columns 10 .. 49 crosses it on both axes."""
    rng = np.random.default_rng(77)
    for T, H, plants in ((16, 64, [(6, 4, 13), (1, 0, 16), (5, 11, 16), (16, 0, 16)]),
                         (64, 64, [(31, 20, 64), (40, 10, 55), (3, 31, 64), (33, 31, 64)])):
        pairs = [planted(rng, T, H, L, at, Ln) for (L, at, Ln) in plants]
        fq, fc = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
        ql = np.array([p[0] for p in plants], dtype=np.int32)
        cl = np.array([p[2] for p in plants], dtype=np.int32)
        nan_behind(fq, ql), nan_behind(fc, cl)
        case = (fq, ql, *full_gate(len(ql), T), fc, cl)
        d, span = device_sub(*case)
        check_all(d, span, *case, f"planted copies T {T}")
        for k, (L, at, Ln) in enumerate(plants):
            assert span[k, k].tolist() == [at, at + L], (T, k, span[k, k].tolist())
            assert abs(d[k, k]) <= bound_sub(H, L, Ln)
        assert span[0, 0].tolist() == ([20, 51] if T == 64 else [4, 10])


# ------------------------------------------------------------------------------------------------ case 3: the envelope
def test_sub_gate_and_lengths_outside_the_envelope(cuda):
    from manuscript_ocr_amd import ops
    rng = np.random.default_rng(5)
    T, H = 33, 256
    N = 2 * tile() + 3
    fq, ql = random_words(rng, 2, T, H, [10, 20])
    fc, cl = random_words(rng, N, T, H, [5] * (N - 1) + [12])
    nan_behind(fq, ql), nan_behind(fc, cl)                 # padding frames are NaN: never read
    # the only admissible word is the last one; then nothing is admissible
    d, span = device_sub(fq, ql, [12, 12], [12, 33], fc, cl)
    check_all(d, span, fq, ql, [12, 12], [12, 33], fc, cl, "only the last word")
    assert np.isposinf(d[:, :-1]).all() and (span[:, :-1] == -1).all() and np.isfinite(d[:, -1]).all() and (span[:, -1, 0] >= 0).all()
    d, span = device_sub(fq, ql, [6, 13], [11, 33], fc, cl)
    assert np.isposinf(d).all() and (span == -1).all()
    # at len_lo, at len_hi and one outside each
    fc, cl = random_words(rng, 4, T, H, [4, 5, 9, 10])
    nan_behind(fc, cl)
    d, span = device_sub(fq[:1], ql[:1], [5], [9], fc, cl)
    check_all(d, span, fq[:1], ql[:1], [5], [9], fc, cl, "gate edges")
    assert np.isfinite(d[0]).tolist() == [False, True, True, False]
    # a length outside [1, T] cannot be refused on the device: its pairs are +inf and (-1, -1)
    cl_bad = np.array([0, 5, T + 1, -7], dtype=np.int32)
    ql_bad = np.array([10, 0, T + 1], dtype=np.int32)
    fq3 = np.concatenate([np.nan_to_num(fq), np.nan_to_num(fq[:1])])
    uq = ops.frame_normalize(dev(fq3), dev(ql_bad))
    uc = ops.frame_normalize(dev(np.nan_to_num(fc)), dev(cl_bad))
    d, span = ops.dtw_subsequence(uq, dev(ql_bad), dev([1, 1, 1], np.int32), dev([T, T, T], np.int32), uc, dev(cl_bad))
    d, span = d.cpu().numpy(), span.cpu().numpy()
    assert np.isfinite(d).tolist() == [[False, True, False, False], [False] * 4, [False] * 4]
    assert np.isposinf(d[~np.isfinite(d)]).all() and (span[~np.isfinite(d)] == -1).all() and 0 <= span[0, 1, 0] < span[0, 1, 1] <= 5
    # no query, no word; results into given tensors
    e, s = ops.dtw_subsequence(uq[:0], dev(ql_bad[:0]), dev(ql_bad[:0]), dev(ql_bad[:0]), uc, dev(cl_bad))
    assert e.shape == (0, 4) and s.shape == (0, 4, 2)
    e, s = ops.dtw_subsequence(uq, dev(ql_bad), dev(ql_bad), dev(ql_bad), uc[:0], dev(cl_bad[:0]))
    assert e.shape == (3, 0) and s.shape == (3, 0, 2)
    out, sp = torch.empty((3, 4), device="cuda"), torch.empty((3, 4, 2), dtype=torch.int32, device="cuda")
    e, s = ops.dtw_subsequence(uq, dev(ql_bad), dev([1, 1, 1], np.int32), dev([T, T, T], np.int32), uc, dev(cl_bad), out=out, span_out=sp)
    assert e is out and s is sp and same_bits(out.cpu().numpy(), d) and np.array_equal(sp.cpu().numpy(), span)


# ------------------------------------------------------------------------------------------------ case 4: launch geometry
# msocr_dtw_subsequence uses msocr_dtw_distances' grid: tiles of 4 words by `rows` query rows, about four workgroups per CU, and a
# workgroup walks the queries q = blockIdx.y, blockIdx.y + rows, ..  The tests below read the CU count, restate the host's formula
# and assert the geometry they are there for, so on a part with another CU count they either still enter their path or fail and
# say so.
def cu_count():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def grid_rows(Q, N, cu):
    tiles = -(-N // tile())
    return max(1, min(Q, 65535, -(-4 * cu // tiles)))


def check_rows_alone(fq, ql, lo, hi, fc, cl, got, what):
    """Every row of the batched result against a call that holds its query alone (a fresh LDS tile, fresh wavefront registers):
    bit for bit, d and span."""
    from manuscript_ocr_amd import ops
    qlen, clen, lo_d, hi_d = dev(ql, np.int32), dev(cl, np.int32), dev(lo, np.int32), dev(hi, np.int32)
    uq, uc = ops.frame_normalize(dev(fq), qlen), ops.frame_normalize(dev(fc), clen)
    alone = [ops.dtw_subsequence(uq[q:q + 1], qlen[q:q + 1], lo_d[q:q + 1], hi_d[q:q + 1], uc, clen) for q in range(len(ql))]
    torch.cuda.synchronize()
    d = torch.cat([a[0] for a in alone]).cpu().numpy()
    span = torch.cat([a[1] for a in alone]).cpu().numpy()
    bad = np.argwhere(d.view(np.uint32) != got[0].view(np.uint32))
    assert len(bad) == 0, (what, len(bad), bad[:8].tolist())
    assert np.array_equal(span, got[1]), (what, np.argwhere(span != got[1])[:8].tolist())


def test_sub_one_grid_row_walks_all_queries(cuda):
    """rows = 1: every workgroup takes several trips of the query loop, reusing its wave's LDS cost tile and resetting the
    wavefront's values, starts and running minimum between queries.  A short query follows a long one on the same tile; the gates
    skip pairs between computed ones."""
    cu = cu_count()
    T, H, Q = 8, 64, 5
    N = 16 * cu
    assert grid_rows(Q, N, cu) == 1
    rng = np.random.default_rng(61)
    fq, ql = random_words(rng, Q, T, H, [T, 1, T - 1, 2, T])
    fc, cl = random_words(rng, N, T, H, (list(range(1, T + 1)) + list(rng.integers(1, T + 1, N)))[:N])
    nan_behind(fq, ql), nan_behind(fc, cl)
    lo, hi = np.array([1, 1, 4, 1, 3], dtype=np.int32), np.array([T, 4, T, 2, T], dtype=np.int32)
    got = device_sub(fq, ql, lo, hi, fc, cl)
    check_all(*got, fq, ql, lo, hi, fc, cl, f"rows 1: Q {Q} N {N} T {T} H {H}")
    assert np.isfinite(got[0][:, 2]).tolist() == [True, True, False, False, True]      # a word of 3 frames
    assert np.isfinite(got[0][:, 5]).tolist() == [True, False, True, False, True]      # a word of 6 frames
    check_rows_alone(fq, ql, lo, hi, fc, cl, got, "rows 1")


@pytest.mark.parametrize("T,H", [(33, 256), (64, 64)])
def test_sub_a_few_queries_per_workgroup(cuda, T, H):
    """1 < rows < Q: the stride of the query loop is neither 1 nor Q; both tile pitches (T + 1 and T), a partial last tile, two
    blocks of the cost tile per side"""
    cu = cu_count()
    Q, N = 6, 4 * cu + 3
    rows = grid_rows(Q, N, cu)
    assert 1 < rows < Q, (rows, cu)
    rng = np.random.default_rng(62 + T)
    fq, ql = random_words(rng, Q, T, H, [T, 1, T - 1, 2, T, T // 2 + 1])
    fc, cl = random_words(rng, N, T, H)
    cl[:4] = [T, 1, T - 1, 2]
    cl[-1] = T
    nan_behind(fq, ql), nan_behind(fc, cl)
    lo, hi = partial_gate(ql, T)
    lo[4] = 1
    got = device_sub(fq, ql, lo, hi, fc, cl)
    check_all(*got, fq, ql, lo, hi, fc, cl, f"rows {rows}: Q {Q} N {N} T {T} H {H}")
    assert np.isinf(got[0]).any() and np.isfinite(got[0][4]).all()
    check_rows_alone(fq, ql, lo, hi, fc, cl, got, f"rows {rows} T {T}")


def test_sub_many_queries_one_partial_tile(cuda):
    """rows < Q with a single tile of three words: the fourth wave of every workgroup returns before the query loop while the
    other three take two trips of it"""
    cu = cu_count()
    T, H, N = 2, 64, 3
    Q = 4 * cu + 5
    rows = grid_rows(Q, N, cu)
    assert rows < Q, (rows, cu)
    rng = np.random.default_rng(63)
    fq, ql = random_words(rng, Q, T, H)
    fc, cl = random_words(rng, N, T, H, [2, 1, 2])
    nan_behind(fq, ql), nan_behind(fc, cl)
    lo = np.where(np.arange(Q) % 7 == 3, 2, 1).astype(np.int32)
    hi = np.full(Q, T, dtype=np.int32)
    got = device_sub(fq, ql, lo, hi, fc, cl)
    check_all(*got, fq, ql, lo, hi, fc, cl, f"rows {rows}: Q {Q} N {N} T {T} H {H}")
    assert np.isfinite(got[0][:, 0]).all() and np.array_equal(np.isfinite(got[0][:, 1]), lo == 1)


# ------------------------------------------------------------------------------------------------ case 5: WordIndex and Pipeline
def test_word_index_partial_on_the_device(cuda, monkeypatch):
    """the hand-built index of the CPU test on the device, and the index in blocks of 5, 5, 5, 5, 3 against the one in one block"""
    from test_word_spotting_cpu import words_for_blocks
    check_stem_index(*stem_index("cuda"))
    everything = partial_in_blocks_and_in_one(monkeypatch, "cuda")
    feat, lens, _ids, _texts, fq, ql = words_for_blocks()
    uq, uc = yard_unit(fq, ql), yard_unit(feat, lens)
    for q, hits in enumerate(everything):
        assert [h.distance for h in hits] == sorted(h.distance for h in hits)
        for h in hits:
            want, _ = yard_sub(yard_cost(uq[q], ql[q], uc[h.word], lens[h.word]))
            assert abs(h.distance - want) <= bound_sub(64, ql[q], lens[h.word])


@pytest.fixture(scope="module")
def rec(cuda):
    from manuscript_ocr_amd import synth
    from manuscript_ocr_amd.recognizers import TRBA
    return TRBA(state_dict=synth.trba_state_dict_confident(194, 256, seed=3), config=CFG, device="cuda")


def test_partial_through_the_pipeline(cuda, rec):
    from manuscript_ocr_amd import Pipeline, synth
    from manuscript_ocr_amd.detectors import EAST
    from manuscript_ocr_amd.detectors._types import PartSpotHit
    H, W = 224, 320
    pipe = Pipeline(EAST(state_dict=synth.east_state_dict(), target_size=(W, H), device="cuda"), rec)
    img, rects = synth.synth_page(41, H, W)
    score, geo = synth.synth_maps(rects, (H, W), (H // 4, W // 4), 41)
    page = pipe.predict_batch([img], _maps_override=(torch.from_numpy(score)[None].cuda(), torch.from_numpy(geo)[None].cuda()))[0]
    index = pipe.index_words([img, img], pages=[page, page])
    words = page.blocks[0].words
    n = len(index) // 2
    assert n >= 4
    T, Hd = index.T, index.H
    # the f64 yardstick over the same raw frames: the index's own cut, embedded once more (the encoder is deterministic)
    kept = [words[w] for (_, _, w) in index.ids[:n]]
    canv, new_w, rows = index._cut(np.ascontiguousarray(img), kept)
    raw, lens = rec.embed_canvases(canv, new_w)
    raw = np.concatenate([raw.cpu().numpy()] * 2)
    lens = np.concatenate([lens] * 2)
    unit = yard_unit(raw, lens)
    k = 5
    refs = [index.ids[j] for j in (0, n - 1, n + 1)]
    got = pipe.spot(index, refs, k=k, partial=True)
    worst = 0.0
    for q, ref in enumerate(refs):
        row = index.ids.index(ref)
        L = int(lens[row])
        lo = -(-L // 2)
        S, st = yard_sub_all(unit[row:row + 1], lens[row:row + 1], unit, lens)
        want, _ = yard_sub_results(S, st, lens[row:row + 1], lens)
        want = np.where(lens >= lo, want[0], np.inf)
        hits = got[q]
        assert all(type(h) is PartSpotHit for h in hits)
        lim = [bound_sub(Hd, L, lens[index.ids.index((h.page, h.block, h.word))]) for h in hits]
        # a reference query finds itself and its identical twin of the other page copy: span [0, L), distance about 0, equal bits
        assert (hits[0].page, hits[0].block, hits[0].word) == (0,) + ref[1:] and abs(hits[0].distance) <= lim[0]
        assert (hits[1].page, hits[1].block, hits[1].word) == (1,) + ref[1:] and hits[1].distance == hits[0].distance
        for h in hits[:2]:
            assert (h.frame_start, h.frame_end, h.fraction) == (0, L, (0.0, 1.0))
        assert [h.rank for h in hits] == list(range(len(hits))) and len(hits) == min(k, int(np.isfinite(want).sum()))
        assert [h.distance for h in hits] == sorted(h.distance for h in hits)
        kth = np.sort(want[np.isfinite(want)])[len(hits) - 1]
        for h, b in zip(hits, lim):
            i = index.ids.index((h.page, h.block, h.word))
            assert abs(h.distance - want[i]) <= b
            worst = max(worst, abs(h.distance - want[i]) / b)
            assert want[i] <= kth + 2 * b
            assert 0 <= h.frame_start < h.frame_end <= lens[i] and h.fraction == (h.frame_start / lens[i], h.frame_end / lens[i])
            assert yard_pinned(yard_cost(unit[row], L, unit[i], lens[i]), h.frame_start, h.frame_end - 1) <= want[i] + 2 * b
    print(f"index through the pipeline, partial: worst error / bound {worst:.4f}")
    # by (image, polygon): the word's own polygon, cut the pipeline's way (one canvas through the encoder alone need not give the
    # bits it gives inside a page's batch, so: about 0, not equal)
    w0 = index.ids[1][2]
    L0 = int(lens[1])
    by_polygon = pipe.spot(index, [(img, words[w0].polygon), index.ids[1]], k=k, partial=True)
    assert [(h.page, h.word) for h in by_polygon[0][:2]] == [(0, w0), (1, w0)] == [(h.page, h.word) for h in by_polygon[1][:2]]
    assert abs(by_polygon[0][0].distance) <= bound_sub(Hd, T, T) and (by_polygon[0][0].frame_start, by_polygon[0][0].frame_end) == (0, L0)
    assert by_polygon[0][0].query == 0 and by_polygon[1][0].query == 1
    # by a crop image: the word's window of the page, embedded as TRBA.embed embeds an image (the host's ResizeAndPadA is the
    # device crop's, byte for byte: the same frames as the indexed word's)
    p = np.array(words[w0].polygon, dtype=np.int32)
    (x0, y0), (x1, y1) = p.min(0), p.max(0)
    window = np.ascontiguousarray(img[max(0, y0):min(H, y1), max(0, x0):min(W, x1)])
    by_image = index.spot([window], k=k, partial=True)[0]
    print(f"image query, partial: {[((h.page, h.word), round(h.distance, 6), (h.frame_start, h.frame_end)) for h in by_image]}")
    assert by_image[0].word == w0 and abs(by_image[0].distance) <= bound_sub(Hd, T, T)
    assert (by_image[0].frame_start, by_image[0].frame_end) == (0, L0)
    # partial=False through the pipeline is the call without the argument
    assert [[h.model_dump() for h in hs] for hs in pipe.spot(index, refs, k=k, partial=False)] == \
           [[h.model_dump() for h in hs] for hs in pipe.spot(index, refs, k=k)]


# ------------------------------------------------------------------------------------------------ case 6: msocr_dtw_distances' bits
def dtw_distances_of_the_cases():
    """ops.dtw_distances on the arrays of case 1, in their order, flattened into one f32 array"""
    from manuscript_ocr_amd import ops
    out = []
    for case in [grid_case(T, H) for (T, H) in GRID] + [count_case(*c) for c in COUNTS]:
        fq, ql, lo, hi, fc, cl = case
        qlen, clen = dev(ql, np.int32), dev(cl, np.int32)
        uq, uc = ops.frame_normalize(dev(fq), qlen), ops.frame_normalize(dev(fc), clen)
        out.append(ops.dtw_distances(uq, qlen, dev(lo, np.int32), dev(hi, np.int32), uc, clen).cpu().numpy().reshape(-1))
    return np.concatenate(out)


def test_dtw_distances_keeps_its_bits(cuda):
    """ws_dtw_kernel now shares its product-and-store part with ws_dtw_sub_kernel.  Its results on the arrays of case 1 are, bit
    for bit, the ones recorded from the same calls on an MI355X with the build before the factoring (`dist`, f32, flattened in the
    order of the cases)."""
    want = np.load(GOLDEN)["dist"]
    got = dtw_distances_of_the_cases()
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert len(bad) == 0, (len(bad), bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())
    assert np.isfinite(want).sum() > 2000 and np.isposinf(want).any()
