"""msocr_text_search_weighted on the MI355X against its host twin msocr_text_search_weighted_host, which
tests/test_text_search_weighted_cpu.py holds to a plain table.  Hits are integers: every comparison is equality, after
text_search_select or a canonical sort (the device writes its hits in no particular order).

Sizes follow L = MSOCR_SEARCH_SEGMENT, the tokens one lane of the scan kernel reports, and the kernel's groups of 8 positions: patterns
on both sides of a group boundary, the full column and the single cell; copies planted around the cuts and exactly a warm-up in front
of one; the window at its cap of 256; ragged batches; more segments than a workgroup has lanes; every lane appending at once;
capacities below the count; the alphabet caps; token arrays off the 16-byte boundary with junk around them; and one case per capped
grid dimension that enters the second trip of its stride loop."""
import numpy as np
import pytest

from test_text_search_cpu import canonical, csr
from test_text_search_weighted_cpu import host, make_costs, random_costs

pytestmark = pytest.mark.gpu

SCAN_ROWS = 65535   # gridDim.y of tsw_scan_kernel at most: patterns
SCAN_COLS = 4096    # gridDim.x at most: blocks of 256 segments


def seg():
    from manuscript_ocr_amd import ops
    return ops.SEARCH_SEGMENT


def device(patterns, ks, texts, v, tok_class, costs, capacity=None):
    """ops.text_search_weighted (both passes of its overflow protocol if need be) -> hits [count, 5] as the device wrote them"""
    import torch
    from manuscript_ocr_amd import ops
    pat_tok, pat_off = csr(patterns)
    txt_tok, txt_off = csr(texts)
    kw = {} if capacity is None else {"capacity": capacity}
    return ops.text_search_weighted(torch.from_numpy(pat_tok).cuda(), pat_off, ks, torch.from_numpy(txt_tok).cuda(), txt_off, v,
                                    torch.from_numpy(np.ascontiguousarray(tok_class, dtype=np.int32)).cuda(), costs, **kw)


def same_as_host(patterns, ks, texts, v, tok_class, costs):
    from manuscript_ocr_amd import ops
    want, count = host(patterns, ks, texts, v, tok_class, costs)
    got = device(patterns, ks, texts, v, tok_class, costs)
    assert len(got) == count
    assert np.array_equal(canonical(got), want)
    assert np.array_equal(ops.text_search_select(got), ops.text_search_select(want))
    return want


def cut_costs(rng, V):
    """deletes of 3 to 9, so that a bound of the whole pattern's cost - 1 (at most 64 * 9 - 1) stays inside the window cap:
    64 + 575 // 3 = 255; one cheap and one dear substitution between classes 0, 1, 2"""
    sub = rng.integers(2, 9, (V, V))
    np.fill_diagonal(sub, 0)
    sub[1, 0], sub[2, 0] = 1, 9      # reading a recognised 1 as a true 0 is cheap, a recognised 2 as a true 0 dear
    return make_costs(sub, rng.integers(3, 10, V), rng.integers(1, 10, V), 7)


def ins_sum(a, tok_class, costs):
    cls = np.asarray(tok_class)[np.asarray(a)]
    return int(np.where(cls >= 0, costs.insert[np.maximum(cls, 0)], costs.unknown).sum())


@pytest.mark.parametrize("m", [1, 5, 8, 9, 63, 64])
def test_cuts_and_the_first_token_after_the_warm_up(m):
    L = seg()
    rng = np.random.default_rng(400 + m)
    v, V = 40, 12
    costs = cut_costs(rng, V)
    tok_class = rng.integers(0, V, v).astype(np.int32)
    tok_class[:3] = (0, 1, 2)
    tok_class[[11, 12]] = -1
    a = rng.integers(3, v, m).astype(np.int32)
    a[m // 2] = 0                                     # the token the two substitutions are made at
    full = ins_sum(a, tok_class, costs)
    dmin = min(costs.min_del, costs.unknown)
    ks = sorted({0, min(4, full - 1), full - 1})
    texts = [rng.integers(0, v, n).astype(np.int32) for n in (L - 1, L, L + 1, 2 * L - 1, 2 * L + 1, 3 * L + 7)]
    planted_at = []
    for k in ks:
        W = m + k // dmin
        assert W <= 256
        cut = -(-W // L) * L                          # the first cut with room for the warm-up before it
        for end in (L - 1, L, L + 1, L + W, cut - W + m, cut + m):   # the last two: a start exactly W before a cut, and at it
            if end - m < 0:
                continue
            b = rng.integers(0, v, max(3 * L + 7, end + 3)).astype(np.int32)
            b[end - m:end] = a
            texts.append(b)
            planted_at.append((len(texts) - 1, end))
            for wrong in (1, 2):                      # the same copy with the cheap / the dear substitution and a token dropped in front
                noisy = b.copy()
                noisy[end - m + m // 2] = wrong
                texts.append(np.delete(noisy, max(end - m - 1, 0)))
    want = same_as_host([a] * len(ks), ks, texts, v, tok_class, costs)
    exact = {(h[1], h[3]) for h in want.tolist() if h[0] == 0 and h[4] == 0}
    assert all(p in exact for p in planted_at)
    counts = [int((want[:, 0] == q).sum()) for q in range(len(ks))]
    assert counts == sorted(counts) and counts[-1] > counts[0]


def test_a_window_at_the_cap():
    """W = 256 with m = 64 and a cheapest delete of 1: the warm-up crosses four segments and is clamped at the text's start"""
    L = seg()
    rng = np.random.default_rng(41)
    v = V = 6
    sub = rng.integers(1, 9, (V, V))
    np.fill_diagonal(sub, 0)
    delete = rng.integers(1, 4, V)
    delete[0] = 1
    costs = make_costs(sub, delete, rng.integers(4, 10, V), 5)
    cls = np.arange(v, dtype=np.int32)
    a = rng.integers(0, v, 64).astype(np.int32)
    k = 192
    assert ins_sum(a, cls, costs) > k and 64 + k // 1 == 256
    stretched = np.insert(a, np.sort(rng.integers(1, 64, 150)), 0)   # the pattern with 150 cheap tokens to drop inside it: 214 tokens
    texts = [np.concatenate([rng.integers(0, v, 30), stretched, rng.integers(0, v, 5 * L - 244 + 9)]).astype(np.int32),
             stretched.astype(np.int32), rng.integers(0, v, 6 * L).astype(np.int32), a[:40]]
    want = same_as_host([a, a[:63]], [k, k], texts, v, cls, costs)
    # dropping the 150 tokens costs 150; a cheaper alignment may exist, and the shortest substring may begin behind the copy's start
    assert any(h[0] == 0 and h[1] == 1 and h[3] == 214 and h[4] <= 150 for h in want.tolist())
    assert any(h[0] == 0 and h[1] == 0 and h[3] == 244 and h[4] <= 150 for h in want.tolist())
    assert (want[:, 3] - want[:, 2]).max() > 3 * L and (want[:, 1] == 2).any()


def test_ragged_batch_text_boundaries():
    """about 40 texts with empty ones between them; texts end with the first half of a pattern where the next begins with the second"""
    L = seg()
    rng = np.random.default_rng(71)
    v, V = 30, 9
    costs = random_costs(rng, V, top=5)
    tok_class = rng.integers(-1, V, v).astype(np.int32)
    a = rng.integers(0, v, 12).astype(np.int32)
    c = rng.integers(0, v, 64).astype(np.int32)
    empty = np.zeros(0, dtype=np.int32)
    texts = []
    for n in rng.integers(0, 3 * L, 26).tolist():
        texts.append(rng.integers(0, v, n).astype(np.int32))
        if len(texts) % 4 == 0:
            texts.append(empty)
    texts += [a[:11], a[:6], a[6:], empty, a[:6], empty, a[6:], a, c[:40], c[40:], c,
              np.concatenate([rng.integers(0, v, L - 6).astype(np.int32), a[:6]]), np.concatenate([a[6:], rng.integers(0, v, L).astype(np.int32)])]
    texts = [empty] + texts + [empty]
    want = same_as_host([a, c, a], [5, 20, 0], texts, v, tok_class, costs)
    whole = [t for t, b in enumerate(texts) if len(b) == 12 and np.array_equal(b, a)]
    assert [h[1] for h in want.tolist() if h[0] == 2] == whole and len(whole) == 1
    assert len(want[want[:, 0] == 0]) >= 2 and len(want[want[:, 0] == 1]) >= 1


@pytest.mark.parametrize("Q", [1, 3])
def test_more_segments_than_a_workgroup_has_lanes(Q):
    L = seg()
    rng = np.random.default_rng(80 + Q)
    v = V = 4
    costs = random_costs(rng, V, top=3)
    cls = np.arange(v, dtype=np.int32)
    text = rng.integers(0, v, 256 * L + 1).astype(np.int32)
    patterns = [rng.integers(0, v, int(m)).astype(np.int32) for m in rng.integers(6, 12, Q)]
    patterns[0] = text[-7:].copy()            # the last pattern token is the text's last token, alone in its segment
    want = same_as_host(patterns, [3] * Q, [text, text[:L + 3]], v, cls, costs)
    assert [0, 0, 256 * L - 6, 256 * L + 1, 0] in want.tolist() and len(want) >= 100 * Q


def test_dense_hits_every_lane_appends():
    """the one-symbol text of 4 L tokens under a bound one below the pattern's cost: every end is a hit"""
    L = seg()
    n = 4 * L
    costs = make_costs([[0]], [2], [3], 4)
    zeros = lambda k: np.zeros(k, dtype=np.int32)  # noqa: E731
    shapes = [(1, 2), (5, 14), (64, 191), (64, 0), (33, 20)]
    texts = [zeros(n), zeros(0), zeros(n), zeros(L + 1)]
    want = same_as_host([zeros(m) for m, _ in shapes], [k for _, k in shapes], texts, 1, [0], costs)
    # the end j costs 3 * max(m - j, 0): a hit from m - k // 3 on
    assert len(want) == sum(max(0, length - max(m - k // 3, 1) + 1) for m, k in shapes for length in (n, n, L + 1))


def test_capacities_guard_rows_and_the_workspace_guard():
    import torch
    from manuscript_ocr_amd import ops
    L = seg()
    rng = np.random.default_rng(91)
    v, V = 3, 3
    costs = random_costs(rng, V, top=3)
    cls = np.arange(v, dtype=np.int32)
    patterns = [rng.integers(0, v, m).astype(np.int32) for m in (4, 9, 30)]
    ks = [2, 6, 25]
    texts = [rng.integers(0, v, n).astype(np.int32) for n in (3 * L + 7, 0, 5 * L)]
    full, count = host(patterns, ks, texts, v, cls, costs)
    members = set(map(tuple, full.tolist()))
    assert count == len(members) > 300
    pat_tok, pat_off = csr(patterns)
    txt_tok, txt_off = csr(texts)
    pd, td, cd = torch.from_numpy(pat_tok).cuda(), torch.from_numpy(txt_tok).cuda(), torch.from_numpy(cls).cuda()
    for cap in (0, 1, count - 1, count, count + 9):
        buf = torch.full((cap + 16, 5), -7, dtype=torch.int32, device="cuda")
        cnt = torch.full((1,), -7, dtype=torch.int64, device="cuda")
        ops.text_search_weighted_into(pd, pat_off, ks, td, txt_off, v, cd, costs, buf[:cap], cnt)
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert int(cnt.item()) == count, cap
        written = min(cap, count)
        rows = list(map(tuple, got[:written].tolist()))
        assert all(r in members for r in rows) and len(set(rows)) == written, cap   # true hits, all distinct
        assert (got[written:] == -7).all(), cap                                        # the guard behind hits_out[capacity]
    for cap in (0, 1, count - 1, count):                                               # the two-pass protocol
        assert np.array_equal(canonical(device(patterns, ks, texts, v, cls, costs, capacity=cap)), full), cap
    need = ops.text_search_weighted_workspace_bytes(pat_off, ks, txt_off, v, costs)
    ws = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    buf = torch.empty((count, 5), dtype=torch.int32, device="cuda")
    cnt = torch.zeros((1,), dtype=torch.int64, device="cuda")
    ops.text_search_weighted_into(pd, pat_off, ks, td, txt_off, v, cd, costs, buf, cnt, workspace=ws[:need])
    torch.cuda.synchronize()
    assert np.array_equal(canonical(buf.cpu().numpy()), full) and bool((ws[need:] == 0xA5).all())


def test_alphabets_of_one_and_of_the_caps_and_foreign_tokens():
    from manuscript_ocr_amd import ops
    L = seg()
    rng = np.random.default_rng(101)
    # v = 1 and V = 1: one profile row beside the foreign row; every other token costs `unknown`
    one = make_costs([[0]], [2], [3], 4)
    mixed = (rng.random(3 * L + 7) < 0.2).astype(np.int32)
    same_as_host([np.zeros(3, dtype=np.int32), np.array([0, 1, 0], dtype=np.int32)], [3, 6], [mixed, np.zeros(L, dtype=np.int32)], 1, [0], one)
    # v = 768 with 768 distinct text symbols and V = 512: the whole LDS profile is built and read
    v, V = ops.SEARCH_W_MAX_ALPHABET, 512
    costs = random_costs(rng, V, top=9)
    tok_class = (np.arange(v) % V).astype(np.int32)
    tok_class[rng.integers(0, v, 40)] = -1
    text = rng.permutation(v).astype(np.int32)
    part = text[300:340]
    twin = np.where(part < v - V, part + V, np.where(part >= V, part - V, part)).astype(np.int32)  # another token of the same class
    twin_cost = int(((twin != part) & ((tok_class[part] < 0) | (tok_class[twin] < 0))).sum()) * costs.unknown
    patterns = [text[100:164].copy(), text[v - 5:].copy(), np.array([v - 1, v - 2, 0, 1], dtype=np.int32), text[L - 3:L + 4].copy(), twin]
    patterns[0][10] = v          # foreign tokens in the pattern
    patterns[0][20] = -1
    assert (twin != part).sum() > 20
    want = same_as_host(patterns, [2 * costs.unknown, 0, 4, 0, twin_cost], [text, text[::-1].copy(), text[:L]], v, tok_class, costs)
    rows = want.tolist()
    assert [0, 0, 100, 164, 2 * costs.unknown] in rows and [1, 0, v - 5, v, 0] in rows and [3, 0, L - 3, L + 4, 0] in rows
    assert any(h[0] == 4 and h[1] == 0 and h[3] == 340 and h[4] <= twin_cost for h in rows)   # tokens of one class cost the diagonal
    # foreign tokens on both sides, garbage included, and garbage classes
    big = 2**31 - 1
    wild = np.array([-1, 6, big, -2**31, 1, 2, 3], dtype=np.int32)
    patterns = [wild[rng.integers(0, 7, m)] for m in (4, 33, 64)]
    texts = [wild[rng.integers(0, 7, n)] for n in (0, L + 6, 5 * L)]
    few = random_costs(rng, 5, top=4)
    same_as_host(patterns, [6, 40, 90], texts, 6, [0, 1, 7, -2**31, 4, 4], few)


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_token_arrays_off_the_16_byte_boundary_with_junk_around_them(shift):
    """both token arrays are the views buf[shift:] of a fresh allocation, the first offsets lie above 0, and the junk before
    txt_off[0] ends with the first half of a pattern whose second half opens text 0, the junk behind txt_off[T] completes a pattern
    that the last text begins: a read across either edge makes a hit the host twin, given the same arrays, does not have"""
    import torch
    from manuscript_ocr_amd import ops
    L = seg()
    rng = np.random.default_rng(320)
    v, V = 30, 30
    costs = cut_costs(rng, V)
    cls = np.arange(v, dtype=np.int32)
    a = rng.integers(0, v, 12).astype(np.int32)
    c = rng.integers(0, v, 9).astype(np.int32)
    rnd = lambda n: rng.integers(0, v, n).astype(np.int32)  # noqa: E731
    texts = [np.concatenate([a[6:], rnd(L + 2), a, rnd(5)]), np.zeros(0, dtype=np.int32), rnd(2 * L - 1), np.concatenate([rnd(L - 3), a, a[:6]])]
    patterns, ks = [a, a, c[3:6], a[:7]], [0, 8, 0, 3]
    clean, count = host(patterns, ks, texts, v, cls, costs)
    txt_tok, txt_off = csr(texts)
    pat_tok, pat_off = csr(patterns)
    before_t, after_t = np.concatenate([rnd(7), a[:6]]), np.concatenate([a[6:], rnd(6)])
    before_p, after_p = c[:3], c[6:]
    txt_tok, txt_off = np.concatenate([before_t, txt_tok, after_t]), txt_off + len(before_t)
    pat_tok, pat_off = np.concatenate([before_p, pat_tok, after_p]), pat_off + len(before_p)
    assert txt_off[0] == 13 and pat_off[0] == 3
    want, n = ops.text_search_weighted_host(pat_tok, pat_off, ks, txt_tok, txt_off, v, cls, costs)
    assert n == count and np.array_equal(want, clean)       # the host twin reads nothing outside the offsets
    views = []
    for tok in (pat_tok, txt_tok):
        buf = torch.full((shift + len(tok),), -3, dtype=torch.int32, device="cuda")
        buf[shift:] = torch.from_numpy(np.ascontiguousarray(tok, dtype=np.int32)).cuda()
        views.append(buf[shift:])
        assert views[-1].data_ptr() % 16 == 4 * shift and views[-1].is_contiguous()
    got = ops.text_search_weighted(views[0], pat_off, ks, views[1], txt_off, v, torch.from_numpy(cls).cuda(), costs)
    assert len(got) == count
    assert np.array_equal(canonical(got), want)
    assert np.array_equal(ops.text_search_select(got), ops.text_search_select(want))
    exact = [h for h in want.tolist() if h[0] == 0]
    assert [(h[1], h[2], h[3]) for h in exact] == [(0, 6 + L + 2, 6 + L + 2 + 12), (3, L - 3, L + 9)]  # the two whole copies, no half


def test_more_patterns_than_grid_rows():
    """a workgroup handles a second pattern (q += gridDim.y): 65 539 two-token patterns against at most 65 535 grid rows; it then
    builds another profile over the one in LDS, between the barriers at the loop's head"""
    L = seg()
    Q = SCAN_ROWS + 4
    rng = np.random.default_rng(340)
    v = V = 16
    costs = random_costs(rng, V, top=6)
    cls = np.arange(v, dtype=np.int32)
    texts = [rng.integers(0, v, L + 6).astype(np.int32), rng.integers(0, v, L + 9).astype(np.int32)]
    patterns = list(rng.integers(0, v, (Q, 2)).astype(np.int32))
    ks = [0] * Q
    for q in (7, 30000, SCAN_ROWS - 1):                       # a few of three tokens within a small cost
        patterns[q], ks[q] = rng.integers(0, v, 3).astype(np.int32), 2
    known = []
    for j, (t, s) in enumerate(((0, 10), (0, L - 1), (1, 10), (1, L - 1))):
        patterns[SCAN_ROWS + j] = texts[t][s:s + 2].copy()
        known.append([SCAN_ROWS + j, t, s, s + 2, 0])
    want = same_as_host(patterns, ks, texts, v, cls, costs)
    rows = want.tolist()
    assert all(h in rows for h in known)
    assert (want[:, 0] >= SCAN_ROWS).sum() >= 4 and len(np.unique(want[:, 0])) > 10000


def test_more_segment_blocks_than_grid_columns():
    """a workgroup handles a second block of 256 segments (sb += gridDim.x): 4096 * 256 + 300 texts of one or two tokens against at
    most 4096 grid columns; the texts of the second trip hold known hits"""
    T = SCAN_COLS * 256 + 300
    rng = np.random.default_rng(350)
    v = V = 16
    costs = random_costs(rng, V, top=6)
    cls = np.arange(v, dtype=np.int32)
    lengths = np.ones(T, dtype=np.int64)
    lengths[-200:] = 2
    txt_off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    txt_tok = rng.integers(0, v, int(txt_off[-1])).astype(np.int32)
    txt_tok[txt_off[T - 5]:txt_off[T - 5] + 2] = (3, 9)
    import torch
    from manuscript_ocr_amd import ops
    pat_tok, pat_off, ks = np.array([3, 9], dtype=np.int32), np.array([0, 2], dtype=np.int32), [0]
    want, count = ops.text_search_weighted_host(pat_tok, pat_off, ks, txt_tok, txt_off, v, cls, costs)
    got = ops.text_search_weighted(torch.from_numpy(pat_tok).cuda(), pat_off, ks, torch.from_numpy(txt_tok).cuda(), txt_off, v,
                                   torch.from_numpy(cls).cuda(), costs)
    assert len(got) == count and np.array_equal(canonical(got), want)
    assert [0, T - 5, 0, 2, 0] in want.tolist() and (want[:, 1] >= SCAN_COLS * 256).all()
    # one token: hits in both trips
    pat_tok, pat_off = np.array([5], dtype=np.int32), np.array([0, 1], dtype=np.int32)
    want, count = ops.text_search_weighted_host(pat_tok, pat_off, ks, txt_tok, txt_off, v, cls, costs)
    got = ops.text_search_weighted(torch.from_numpy(pat_tok).cuda(), pat_off, ks, torch.from_numpy(txt_tok).cuda(), txt_off, v,
                                   torch.from_numpy(cls).cuda(), costs)
    assert len(got) == count > 60000 and np.array_equal(canonical(got), want)
    assert (want[:, 1] < SCAN_COLS * 256).any() and (want[:, 1] >= SCAN_COLS * 256).any()


def test_uniform_costs_on_the_device_are_the_unit_search():
    import torch
    from manuscript_ocr_amd import ops
    from manuscript_ocr_amd.recognizers import EditCosts
    L = seg()
    rng = np.random.default_rng(360)
    v = 20
    patterns = [rng.integers(0, v, m).astype(np.int32) for m in (1, 5, 8, 9, 63, 64)]
    ks = [0, 2, 3, 3, 20, 63]
    texts = [rng.integers(0, v + 1, n).astype(np.int32) for n in (L - 1, 0, 2 * L + 1, 3 * L + 7)]
    texts.append(np.concatenate([patterns[4], patterns[5][:60], patterns[3]]))
    pat_tok, pat_off = csr(patterns)
    txt_tok, txt_off = csr(texts)
    pd, td = torch.from_numpy(pat_tok).cuda(), torch.from_numpy(txt_tok).cuda()
    unit = canonical(ops.text_search(pd, pat_off, ks, td, txt_off, v))
    assert len(unit) > 100
    costs = EditCosts.uniform([f"<{k}>" for k in range(v)], 1)
    for cls in (np.arange(v, dtype=np.int32), np.full(v, -1, dtype=np.int32)):   # inside the charset, and outside it
        got = ops.text_search_weighted(pd, pat_off, ks, td, txt_off, v, torch.from_numpy(cls).cuda(), costs)
        assert np.array_equal(canonical(got), unit)


def test_no_patterns_no_texts_and_empty_texts_only():
    import torch
    from manuscript_ocr_amd import ops
    costs = make_costs([[0]], [2], [3], 4)
    none = torch.zeros(0, dtype=torch.int32, device="cuda")
    some = torch.zeros(9, dtype=torch.int32, device="cuda")
    cls = torch.zeros(4, dtype=torch.int32, device="cuda")
    assert ops.text_search_weighted(none, [0], [], some, [0, 9], 4, cls, costs).shape == (0, 5)
    assert ops.text_search_weighted(some, [0, 9], [2], none, [0], 4, cls, costs).shape == (0, 5)
    assert ops.text_search_weighted(some, [0, 9], [2], none, [0, 0, 0], 4, cls, costs).shape == (0, 5)
    cnt = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    ops.text_search_weighted_into(none, [0], [], some, [0, 9], 4, cls, costs, torch.empty((0, 5), dtype=torch.int32, device="cuda"), cnt)
    assert int(cnt.item()) == 0


def letter_costs(rng, charset):
    V = len(charset)
    sub = rng.integers(2, 7, (V, V))
    np.fill_diagonal(sub, 0)
    from manuscript_ocr_amd.recognizers import EditCosts
    return EditCosts(sub, rng.integers(1, 7, V), rng.integers(2, 7, V), charset, unknown=6)


def test_text_corpus_and_page_corpus_resident_on_the_device():
    from manuscript_ocr_amd import PageCorpus
    from manuscript_ocr_amd.recognizers import TextCorpus, search_texts
    from test_text_search_cpu import hand_pages
    rng = np.random.default_rng(111)
    letters = np.array(list("abcdefghijklmnopqrstuvwxyz "))
    costs = letter_costs(rng, list("abcdefghijklmnopqrstuvw"))     # x, y, z and the space lie outside the charset
    texts = ["".join(letters[rng.integers(0, 27, int(n))]) for n in rng.integers(0, 700, 24)] + ["", "needle in a haystack"]
    first = [texts[3][40:52], texts[5][10:18], "needle", "haystick", "zzzzzq"]
    second = [texts[7][5:30], "in a", "e"]
    corpus = TextCorpus(texts, device="cuda")
    for queries, bound in ((first, dict(max_distance=4)), (second, dict(max_error_rate=0.2)), (first, dict(max_error_rate=0.15, overlapping=True))):
        got = corpus.search(queries, costs=costs, **bound)
        assert got == search_texts(queries, texts, device="cuda", costs=costs, **bound)
        assert got == search_texts(queries, texts, costs=costs, **bound) and len(got) > 0   # the device route equals the host route
    host_cls, dev_cls = corpus.token_classes(costs)
    assert dev_cls.is_cuda and corpus.token_classes(costs)[1] is dev_cls and np.array_equal(dev_cls.cpu().numpy(), host_cls)
    pages = hand_pages()
    page_costs = letter_costs(rng, sorted(set("alphabetagammadelta")))
    for bound in (dict(max_distance=[3, 3, 1]), dict(max_error_rate=0.2, overlapping=True)):   # "a" costs 2 or more to supply
        on_dev = PageCorpus(pages, device="cuda").search(["beta gamma", "delta", "a"], costs=page_costs, **bound)
        assert on_dev == PageCorpus(pages).search(["beta gamma", "delta", "a"], costs=page_costs, **bound) and len(on_dev) > 0


def test_pipeline_search_with_costs_and_the_package_plugins():
    """Pipeline.search(costs=) with this package's detector and recogniser on one synthetic page, costs over the recogniser's own
    charset, queries taken from the decode's own texts: the device route equals the host route"""
    from manuscript_ocr_amd import PageCorpus, Pipeline, synth
    from manuscript_ocr_amd.detectors import EAST
    from manuscript_ocr_amd.recognizers import TRBA, EditCosts
    H, W = 512, 768
    det = EAST(state_dict=synth.east_state_dict(), target_size=(W, H), device="cuda")
    rec = TRBA(state_dict=synth.trba_state_dict(194, 256, seed=20260128), config={"img_h": 32, "img_w": 100, "max_len": 25, "hidden_size": 256},
               device="cuda")
    rng = np.random.default_rng(5)
    V = len(rec.itos)
    sub = rng.integers(1, 41, (V, V))
    np.fill_diagonal(sub, 0)
    costs = EditCosts(sub, rng.integers(8, 41, V), rng.integers(1, 41, V), rec.stoi)   # deletes of 8 and more keep every window short
    pipe = Pipeline(detector=det, recognizer=rec)
    img = synth.synth_page(5, H, W)[0]
    page = pipe.predict(img)
    words = [word.text for block in page.blocks for word in block.words if word.text]
    assert len(words) >= 2
    queries = sorted({t for t in words if len(t) <= 64 and t == "".join(t.split())})
    assert queries
    on_dev = pipe.search([img, page], queries, max_distance=0, device=rec.device, costs=costs)
    assert on_dev == pipe.search([page, page], queries, max_distance=0, costs=costs)
    assert all(any(h.query == q and h.distance == 0 and h.matched_text == t for h in on_dev) for q, t in enumerate(queries))
    near = dict(max_error_rate=0.3, overlapping=True, costs=costs)
    got = PageCorpus([page], device=rec.device).search(queries, **near)
    assert got == PageCorpus([page]).search(queries, **near) and len(got) >= len(queries)
