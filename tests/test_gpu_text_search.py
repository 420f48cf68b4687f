"""msocr_text_search on the MI355X against its host twin msocr_text_search_host, which
tests/test_text_search_cpu.py holds to the plain Sellers table.  Hits are integers: every comparison is equality, after
text_search_select or a canonical sort (the device writes its hits in no particular order).

Sizes follow L = MSOCR_SEARCH_SEGMENT, the tokens one lane of the scan kernel reports: text lengths around one, two and three
segments, patterns planted around the first cut and around the first token after the warm-up of m + k tokens, texts whose neighbours
hold the rest of the pattern, more segments than a workgroup has lanes, every lane of every wave appending at once, and capacities
below the count.  A last group enters what those sizes leave out: token arrays off the 16-byte boundary, first offsets above 0,
and tables, records and patterns beyond one trip of a capped grid."""
import numpy as np
import pytest

from test_text_search_cpu import canonical, csr, host

pytestmark = pytest.mark.gpu


def seg():
    from manuscript_ocr_amd import ops
    return ops.SEARCH_SEGMENT


def device(patterns, ks, texts, v, capacity=None):
    """ops.text_search (both passes of its overflow protocol if need be) -> hits [count, 5] as the device wrote them"""
    import torch
    from manuscript_ocr_amd import ops
    pat_tok, pat_off = csr(patterns)
    txt_tok, txt_off = csr(texts)
    kw = {} if capacity is None else {"capacity": capacity}
    return ops.text_search(torch.from_numpy(pat_tok).cuda(), pat_off, ks, torch.from_numpy(txt_tok).cuda(), txt_off, v, **kw)


def same_as_host(patterns, ks, texts, v):
    from manuscript_ocr_amd import ops
    want, count = host(patterns, ks, texts, v)
    got = device(patterns, ks, texts, v)
    assert len(got) == count
    assert np.array_equal(canonical(got), want)
    assert np.array_equal(ops.text_search_select(got), ops.text_search_select(want))
    return want


def device_views(pat_tok, pat_off, ks, txt_tok, txt_off, v, shift=0):
    """ops.text_search on token arrays that lie `shift` elements behind the start of a fresh allocation, as the views buf[shift:]:
    the array's memory then begins 4 * shift bytes behind a 16-byte boundary, which the view's address must show"""
    import torch
    from manuscript_ocr_amd import ops
    views = []
    for tok in (pat_tok, txt_tok):
        buf = torch.full((shift + len(tok),), -3, dtype=torch.int32, device="cuda")
        buf[shift:] = torch.from_numpy(np.ascontiguousarray(tok, dtype=np.int32)).cuda()
        views.append(buf[shift:])
        assert views[-1].data_ptr() % 16 == 4 * shift and views[-1].is_contiguous()
    return ops.text_search(views[0], pat_off, ks, views[1], txt_off, v)


def cut_texts(m):
    """one pattern of m tokens under three bounds, and texts with its copies planted around the segment cuts
    -> (a, ks, v, texts, planted_at)"""
    L = seg()
    rng = np.random.default_rng(300 + m)
    v = 60
    a = rng.integers(0, v, m).astype(np.int32)
    ks = [0, 2, m - 1]
    texts = [rng.integers(0, v, n).astype(np.int32) for n in (L - 1, L, L + 1, 2 * L - 1, 2 * L + 1, 3 * L + 7)]
    planted_at = []
    for k in ks:
        W = m + k
        cut = -(-W // L) * L                       # the first cut with room for m + k tokens before it
        for end in (L - 1, L, L + 1, L + W, cut - W + m, cut + m):   # the last two: a start exactly m + k before a cut, and at it
            if end - m < 0:
                continue
            b = rng.integers(0, v, max(3 * L + 7, end + 3)).astype(np.int32)
            b[end - m:end] = a
            texts.append(b)
            planted_at.append((len(texts) - 1, end))
            noisy = b.copy()                        # the same copy with one substitution and one token dropped in front of it
            noisy[end - 1 - m // 2] = v + 3
            texts.append(np.delete(noisy, max(end - m - 1, 0)))
    return a, ks, v, texts, planted_at


@pytest.mark.parametrize("m", [5, 63, 64])
def test_cuts_and_the_first_token_after_the_warm_up(m):
    a, ks, v, texts, planted_at = cut_texts(m)
    want = same_as_host([a, a, a], ks, texts, v)
    exact = {(h[1], h[3]) for h in want.tolist() if h[0] == 0}
    assert all(p in exact for p in planted_at)
    assert len(want[want[:, 0] == 2]) > len(want[want[:, 0] == 1]) > len(exact)  # the wider the bound, the more ends


def test_ragged_batch_text_boundaries():
    """about 40 texts with empty ones between them.  A warm-up must stop at its text's own start: one text is the pattern's own
    prefix, and texts end with the first half of the pattern where the next begins with the second half."""
    L = seg()
    rng = np.random.default_rng(71)
    v = 30
    a = rng.integers(0, v, 12).astype(np.int32)
    c = rng.integers(0, v, 64).astype(np.int32)
    texts = []
    for n in rng.integers(0, 3 * L, 26).tolist():
        texts.append(rng.integers(0, v, n).astype(np.int32))
        if len(texts) % 4 == 0:
            texts.append(np.zeros(0, dtype=np.int32))
    texts += [a[:11], a[:6], a[6:], np.zeros(0, dtype=np.int32), a[:6], np.zeros(0, dtype=np.int32), a[6:], a, c[:40], c[40:], c,
              np.concatenate([rng.integers(0, v, L - 6).astype(np.int32), a[:6]]), np.concatenate([a[6:], rng.integers(0, v, L).astype(np.int32)])]
    texts = [np.zeros(0, dtype=np.int32)] + texts + [np.zeros(0, dtype=np.int32)]
    assert 38 <= len(texts) <= 50
    want = same_as_host([a, c, a], [1, 5, 0], texts, v)
    whole = [t for t, b in enumerate(texts) if len(b) == 12 and np.array_equal(b, a)]
    assert [h[1] for h in want.tolist() if h[0] == 2] == whole and len(whole) == 1  # exact hits of `a`: the one text that is `a`
    assert len(want[want[:, 0] == 0]) >= 3  # the 11-token prefix is within one edit


@pytest.mark.parametrize("Q", [1, 2, 65])
def test_more_segments_than_a_workgroup_has_lanes(Q):
    L = seg()
    rng = np.random.default_rng(80 + Q)
    v = 4
    text = rng.integers(0, v, 256 * L + 1).astype(np.int32)
    patterns = [rng.integers(0, v, int(m)).astype(np.int32) for m in rng.integers(6, 12, Q)]
    patterns[0] = text[-7:].copy()            # the last pattern token is the text's last token, alone in its segment
    ks = [2] * Q
    want = same_as_host(patterns, ks, [text, text[:L + 3]], v)
    assert [0, 0, 256 * L - 6, 256 * L + 1, 0] in want.tolist() and len(want) >= 100 * Q


def test_dense_hits_every_lane_appends():
    """the one-symbol text of 4 L tokens: every position from m - k on is a hit, so every lane of every wave appends at every step"""
    L = seg()
    n = 4 * L
    zeros = lambda k: np.zeros(k, dtype=np.int32)  # noqa: E731
    shapes = [(1, 0), (5, 2), (64, 63), (64, 0), (33, 7)]
    want = same_as_host([zeros(m) for m, _ in shapes], [k for _, k in shapes], [zeros(n), zeros(0), zeros(n), zeros(L + 1)], 1)
    assert len(want) == sum(max(0, length - max(m - k, 1) + 1) for m, k in shapes for length in (n, n, L + 1))


def test_overflow_exact_count_true_distinct_records_and_the_guard():
    import torch
    from manuscript_ocr_amd import ops
    L = seg()
    rng = np.random.default_rng(91)
    v = 3
    patterns = [rng.integers(0, v, m).astype(np.int32) for m in (4, 9, 30)]
    ks = [1, 3, 12]
    texts = [rng.integers(0, v, n).astype(np.int32) for n in (3 * L + 7, 0, 5 * L)]
    full, count = host(patterns, ks, texts, v)
    members = set(map(tuple, full.tolist()))
    assert count == len(members) > 300
    pat_tok, pat_off = csr(patterns)
    txt_tok, txt_off = csr(texts)
    pd, td = torch.from_numpy(pat_tok).cuda(), torch.from_numpy(txt_tok).cuda()
    for cap in (0, 1, count - 1, count, count + 9):
        buf = torch.full((cap + 16, 5), -7, dtype=torch.int32, device="cuda")
        cnt = torch.full((1,), -7, dtype=torch.int64, device="cuda")
        ops.text_search_into(pd, pat_off, ks, td, txt_off, v, buf[:cap], cnt)
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert int(cnt.item()) == count, cap
        written = min(cap, count)
        rows = list(map(tuple, got[:written].tolist()))
        assert all(r in members for r in rows) and len(set(rows)) == written, cap   # true hits, all distinct
        assert (got[written:] == -7).all(), cap                                        # the guard behind hits_out[capacity]
    # the two-pass protocol of ops.text_search: complete whatever the first capacity was
    for cap in (0, 1, count - 1, count):
        assert np.array_equal(canonical(device(patterns, ks, texts, v, capacity=cap)), full), cap
    # the workspace: exactly the stated size is handed over, the rest is a guard
    need = ops.text_search_workspace_bytes(pat_off, ks, txt_off, v)
    ws = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    buf = torch.empty((count, 5), dtype=torch.int32, device="cuda")
    cnt = torch.zeros((1,), dtype=torch.int64, device="cuda")
    ops.text_search_into(pd, pat_off, ks, td, txt_off, v, buf, cnt, workspace=ws[:need])
    torch.cuda.synchronize()
    assert np.array_equal(canonical(buf.cpu().numpy()), full) and bool((ws[need:] == 0xA5).all())


def test_alphabets_of_one_and_of_the_cap_and_foreign_tokens():
    from manuscript_ocr_amd import ops
    L = seg()
    rng = np.random.default_rng(101)
    # v = 1: one table row; 0 matches, every other token equals nothing
    mixed = (rng.random(3 * L + 7) < 0.2).astype(np.int32)
    same_as_host([np.zeros(3, dtype=np.int32), np.array([0, 1, 0], dtype=np.int32)], [1, 2], [mixed, np.zeros(L, dtype=np.int32)], 1)
    # v = 2048 with 2048 distinct text symbols: the whole LDS row is loaded and read
    V = ops.SEARCH_MAX_ALPHABET
    text = rng.permutation(V).astype(np.int32)
    patterns = [text[100:164].copy(), text[V - 5:].copy(), np.array([V - 1, V - 2, 0, 1], dtype=np.int32), text[L - 3:L + 4].copy()]
    patterns[0][10] = V          # foreign tokens in the pattern
    patterns[0][20] = -1
    want = same_as_host(patterns, [2, 0, 1, 0], [text, text[::-1].copy(), text[:L]], V)
    assert [0, 0, 100, 164, 2] in want.tolist() and [1, 0, V - 5, V, 0] in want.tolist() and [3, 0, L - 3, L + 4, 0] in want.tolist()
    # foreign tokens on both sides, garbage included
    big = 2**31 - 1
    wild = np.array([-1, 6, big, -2**31, 1, 2, 3], dtype=np.int32)
    patterns = [wild[rng.integers(0, 7, m)] for m in (4, 33, 64)]
    texts = [wild[rng.integers(0, 7, n)] for n in (0, L + 6, 5 * L)]
    same_as_host(patterns, [2, 20, 50], texts, 6)


# ------------------------------------------------------------------------------------------------ launch geometry and views
# The tests above hand over fresh allocations with offsets from 0 and stay below every cap of a grid.  The ones below enter the
# code that runs otherwise: each names the loop or branch it is the first to enter and asserts the geometry it is there for.
ZERO_CAP = 4096 * 256      # workgroups x words of one trip of ts_zero_kernel, and workgroups x records of one of ts_start_kernel
SCAN_ROWS = 65535          # gridDim.y of ts_scan_kernel at most


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_token_arrays_off_the_16_byte_boundary(shift):
    """The first test in which `align` of ts_scan_kernel is not 0: both token arrays are the views buf[shift:] of a fresh
    allocation, so the 16-byte loads of ts_load4 start `shift` elements off the array's own index and both ends of the array go
    through its element-wise arm.  The texts of the cut test for m = 5, between texts of L - 1, L and L + 1 tokens whose first and
    whose last m tokens are the pattern: the first and the last token of the array end and begin a hit."""
    L = seg()
    a, ks, v, texts, planted_at = cut_texts(5)
    rng = np.random.default_rng(310 + shift)
    ends = []
    for n in (L - 1, L, L + 1):
        b = rng.integers(0, v, n).astype(np.int32)
        b[:5], b[-5:] = a, a
        ends.append(b)
    texts = ends[:2] + texts + ends[2:]
    patterns = [a, a, a]
    want, count = host(patterns, ks, texts, v)
    pat_tok, pat_off = csr(patterns)
    txt_tok, txt_off = csr(texts)
    plain = device_views(pat_tok, pat_off, ks, txt_tok, txt_off, v, 0)
    got = device_views(pat_tok, pat_off, ks, txt_tok, txt_off, v, shift)
    assert len(got) == count == len(plain)
    assert np.array_equal(canonical(got), canonical(plain)) and np.array_equal(canonical(got), want)
    exact = {(h[1], h[3]) for h in want.tolist() if h[0] == 0}
    assert all((t + 2, end) in exact for t, end in planted_at)
    last = len(texts) - 1
    assert {(0, 5), (0, L - 1), (1, 5), (1, L), (last, 5), (last, L + 1)} <= exact


@pytest.mark.parametrize("shift", [0, 1])
def test_first_offsets_above_zero(shift):
    """The first test on the device with txt_off[0] > 0 and pat_off[0] > 0 (glo > 0 in ts_scan_kernel, a0 > 0 for pattern 0 in
    ts_masks_kernel): the token arrays carry junk before the first offset and behind the last.  The junk before txt_off[0] ends
    with the first half of a pattern whose second half opens text 0, the junk behind txt_off[T] completes a pattern that the last
    text begins, and the junk around the patterns would complete a third: a read across either edge makes a hit the host twin, given
    the same arrays and offsets, does not have.  Once aligned, once with both arrays one element off the 16-byte boundary."""
    from manuscript_ocr_amd import ops
    L = seg()
    rng = np.random.default_rng(320)
    v = 30
    a = rng.integers(0, v, 12).astype(np.int32)
    c = rng.integers(0, v, 9).astype(np.int32)
    rnd = lambda n: rng.integers(0, v, n).astype(np.int32)  # noqa: E731
    texts = [np.concatenate([a[6:], rnd(L + 2), a, rnd(5)]), np.zeros(0, dtype=np.int32), rnd(2 * L - 1), np.concatenate([rnd(L - 3), a, a[:6]])]
    patterns, ks = [a, a, c[3:6], a[:7]], [0, 2, 0, 1]
    clean, count = host(patterns, ks, texts, v)
    txt_tok, txt_off = csr(texts)
    pat_tok, pat_off = csr(patterns)
    before_t, after_t = np.concatenate([rnd(7), a[:6]]), np.concatenate([a[6:], rnd(6)])    # 13 tokens: text 0 starts off the boundary
    before_p, after_p = c[:3], c[6:]                                                       # c[3:6] is a pattern: c would be one too
    txt_tok, txt_off = np.concatenate([before_t, txt_tok, after_t]), txt_off + len(before_t)
    pat_tok, pat_off = np.concatenate([before_p, pat_tok, after_p]), pat_off + len(before_p)
    assert txt_off[0] == 13 and txt_off[-1] == len(txt_tok) - 12 and pat_off[0] == 3 and pat_off[-1] == len(pat_tok) - 3
    want, n = ops.text_search_host(pat_tok, pat_off, ks, txt_tok, txt_off, v)
    assert n == count and np.array_equal(want, clean)       # the host twin reads nothing outside the offsets
    got = device_views(pat_tok, pat_off, ks, txt_tok, txt_off, v, shift)
    assert len(got) == count
    assert np.array_equal(canonical(got), want)
    assert np.array_equal(ops.text_search_select(got), ops.text_search_select(want))
    exact = [h for h in want.tolist() if h[0] == 0]
    assert [(h[1], h[2], h[3]) for h in exact] == [(0, 6 + L + 2, 6 + L + 2 + 12), (3, L - 3, L + 9)]  # the two whole copies, no half


def test_mask_tables_beyond_one_trip_of_the_zero_kernel():
    """The first test in which ts_zero_kernel takes a second trip of its grid-stride loop: 257 patterns over v = 2048 are
    257 * 2 * 2048 table words, above the 4096 workgroups x 256 words of one trip.  The workspace holds 0xA5 everywhere, so a word
    that is not cleared matches at garbage positions; the words of the second trip are the rows of the last pattern, which has
    known hits, and a text over all 2048 symbols reads every row's every word."""
    import torch
    from manuscript_ocr_amd import ops
    Q, V = 257, ops.SEARCH_MAX_ALPHABET
    words = Q * 2 * V
    assert words == 1052672 and words > ZERO_CAP and (Q - 1) * 2 * V >= ZERO_CAP   # pattern 256's rows lie in the second trip
    rng = np.random.default_rng(330)
    text = rng.permutation(V).astype(np.int32)
    at = rng.integers(0, V - 8, Q)
    patterns = [text[int(s):int(s) + 4 + q % 5].copy() for q, s in enumerate(at)]
    patterns[Q - 1] = text[V - 5:].copy()
    ks = [q % 2 for q in range(Q)]
    texts = [text, text[::-1].copy(), text[:100]]
    want, count = host(patterns, ks, texts, V)
    pat_tok, pat_off = csr(patterns)
    txt_tok, txt_off = csr(texts)
    need = ops.text_search_workspace_bytes(pat_off, ks, txt_off, V)
    assert need >= 8 * words
    ws = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    buf = torch.full((count + 16, 5), -7, dtype=torch.int32, device="cuda")
    cnt = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    ops.text_search_into(torch.from_numpy(pat_tok).cuda(), pat_off, ks, torch.from_numpy(txt_tok).cuda(), txt_off, V, buf[:count], cnt,
                         workspace=ws[:need])
    torch.cuda.synchronize()
    assert int(cnt.item()) == count
    assert np.array_equal(canonical(buf[:count].cpu().numpy()), want)
    assert bool((buf[count:] == -7).all()) and bool((ws[need:] == 0xA5).all())
    assert [Q - 1, 0, V - 5, V, 0] in want.tolist() and len(want[want[:, 0] == Q - 1]) >= 1


def test_more_records_than_one_trip_of_the_start_kernel():
    """The first test in which ts_start_kernel takes a second trip of its grid-stride loop: the one-symbol text of 2^20 + 300 tokens
    holds the pattern [0] at every position, more records than 4096 workgroups x 256 lanes.  Every record must be a true hit with
    its start, end = 1 .. n each exactly once, and the guard rows behind hits[capacity] stay as they were."""
    import torch
    from manuscript_ocr_amd import ops
    n = (1 << 20) + 300
    patterns, ks, texts = [np.zeros(1, dtype=np.int32)], [0], [np.zeros(n, dtype=np.int32)]
    count = host(patterns, ks, texts, 1, capacity=0)[1]
    assert count == n and count > ZERO_CAP
    pat_tok, pat_off = csr(patterns)
    txt_tok, txt_off = csr(texts)
    buf = torch.full((count + 16, 5), -7, dtype=torch.int32, device="cuda")
    cnt = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    ops.text_search_into(torch.from_numpy(pat_tok).cuda(), pat_off, ks, torch.from_numpy(txt_tok).cuda(), txt_off, 1, buf[:count], cnt)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert int(cnt.item()) == count
    rows = got[:count]
    assert not rows[:, 0].any() and not rows[:, 1].any() and not rows[:, 4].any()        # pattern 0 in text 0 at distance 0
    assert np.array_equal(rows[:, 2], rows[:, 3] - 1)                                      # start == end - 1 throughout
    assert np.array_equal(np.sort(rows[:, 3]), np.arange(1, n + 1, dtype=np.int32))        # every end once: true hits, all distinct
    assert (got[count:] == -7).all()


def test_more_patterns_than_grid_rows():
    """The first test in which a workgroup of ts_scan_kernel handles a second pattern (q += gridDim.y): 65 539 patterns against a
    grid of at most 65 535 rows.  The workgroup then loads another mask row over the one in LDS, between the two barriers at the
    loop's head.  The four patterns of the second trip are copies of text[10:12] and of the two tokens around the cut at L of
    both texts."""
    L = seg()
    Q = 65539
    assert Q > SCAN_ROWS
    rng = np.random.default_rng(340)
    v = 16
    texts = [rng.integers(0, v, L + 6).astype(np.int32), rng.integers(0, v, L + 9).astype(np.int32)]
    two = rng.integers(0, v, (Q, 2)).astype(np.int32)
    patterns = list(two)
    ks = [0] * Q
    for q in (7, 30000, SCAN_ROWS - 1):                       # a few of three tokens within one error
        patterns[q], ks[q] = rng.integers(0, v, 3).astype(np.int32), 1
    known = []
    for j, (t, s) in enumerate(((0, 10), (0, L - 1), (1, 10), (1, L - 1))):
        patterns[SCAN_ROWS + j] = texts[t][s:s + 2].copy()
        known.append([SCAN_ROWS + j, t, s, s + 2, 0])
    assert SCAN_ROWS + 3 == Q - 1
    want = same_as_host(patterns, ks, texts, v)
    rows = want.tolist()
    assert all(h in rows for h in known)
    assert 10000 <= len(want) <= 60000
    assert (want[:, 0] >= SCAN_ROWS).sum() >= 4 and len(np.unique(want[:, 0])) > 10000


def test_no_patterns_no_texts_and_empty_texts_only():
    import torch
    from manuscript_ocr_amd import ops
    none = torch.zeros(0, dtype=torch.int32, device="cuda")
    some = torch.zeros(9, dtype=torch.int32, device="cuda")
    assert ops.text_search(none, [0], [], some, [0, 9], 4).shape == (0, 5)
    assert ops.text_search(some, [0, 9], [2], none, [0], 4).shape == (0, 5)
    assert ops.text_search(some, [0, 9], [2], none, [0, 0, 0], 4).shape == (0, 5)
    cnt = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    ops.text_search_into(none, [0], [], some, [0, 9], 4, torch.empty((0, 5), dtype=torch.int32, device="cuda"), cnt)
    assert int(cnt.item()) == 0


def test_text_corpus_resident_on_the_device():
    from manuscript_ocr_amd.recognizers import TextCorpus, search_texts
    rng = np.random.default_rng(111)
    letters = np.array(list("abcdefghijklmnopqrstuvwxyz "))
    texts = ["".join(letters[rng.integers(0, 27, int(n))]) for n in rng.integers(0, 700, 24)] + ["", "needle in a haystack"]
    first = [texts[3][40:52], texts[5][10:18], "needle", "haystick", "zzzzzq"]
    second = [texts[7][5:30], "in a", "e"]
    corpus = TextCorpus(texts, device="cuda")
    for queries, bound in ((first, dict(max_distance=1)), (second, dict(max_error_rate=0.25)), (first, dict(max_error_rate=0.2, overlapping=True))):
        got = corpus.search(queries, **bound)
        assert got == search_texts(queries, texts, device="cuda", **bound)   # the same hits as a one-shot call
        assert got == search_texts(queries, texts, **bound) and len(got) > 0  # the device route equals the host route
    assert any(h.pattern == 3 and h.distance == 1 and texts[h.text][h.start:h.end] == "haystack" for h in corpus.search(first, max_distance=1))


def test_pipeline_search_with_the_package_plugins():
    """Pipeline.search with this package's detector and recogniser on a synthetic page, queries taken from the decode's own texts:
    every word that is a query is found at distance 0 and mapped back to itself, and the device route equals the host route."""
    from manuscript_ocr_amd import PageCorpus, Pipeline, synth
    from manuscript_ocr_amd.detectors import EAST
    from manuscript_ocr_amd.recognizers import TRBA
    H, W = 512, 768
    det = EAST(state_dict=synth.east_state_dict(), target_size=(W, H), device="cuda")
    rec = TRBA(state_dict=synth.trba_state_dict(194, 256, seed=20260128), config={"img_h": 32, "img_w": 100, "max_len": 25, "hidden_size": 256},
               device="cuda")
    pipe = Pipeline(detector=det, recognizer=rec)
    img = synth.synth_page(5, H, W)[0]
    page = pipe.predict(img)
    words = [(b, w, word.text) for b, block in enumerate(page.blocks) for w, word in enumerate(block.words) if word.text]
    assert len(words) >= 2
    queries = sorted({t for _b, _w, t in words if len(t) <= 64 and t == "".join(t.split())})  # a query is whitespace-normalised
    assert queries
    on_dev = pipe.search([img, page], queries, max_distance=0, device=rec.device)
    on_host = pipe.search([page, page], queries, max_distance=0)
    assert on_dev == on_host
    for b, w, t in words:
        if t in queries:
            for p in (0, 1):
                assert any(h.page == p and h.query == queries.index(t) and h.distance == 0 and h.matched_text == t and h.words == [(b, w)]
                           for h in on_dev), (p, b, w, t)
    near = dict(max_error_rate=0.34, overlapping=True)
    assert PageCorpus([page], device=rec.device).search(queries, **near) == PageCorpus([page]).search(queries, **near)
