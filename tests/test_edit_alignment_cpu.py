"""The alignment behind the error rates, host side: csrc/edit_alignment.h through the host twin
msocr_edit_alignment_host against a full-table NumPy programme that applies the four rules literally, the invariants of every
alignment (also at the cap), by-hand cases, the C ABI's refusals, recognizers.sequence_alignments / error_breakdown /
text_error_rates(breakdown=True), Pipeline.evaluate_text(breakdown=True) and Pipeline.transfer_text on stand-in plugins, and the
header in a C++ program of its own under the address and undefined-behaviour sanitizers (tests/native/edit_alignment_fuzz.cpp).
No GPU.

Every comparison is integer equality.  tests/test_gpu_edit_alignment.py imports the helpers of this file."""
import os
import subprocess
from collections import Counter

import numpy as np
import pytest

from test_edit_distance_long_cpu import CAP, OTHER_LENS, PATTERN_LENS, csr, random_pair, structured_pairs

E_ARG = -1


def _lib():
    from manuscript_ocr_amd import _native as nat
    return nat.lib()


def full_table(a, b, v):
    """D [m + 1][n + 1] of the textbook programme, one NumPy row per token of the shorter side (the matching rule is symmetric, so
    the table of (b, a) is the transpose).  A token outside [0, v) equals nothing."""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    if len(a) > len(b):
        return np.ascontiguousarray(full_table(b, a, v).T)
    n = len(b)
    ar = np.arange(n + 1)
    D = np.empty((len(a) + 1, n + 1), dtype=np.int64)
    D[0] = ar
    for i, x in enumerate(a.tolist()):
        cur = np.empty(n + 1, dtype=np.int64)
        cur[0] = i + 1
        ne = (b != x).astype(np.int64) if 0 <= x < v else 1
        cur[1:] = np.minimum(D[i, 1:] + 1, D[i, :-1] + ne)
        D[i + 1] = np.minimum.accumulate(cur - ar) + ar
    return D


def ref_alignment(a, b, v):
    """rules 1-4 of include/msocr.h on the full table -> (dist, a_map, b_map, [hits, substitutions, deletions, insertions])"""
    D = full_table(a, b, v)
    a, b = [int(x) for x in a], [int(x) for x in b]
    i, j = len(a), len(b)
    a_map, b_map, cnt = [-1] * i, [-1] * j, [0, 0, 0, 0]
    while i > 0 and j > 0:
        if a[i - 1] == b[j - 1] and 0 <= a[i - 1] < v:
            op = 0
        elif D[i - 1, j - 1] + 1 == D[i, j]:
            op = 1
        elif D[i - 1, j] + 1 == D[i, j]:
            op = 2
        else:
            op = 3
        cnt[op] += 1
        if op < 2:
            a_map[i - 1], b_map[j - 1] = j - 1, i - 1
            i, j = i - 1, j - 1
        elif op == 2:
            i -= 1
        else:
            j -= 1
    cnt[2] += i
    cnt[3] += j
    return int(D[len(a), len(b)]), a_map, b_map, cnt


def split(pairs, out):
    """the four arrays of a call -> per pair (dist, a_map, b_map, counts) as plain lists"""
    dist, a_map, b_map, counts = (np.asarray(x) for x in out)
    res, ia, ib = [], 0, 0
    for p, (a, b, _v) in enumerate(pairs):
        res.append((int(dist[p]), a_map[ia:ia + len(a)].tolist(), b_map[ib:ib + len(b)].tolist(), counts[p].tolist()))
        ia, ib = ia + len(a), ib + len(b)
    assert ia == len(a_map) and ib == len(b_map)
    return res


def host(pairs):
    """pairs: (a, b, v) -> the host twin's alignments, per pair"""
    from manuscript_ocr_amd import ops
    a_tok, a_off = csr([p[0] for p in pairs])
    b_tok, b_off = csr([p[1] for p in pairs])
    return split(pairs, ops.edit_alignment_host(a_tok, a_off, b_tok, b_off, [p[2] for p in pairs]))


def check_invariants(pair, got, want_dist=None):
    a, b, v = pair
    dist, a_map, b_map, (hits, subs, dels, inss) = got
    a_map, b_map = np.asarray(a_map, dtype=np.int64), np.asarray(b_map, dtype=np.int64)
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    assert subs + dels + inss == dist and (want_dist is None or dist == want_dist)
    assert hits + subs + dels == len(a) and hits + subs + inss == len(b)
    ia, ib = np.flatnonzero(a_map >= 0), np.flatnonzero(b_map >= 0)
    assert len(ia) == len(ib) == hits + subs and int((a_map < -1).sum()) == 0 and int((b_map < -1).sum()) == 0
    assert np.array_equal(b_map[a_map[ia]], ia) and np.array_equal(a_map[b_map[ib]], ib)   # mutually inverse
    assert np.all(np.diff(a_map[ia]) > 0) and np.all(np.diff(b_map[ib]) > 0)               # strictly increasing
    pa, pb = a[ia], b[a_map[ia]]
    assert int(((pa == pb) & (pa >= 0) & (pa < v)).sum()) == hits                            # paired equal tokens = hits


def host_distances(pairs):
    from manuscript_ocr_amd import ops
    a_tok, a_off = csr([p[0] for p in pairs])
    b_tok, b_off = csr([p[1] for p in pairs])
    return ops.edit_distance_long_host(a_tok, a_off, b_tok, b_off, [p[2] for p in pairs]).tolist()


def edited_copy(rng, a, v, n):
    """a text of n tokens that follows a: a's tokens (cycled) with a tenth replaced, some by tokens outside [0, v)"""
    b = np.resize(a, n).astype(np.int32) if len(a) and n else rng.integers(0, v + 2, n).astype(np.int32)
    hit = rng.random(n) < 0.1
    b[hit] = rng.integers(-1, v + 2, int(hit.sum()))
    return b


def check_against_the_table(pairs):
    got = host(pairs)
    dist = host_distances(pairs)
    for pair, g, d in zip(pairs, got, dist):
        want = ref_alignment(*pair)
        assert g[0] == want[0] and g[3] == want[3], (len(pair[0]), len(pair[1]), pair[2], g[0], want[0], g[3], want[3])
        assert g[1] == want[1] and g[2] == want[2], (len(pair[0]), len(pair[1]), pair[2])
        check_invariants(pair, g, d)


@pytest.mark.parametrize("v", [2, 4, 30, 1000])
def test_host_twin_against_the_full_table(v):
    rng = np.random.default_rng(200 + v)
    pairs = [random_pair(rng, m, n, v) for m in PATTERN_LENS for n in OTHER_LENS]
    check_against_the_table(pairs)


@pytest.mark.parametrize("v", [2, 4, 30, 1000])
def test_host_twin_on_edited_copies(v):
    rng = np.random.default_rng(300 + v)
    pairs = []
    for m in PATTERN_LENS:
        for n in OTHER_LENS:
            a = rng.integers(0, v, m).astype(np.int32)
            a[rng.random(m) < 0.02] = v + 1  # pattern tokens outside [0, v) too
            pairs.append((a, edited_copy(rng, a, v, n), v))
    check_against_the_table(pairs)


def test_structured_sequences_garbage_tokens_and_an_empty_alphabet():
    pairs = structured_pairs()
    check_against_the_table(pairs)
    got = host(pairs)
    assert got[0][3] == [1000, 0, 0, 0] and got[0][1] == list(range(1000))     # equal: all hits
    assert got[2][3] == [0, 1000, 0, 0]                                       # disjoint alphabets, equal lengths: all substitutions
    assert got[10][3] == [0, 70, 60, 0]                                       # v = 0: nothing matches
    rng = np.random.default_rng(9)
    wild = np.array([-1, 2**31 - 1, -2**31, 40, 5, 5, 77], dtype=np.int32)
    check_against_the_table([(rng.permutation(np.tile(wild, 30)), rng.permutation(np.tile(wild, 25)), v) for v in (0, 6, 50, 100)])


def test_one_pair_at_the_cap_holds_the_invariants():
    rng = np.random.default_rng(11)
    a = rng.integers(0, 4, CAP).astype(np.int32)
    b = a.copy()
    b[rng.integers(0, CAP, 3000)] = rng.integers(0, 5, 3000)
    b = np.roll(b, 7)
    pair = (a, b, 4)
    check_invariants(pair, host([pair])[0], host_distances([pair])[0])


def test_by_hand():
    i32 = lambda *x: np.array(x, dtype=np.int32)  # noqa: E731
    assert host([(i32(0, 1), i32(1, 0), 2)])[0] == (2, [0, 1], [0, 1], [0, 2, 0, 0])   # "ab" against "ba": two substitutions under this rule
    seq = np.arange(500, dtype=np.int32)
    cut = np.concatenate([seq[:100], seq[300:]])                  # a chunk of 200 removed from the text: all deletions
    foreign = np.concatenate([seq[:100], np.full(200, 999, dtype=np.int32), seq[100:]])  # 200 tokens put in: all insertions
    (d0, am0, bm0, c0), (d1, am1, bm1, c1), (d2, am2, bm2, c2) = host([(seq, cut, 500), (seq, foreign, 500), (seq, seq.copy(), 500)])
    assert (d0, c0) == (200, [300, 0, 200, 0]) and sum(1 for x in am0 if x < 0) == 200 and all(x >= 0 for x in bm0)
    assert am0[:100] == list(range(100)) and am0[300:] == list(range(100, 300))
    assert (d1, c1) == (200, [500, 0, 0, 200]) and bm1[100:300] == [-1] * 200 and all(x >= 0 for x in am1)
    assert (d2, c2) == (0, [500, 0, 0, 0]) and am2 == bm2 == list(range(500))
    # empty sides
    assert host([(i32(), i32(3, 3, 3), 5), (i32(1, 2), i32(), 5), (i32(), i32(), 5)]) == [
        (3, [], [-1, -1, -1], [0, 0, 0, 3]), (2, [-1, -1], [], [0, 0, 2, 0]), (0, [], [], [0, 0, 0, 0])]


def test_offsets_that_do_not_start_at_zero():
    """the maps start at the first pair's tokens: a_map_out [a_off[N] - a_off[0]]"""
    from manuscript_ocr_amd import ops
    rng = np.random.default_rng(17)
    pairs = [random_pair(rng, m, n, 6) for m, n in ((70, 90), (0, 4), (130, 64))]
    a_tok, a_off = csr([p[0] for p in pairs])
    b_tok, b_off = csr([p[1] for p in pairs])
    v = [p[2] for p in pairs]
    want = ops.edit_alignment_host(a_tok, a_off, b_tok, b_off, v)
    got = ops.edit_alignment_host(np.concatenate([[7] * 5, a_tok]), a_off + 5, np.concatenate([[7] * 3, b_tok]), b_off + 3, v)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


def test_symbols_and_wrappers_are_exported():
    from manuscript_ocr_amd import _native as nat
    from manuscript_ocr_amd import ops
    for name in ("msocr_edit_alignment_ws_bytes", "msocr_edit_alignment", "msocr_edit_alignment_host"):
        assert name in nat.exported_symbols() and hasattr(_lib(), name)
    assert callable(ops.edit_alignment) and callable(ops.edit_alignment_host) and callable(ops.edit_alignment_workspace_bytes)


def test_abi_refusals():
    """Everything here is refused (or is N == 0) before any launch: no GPU is touched."""
    L = _lib()
    i32 = lambda *x: np.array(x, dtype=np.int32)  # noqa: E731
    tok = np.zeros(CAP + 8, dtype=np.int32)
    outs = [np.full(4, -7, dtype=np.int32), np.full(400, -7, dtype=np.int32), np.full(400, -7, dtype=np.int32), np.full(12, -7, dtype=np.int32)]
    optr = [o.ctypes.data for o in outs]
    good = (i32(0, 100, 300), i32(0, 64, 64), i32(5, 9))

    def ws(a_off, b_off, v, N=None):
        return L.msocr_edit_alignment_ws_bytes(a_off.ctypes.data, b_off.ctypes.data, v.ctypes.data, len(v) if N is None else N)

    def run_host(a_off, b_off, v, N=None, ptr=optr):
        return L.msocr_edit_alignment_host(tok.ctypes.data, a_off.ctypes.data, tok.ctypes.data, b_off.ctypes.data, v.ctypes.data,
                                           len(v) if N is None else N, *ptr)

    def run_dev(a_off, b_off, v, ws_ptr, ws_bytes, N=None, ptr=optr, a=tok.ctypes.data):  # `tok` stands in for device memory
        return L.msocr_edit_alignment(a, a_off.ctypes.data, tok.ctypes.data, b_off.ctypes.data, v.ctypes.data,
                                      len(v) if N is None else N, *ptr, ws_ptr, ws_bytes, None)

    # the workspace formula of include/msocr.h: 40 N + sum v ceil(m / 64) 8, to a multiple of 16, + sum 16 ceil(m / 64) n
    assert ws(*good) == 40 * 2 + (5 * 2 + 9 * 4) * 8 + 16 * (2 * 64 + 4 * 0)
    assert ws(i32(0, 65), i32(0, 3), i32(3)) == (40 + 3 * 2 * 8 + 8) + 16 * 2 * 3     # 88 bytes round up to 96
    assert ws(i32(0, CAP), i32(0, CAP), i32(CAP)) == 40 + CAP * 256 * 8 + 8 + 16 * 256 * CAP
    assert ws(i32(0), i32(0), i32(), 0) == 0
    assert run_host(*good) == 0
    assert outs[0].tolist() == [36, 200, -7, -7] and outs[3].tolist()[8:] == [-7] * 4
    assert outs[1].tolist()[300:] == [-7] * 100 and outs[2].tolist()[64:] == [-7] * 336   # nothing behind the stated extents
    assert outs[3].tolist()[:8] == [64, 0, 36, 0, 0, 0, 200, 0]
    for o in outs:
        o[:] = -7
    bad = [
        (i32(0, 100, 99), i32(0, 64, 64), i32(5, 9)),        # offsets that decrease
        (i32(0, 100, 300), i32(0, 64, 63), i32(5, 9)),
        (i32(-1, 100, 300), i32(0, 64, 64), i32(5, 9)),      # a start below 0
        (i32(0, CAP + 1, CAP + 1), i32(0, 64, 64), i32(5, 9)),  # a length above the cap
        (i32(0, 100, 300), i32(0, 0, CAP + 1), i32(5, 9)),
        (i32(0, 100, 300), i32(0, 64, 64), i32(5, -1)),      # v < 0
    ]
    wsbuf = np.zeros(1 << 16, dtype=np.int64)
    base = (wsbuf.ctypes.data + 15) & ~15
    for case in bad:
        assert ws(*case) == E_ARG, case
        assert run_host(*case) == E_ARG, case
        assert run_dev(*case, base, wsbuf.nbytes - 16) == E_ARG, case
    assert ws(*good, N=-1) == E_ARG and run_host(*good, N=-1) == E_ARG
    need = ws(*good)
    assert run_dev(*good, base, need - 1) == E_ARG        # a workspace smaller than required
    assert run_dev(*good, base + 8, wsbuf.nbytes - 24) == E_ARG  # misaligned: 16 bytes are asked for
    assert run_dev(*good, base + 4, wsbuf.nbytes - 24) == E_ARG
    assert run_dev(*good, None, need) == E_ARG
    assert run_dev(*good, base, wsbuf.nbytes - 16, a=None) == E_ARG
    for k in range(4):                                    # any output missing
        ptr = list(optr)
        ptr[k] = None
        assert run_dev(*good, base, wsbuf.nbytes - 16, ptr=ptr) == E_ARG and run_host(*good, ptr=ptr) == E_ARG
    assert run_dev(i32(0), i32(0), i32(), None, 0, N=0) == 0 and run_host(i32(0), i32(0), i32(), N=0) == 0  # N == 0: nothing launched
    assert all(o.tolist() == [-7] * len(o) for o in outs)


# ------------------------------------------------------------------------------------------------ the Python layer
def test_sequence_alignments_on_strings_and_word_lists():
    from manuscript_ocr_amd.recognizers import Alignment, sequence_alignments, sequence_edit_distances
    al = sequence_alignments(["kitten", "ab", "", "abc"], ["sitting", "ba", "xy", ""])
    assert all(isinstance(a, Alignment) for a in al)
    k = al[0]
    assert (k.distance, k.hits, k.substitutions, k.deletions, k.insertions) == (3, 4, 2, 0, 1)
    assert k.ref_to_hyp.tolist() == [0, 1, 2, 3, 4, 5] and k.hyp_to_ref.tolist() == [0, 1, 2, 3, 4, 5, -1]
    assert k.ref_to_hyp.dtype == np.int32 and k.hyp_to_ref.dtype == np.int32
    assert (al[1].distance, al[1].substitutions) == (2, 2)
    assert (al[2].distance, al[2].insertions, al[2].hyp_to_ref.tolist(), al[2].ref_to_hyp.tolist()) == (2, 2, [-1, -1], [])
    assert (al[3].distance, al[3].deletions, al[3].ref_to_hyp.tolist()) == (3, 3, [-1, -1, -1])
    # the reference is the pattern whatever the lengths: a dropped word is a deletion, an added one an insertion, on both sides
    ref = "the quick brown fox jumps over the lazy dog".split()
    short, longer = [w for w in ref if w != "brown"], ref[:4] + ["very"] + ref[4:]
    a, b = sequence_alignments([ref, ref], [short, longer])
    assert (a.deletions, a.insertions, a.substitutions, a.hits) == (1, 0, 0, 8) and a.ref_to_hyp.tolist() == [0, 1, -1, 2, 3, 4, 5, 6, 7]
    assert (b.deletions, b.insertions, b.substitutions, b.hits) == (0, 1, 0, 9) and b.hyp_to_ref.tolist() == [0, 1, 2, 3, -1, 4, 5, 6, 7, 8]
    a, = sequence_alignments([["a", ("b", 1), 3]], [["a", ("b", 1), 4, 3]])                    # any hashable is a token
    assert a.distance == 1 and a.hyp_to_ref.tolist() == [0, 1, -1, 2]
    long_a = "the quick brown fox jumps over the lazy dog " * 40
    long_b = long_a.replace("quick", "quack").replace("lazy ", "")
    c, w = sequence_alignments([long_a, long_a.split()], [long_b, long_b.split()])
    assert (c.distance, c.substitutions, c.deletions, c.insertions) == (240, 40, 200, 0)
    assert (w.distance, w.substitutions, w.deletions, w.insertions) == (80, 40, 40, 0)
    assert [c.distance, w.distance] == sequence_edit_distances([long_a, long_a.split()], [long_b, long_b.split()]).tolist()
    assert sequence_alignments([], []) == []
    assert sequence_alignments(["x" * CAP], ["x" * (CAP - 1)])[0].deletions == 1
    with pytest.raises(ValueError):
        sequence_alignments(["x" * (CAP + 1)], ["x"])
    with pytest.raises(ValueError):
        sequence_alignments(["a"], [["w"] * (CAP + 1)])
    with pytest.raises(ValueError):
        sequence_alignments(["a"], [])
    with pytest.raises(TypeError):
        sequence_alignments([5], ["a"])


def test_error_breakdown_by_hand():
    from manuscript_ocr_amd.recognizers import error_breakdown
    r = error_breakdown(["минин", "abc", "abcd"], ["мнннн", "abxc", "acd"])
    assert (r["hits"], r["substitutions"], r["deletions"], r["insertions"]) == (3 + 3 + 3, 2, 1, 1)
    assert r["confusions"] == Counter({("и", "н"): 2, (None, "x"): 1, ("b", None): 1})
    r = error_breakdown(["a b c d".split()], ["a x c".split()])
    assert r["confusions"] == Counter({("b", "x"): 1, ("d", None): 1}) and r["hits"] == 2
    empty = error_breakdown([], [])
    assert empty["hits"] == empty["substitutions"] == 0 and empty["confusions"] == Counter()


def test_text_error_rates_breakdown_leaves_every_figure_as_it_is():
    from manuscript_ocr_amd.recognizers import text_error_rates
    from test_edit_distance_long_cpu import random_page_text
    rng = np.random.default_rng(3)
    refs = ["a b c", "", " ", "one   two\nthree ", "x y", "d e"] + [random_page_text(rng, 120 + 30 * k) for k in range(4)]
    hyps = ["a c b", "", "w", "one two three", "", "d x e"]
    for k, r in enumerate(refs[6:]):
        w = r.split()
        w[5] = "zz"
        del w[20:20 + 3 * k]
        w.insert(40, "extra")
        hyps.append(" ".join(w))
    plain, full = text_error_rates(refs, hyps), text_error_rates(refs, hyps, breakdown=True)
    assert set(full) == set(plain) | {"char_counts", "word_counts", "char_confusions", "word_confusions", "word_alignments"}
    for key, val in plain.items():
        if isinstance(val, np.ndarray):
            assert val.dtype == full[key].dtype and val.tolist() == full[key].tolist(), key
        else:
            assert val == full[key] and type(val) is type(full[key]), key
    for lvl, refs_len, hyp_len in (("char", plain["ref_chars"], [len(" ".join(h.split())) for h in hyps]),
                                   ("word", plain["ref_words"], [len(h.split()) for h in hyps])):
        c = full[lvl + "_counts"]
        assert c.shape == (len(refs), 4)
        assert (c[:, 1] + c[:, 2] + c[:, 3]).tolist() == plain[lvl + "_dist"].tolist()
        assert (c[:, 0] + c[:, 1] + c[:, 2]).tolist() == refs_len.tolist() and (c[:, 0] + c[:, 1] + c[:, 3]).tolist() == list(hyp_len)
        assert sum(full[lvl + "_confusions"].values()) == int(plain[lvl + "_dist"].sum())
    assert full["word_counts"][:6].tolist() == [[1, 2, 0, 0], [0, 0, 0, 0], [0, 0, 0, 1], [3, 0, 0, 0], [0, 0, 2, 0], [2, 0, 0, 1]]
    assert full["word_confusions"][("b", "c")] == 1 and full["word_confusions"][(None, "x")] == 1 and full["word_confusions"][("x", None)] == 1
    assert full["word_alignments"][5].hyp_to_ref.tolist() == [0, -1, 1] and len(full["word_alignments"]) == len(refs)
    assert full["word_alignments"][9].insertions == 1 and full["word_alignments"][9].deletions == 9
    empty = text_error_rates([], [], breakdown=True)
    assert empty["n"] == 0 and empty["char_counts"].shape == (0, 4) and empty["word_alignments"] == [] and not empty["word_confusions"]


def stand_in_pipeline(texts, det=None):
    """Pipeline over stand-in plugins: one box per text, two lines; the box filled with 10 + k reads as texts[k]"""
    from manuscript_ocr_amd import Pipeline
    from test_quad_match_cpu import StandInDetector, StandInRecognizer, rect
    if det is None:
        det = [rect(10 + 94 * (k % 4), 10 + 50 * (k // 4), 50 + 94 * (k % 4), 30 + 50 * (k // 4)) for k in range(len(texts))]
    img = np.full((140, 400, 3), 255, dtype=np.uint8)
    for k, q in enumerate(det):
        img[q[0][1]: q[2][1], q[0][0]: q[2][0]] = 10 + k
    return Pipeline(detector=StandInDetector(det), recognizer=StandInRecognizer({10 + k: t for k, t in enumerate(texts)})), img


def test_pipeline_evaluate_text_breakdown_on_stand_in_plugins():
    pipe, img = stand_in_pipeline(["alpha", "beta", "", "delta", "omega"])
    own = " ".join(w.text for b in pipe.predict(img).blocks for w in b.words if w.text)
    words = own.split()
    assert sorted(words) == ["alpha", "beta", "delta", "omega"]
    gts = [own, " ".join(words[:1] + words[2:]), " ".join(words[:2] + ["gamma"] + words[2:])]
    plain, full = pipe.evaluate_text([img] * 3, gts), pipe.evaluate_text([img] * 3, gts, breakdown=True)
    for key, val in plain.items():
        assert (val.tolist() == full[key].tolist()) if isinstance(val, np.ndarray) else (val == full[key]), key
    assert full["word_counts"].tolist() == [[4, 0, 0, 0], [3, 0, 0, 1], [4, 0, 1, 0]]
    assert full["word_confusions"] == Counter({(None, words[1]): 1, ("gamma", None): 1})
    assert full["word_alignments"][2].ref_to_hyp.tolist() == [0, 1, -1, 2, 3]
    assert full["char_counts"][0].tolist() == [len(own), 0, 0, 0]
    assert pipe.evaluate_text([], [], breakdown=True)["n"] == 0


def test_pipeline_transfer_text_on_stand_in_plugins():
    """A transcription handed to the boxes: a word the detector split in two, a word it dropped, a misread word, and max_cer."""
    from manuscript_ocr_amd.detectors._types import TransferWord
    pipe, img = stand_in_pipeline(["alpha", "be", "ta", "kappa", "", "dolta", "omega", "sigma"])
    flat = [w for b in pipe.predict(img).blocks for w in b.words]
    read = [w.text for w in flat if w.text]
    assert read == ["alpha", "be", "ta", "kappa", "dolta", "omega", "sigma"]  # two rows of four boxes, read row by row
    # the transcription: "beta" where the page has "be" "ta", "delta" for "dolta", and "gamma", which is not on the page
    gt_words = ["alpha", "beta", "kappa", "delta", "omega", "gamma", "sigma"]
    page, unpaired = pipe.transfer_text(img, "  ".join(gt_words) + "\n")
    out = [w for b in page.blocks for w in b.words]
    assert len(out) == len(flat) and [w.text for w in out] == [w.text for w in flat]
    got = {w.text: w for w in out if w.text}
    assert all(isinstance(w, TransferWord) for w in got.values())
    assert [w for w in out if not w.text] and not any(isinstance(w, TransferWord) for w in out if not w.text)
    for w, f in zip(out, flat):
        assert w.polygon == f.polygon and w.detection_confidence == f.detection_confidence and w.recognition_confidence == f.recognition_confidence
    assert (got["alpha"].gt_text, got["alpha"].char_distance) == ("alpha", 0) and got["alpha"].gt_index == gt_words.index("alpha")
    assert (got["omega"].gt_text, got["omega"].char_distance) == ("omega", 0)
    assert (got["dolta"].gt_text, got["dolta"].char_distance, got["dolta"].gt_index) == ("delta", 1, gt_words.index("delta"))
    # the split word: one half takes "beta" as a substitution, the other is an insertion and stays without a partner
    halves = [got["be"], got["ta"]]
    assert sorted((h.gt_text is None) for h in halves) == [False, True]
    kept = [h for h in halves if h.gt_text is not None][0]
    assert (kept.gt_text, kept.char_distance, kept.gt_index) == ("beta", 2, gt_words.index("beta"))
    lost = [h for h in halves if h.gt_text is None][0]
    assert lost.gt_index is None and lost.char_distance is None
    assert unpaired == [gt_words.index("gamma")]                    # the dropped word: a transcription word left without a box
    # max_cer: 1 / 5 passes 0.2, 2 / 4 does not pass 0.4
    page, unpaired = pipe.transfer_text(img, " ".join(gt_words), max_cer=0.4)
    got = {w.text: w for b in page.blocks for w in b.words if w.text}
    assert got["dolta"].gt_text == "delta" and got["be"].gt_text is None and got["ta"].gt_text is None
    assert got["be"].gt_index is None and got["be"].char_distance is None
    assert unpaired == sorted([gt_words.index("beta"), gt_words.index("gamma")])
    page, unpaired = pipe.transfer_text(img, " ".join(gt_words), max_cer=0.0)
    assert sorted(w.text for b in page.blocks for w in b.words if getattr(w, "gt_text", None)) == ["alpha", "kappa", "omega", "sigma"]
    assert unpaired == [1, 3, 5]
    # an empty transcription, and a page without text
    page, unpaired = pipe.transfer_text(img, "")
    assert unpaired == [] and all(w.gt_text is None for b in page.blocks for w in b.words if w.text)
    with pytest.raises(TypeError):
        pipe.transfer_text(img, ["alpha"])


# ------------------------------------------------------------------------------------------------ the sanitizers
def test_header_under_the_sanitizers(tmp_path):
    """csrc/edit_alignment.h (step, rule, host twin, argument check and workspace arithmetic) in a plain C++ program of its own
    (tests/native/edit_alignment_fuzz.cpp) with the address and undefined-behaviour sanitizers: garbage tokens and offsets, every
    array in a heap block of its exact size.  Run as a child process; nothing is loaded into this one."""
    cxx = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cxx):
        pytest.skip("the ROCm clang++ is not available")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "edit_alignment_fuzz"
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(root, "manuscript_ocr_amd", "csrc"),
                           os.path.join(root, "tests", "native", "edit_alignment_fuzz.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe), "400"], capture_output=True, text=True, timeout=600, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.startswith("rounds 400 checked 400")
