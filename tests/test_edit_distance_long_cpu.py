"""Page-level error rates, host side: csrc/edit_distance_long.h through the host twin
msocr_edit_distance_long_host against a plain NumPy row programme, the C ABI's refusals, recognizers.sequence_edit_distances /
word_error_rate / text_error_rates by hand, Pipeline.evaluate_text on stand-in plugins, and the header in a C++ program of its own
under the address and undefined-behaviour sanitizers (tests/native/edit_distance_long_fuzz.cpp).  No GPU.

Every comparison is integer equality.  tests/test_gpu_edit_distance_long.py imports the helpers of this file."""
import os
import subprocess

import numpy as np
import pytest

E_ARG = -1
CAP = 16384


def _lib():
    from manuscript_ocr_amd import _native as nat
    return nat.lib()


def ref_distance(a, b, v):
    """The textbook dynamic programme, one NumPy row per token of the shorter side (the distance and the matching rule are
    symmetric): cur = min(prev + 1, prev_shift + (b != x)), then the insertions along the row by minimum.accumulate.  A token
    outside [0, v) equals nothing."""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    if len(a) > len(b):
        a, b = b, a
    n = len(b)
    ar = np.arange(n + 1)
    prev = ar.copy()
    for i, x in enumerate(a.tolist()):
        cur = np.empty(n + 1, dtype=np.int64)
        cur[0] = i + 1
        ne = (b != x).astype(np.int64) if 0 <= x < v else 1
        cur[1:] = np.minimum(prev[1:] + 1, prev[:-1] + ne)
        prev = np.minimum.accumulate(cur - ar) + ar
    return int(prev[n])


def csr(seqs):
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int32)
    tok = np.concatenate([np.asarray(s, dtype=np.int32) for s in seqs] + [np.zeros(0, dtype=np.int32)])
    return tok, off


def host(pairs):
    """pairs: (a, b, v) -> the host twin's distances"""
    from manuscript_ocr_amd import ops
    a_tok, a_off = csr([p[0] for p in pairs])
    b_tok, b_off = csr([p[1] for p in pairs])
    return ops.edit_distance_long_host(a_tok, a_off, b_tok, b_off, [p[2] for p in pairs]).tolist()


def random_pair(rng, m, n, v, foreign=2):
    """a over [0, v), b over [0, v + foreign): some of b's tokens match nothing"""
    return rng.integers(0, v, m).astype(np.int32), rng.integers(0, v + foreign, n).astype(np.int32), v


PATTERN_LENS = (0, 1, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097)
OTHER_LENS = (0, 1, 64, 65, 700)


@pytest.mark.parametrize("v", [2, 4, 30, 1000])
def test_host_twin_against_the_row_programme(v):
    rng = np.random.default_rng(100 + v)
    pairs = [random_pair(rng, m, n, v) for m in PATTERN_LENS for n in OTHER_LENS]
    assert host(pairs) == [ref_distance(*p) for p in pairs]


def structured_pairs():
    rng = np.random.default_rng(7)
    word = rng.integers(0, 30, 1000).astype(np.int32)
    motif = np.tile(np.array([3, 1, 4, 1, 5, 9, 2, 6], dtype=np.int32), 90)
    edited = np.delete(motif, [5, 77, 300])
    edited[100] = 7
    wild = np.array([-1, 2**31 - 1, -2**31, 40, 5, 5, 77], dtype=np.int32)
    return [
        (word, word.copy(), 30),                                      # equal: 0
        (word[:129], word[:129].copy(), 30),
        (word, word + 30, 60),                                        # disjoint alphabets: max(m, n)
        (word[:65], (word + 30)[:700], 60),
        (motif, edited, 10),                                          # a repeated motif against an edited copy
        (edited, np.tile(motif, 3), 10),
        (np.arange(200, dtype=np.int32), np.arange(200, dtype=np.int32), 100),   # the upper half of the pattern matches nothing
        (np.tile(wild, 20), np.tile(wild, 20), 50),                   # garbage tokens on both sides
        (word[:300], np.tile(wild, 30), 6),
        (np.zeros(130, dtype=np.int32), np.zeros(70, dtype=np.int32), 1),
        (np.zeros(130, dtype=np.int32), np.zeros(70, dtype=np.int32), 0),        # an empty alphabet: nothing matches
    ]


def test_structured_sequences():
    pairs = structured_pairs()
    got = host(pairs)
    assert got == [ref_distance(*p) for p in pairs]
    assert got[0] == 0 and got[1] == 0 and got[2] == 1000 and got[3] == 700 and got[6] == 100 and got[9] == 60 and got[10] == 130


def test_one_pair_at_the_cap():
    rng = np.random.default_rng(11)
    a = rng.integers(0, 4, CAP).astype(np.int32)
    b = a.copy()
    b[rng.integers(0, CAP, 3000)] = rng.integers(0, 5, 3000)
    b = np.roll(b, 7)
    assert host([(a, b, 4)]) == [ref_distance(a, b, 4)]


def test_short_pairs_equal_the_64_symbol_entry_point():
    rng = np.random.default_rng(5)
    B, V = 48, 12
    eos, pad = V - 1, V - 2  # the pair entry point's text rule: tokens below them are text
    la, lb = rng.integers(0, 65, B).astype(np.int32), rng.integers(0, 65, B).astype(np.int32)
    la[:3], lb[:3] = (0, 64, 64), (64, 0, 64)
    a = np.full((B, 64), eos, dtype=np.int32)
    b = np.full((B, 64), eos, dtype=np.int32)
    for r in range(B):
        a[r, :la[r]] = rng.integers(0, V - 2, la[r])
        b[r, :lb[r]] = rng.integers(0, V - 2, lb[r])
    out = [np.empty(B, dtype=np.int32) for _ in range(3)]
    assert _lib().msocr_edit_distance_pairs_host(a.ctypes.data, la.ctypes.data, 64, b.ctypes.data, lb.ctypes.data, 64, B, V, eos, pad, -1,
                                                 *(o.ctypes.data for o in out)) == 0
    assert out[1].tolist() == la.tolist() and out[2].tolist() == lb.tolist()
    assert host([(a[r, :la[r]], b[r, :lb[r]], V) for r in range(B)]) == out[0].tolist()


def test_symbols_and_wrappers_are_exported():
    from manuscript_ocr_amd import _native as nat
    from manuscript_ocr_amd import ops
    for name in ("msocr_edit_distance_long_ws_bytes", "msocr_edit_distance_long", "msocr_edit_distance_long_host"):
        assert name in nat.exported_symbols() and hasattr(_lib(), name)
    assert callable(ops.edit_distance_long) and callable(ops.edit_distance_long_host) and ops.EDL_MAX_LEN == CAP


def test_abi_refusals():
    """Everything here is refused (or is N == 0) before any launch: no GPU is touched."""
    L = _lib()
    i32 = lambda *x: np.array(x, dtype=np.int32)  # noqa: E731
    tok = np.zeros(CAP + 8, dtype=np.int32)
    out = np.full(4, -7, dtype=np.int32)
    good = (i32(0, 100, 300), i32(0, 64, 64), i32(5, 9))

    def ws(a_off, b_off, v, N=None):
        return L.msocr_edit_distance_long_ws_bytes(a_off.ctypes.data, b_off.ctypes.data, v.ctypes.data, len(v) if N is None else N)

    def run_host(a_off, b_off, v, N=None):
        return L.msocr_edit_distance_long_host(tok.ctypes.data, a_off.ctypes.data, tok.ctypes.data, b_off.ctypes.data, v.ctypes.data,
                                               len(v) if N is None else N, out.ctypes.data)

    def run_dev(a_off, b_off, v, ws_ptr, ws_bytes, N=None):  # `tok` stands in for device memory: a refused call reads nothing
        return L.msocr_edit_distance_long(tok.ctypes.data, a_off.ctypes.data, tok.ctypes.data, b_off.ctypes.data, v.ctypes.data,
                                          len(v) if N is None else N, out.ctypes.data, ws_ptr, ws_bytes, None)

    # the workspace formula of include/msocr.h: 32 N + sum v * ceil(m / 64) * 8
    assert ws(*good) == 32 * 2 + (5 * 2 + 9 * 4) * 8
    assert ws(i32(0, CAP), i32(0, CAP), i32(CAP)) == 32 + CAP * 256 * 8
    assert ws(i32(0), i32(0), i32(), 0) == 0
    assert run_host(*good) == 0 and out.tolist()[2:] == [-7, -7]
    bad = [
        (i32(0, 100, 99), i32(0, 64, 64), i32(5, 9)),        # offsets that decrease
        (i32(0, 100, 300), i32(0, 64, 63), i32(5, 9)),
        (i32(-1, 100, 300), i32(0, 64, 64), i32(5, 9)),      # a start below 0
        (i32(0, CAP + 1, CAP + 1), i32(0, 64, 64), i32(5, 9)),  # a length above the cap
        (i32(0, 100, 300), i32(0, 0, CAP + 1), i32(5, 9)),
        (i32(0, 100, 300), i32(0, 64, 64), i32(5, -1)),      # v < 0
    ]
    wsbuf = np.zeros(1 << 16, dtype=np.int64)
    for case in bad:
        assert ws(*case) == E_ARG, case
        assert run_host(*case) == E_ARG, case
        assert run_dev(*case, wsbuf.ctypes.data, wsbuf.nbytes) == E_ARG, case
    assert ws(*good, N=-1) == E_ARG and run_host(*good, N=-1) == E_ARG
    need = ws(*good)
    assert run_dev(*good, wsbuf.ctypes.data, need - 1) == E_ARG        # a workspace smaller than required
    assert run_dev(*good, wsbuf.ctypes.data + 4, wsbuf.nbytes - 4) == E_ARG  # misaligned
    assert run_dev(*good, None, need) == E_ARG
    assert L.msocr_edit_distance_long(None, good[0].ctypes.data, tok.ctypes.data, good[1].ctypes.data, good[2].ctypes.data, 2,
                                      out.ctypes.data, wsbuf.ctypes.data, wsbuf.nbytes, None) == E_ARG
    assert L.msocr_edit_distance_long_host(tok.ctypes.data, good[0].ctypes.data, tok.ctypes.data, good[1].ctypes.data,
                                           good[2].ctypes.data, 2, None) == E_ARG
    assert run_dev(i32(0), i32(0), i32(), None, 0, N=0) == 0 and run_host(i32(0), i32(0), i32(), N=0) == 0  # N == 0: nothing launched
    assert out.tolist()[2:] == [-7, -7]


# ------------------------------------------------------------------------------------------------ the Python layer
def test_sequence_edit_distances_on_strings_and_word_lists():
    from manuscript_ocr_amd.recognizers import edit_distances, sequence_edit_distances
    refs = ["kitten", "flaw", "", "", "abc", "слово", "x" * 64]
    hyps = ["sitting", "lawn", "", "ab", "abc", "слова", "y" + "x" * 63]
    assert sequence_edit_distances(refs, hyps).tolist() == [3, 2, 0, 2, 0, 1, 1] == edit_distances(refs, hyps).tolist()
    long_a = "the quick brown fox jumps over the lazy dog " * 40
    long_b = long_a.replace("quick", "quack").replace("lazy ", "")
    assert sequence_edit_distances([long_a], [long_b]).tolist() == [40 * (1 + 5)]
    assert sequence_edit_distances([long_a.split()], [long_b.split()]).tolist() == [40 * 2]
    assert sequence_edit_distances([["a", ("b", 1), 3]], [["a", ("b", 1), 4, 3]]).tolist() == [1]   # any hashable is a token
    assert sequence_edit_distances([list("abc"), "abc"], ["abd", tuple("xabc")]).tolist() == [1, 1]
    assert sequence_edit_distances([], []).tolist() == []
    assert sequence_edit_distances(["x" * CAP], ["x" * (CAP - 1)]).tolist() == [1]
    with pytest.raises(ValueError):
        sequence_edit_distances(["x" * (CAP + 1)], ["x"])
    with pytest.raises(ValueError):
        sequence_edit_distances(["a"], [["w"] * (CAP + 1)])
    with pytest.raises(ValueError):
        sequence_edit_distances(["a"], [])
    with pytest.raises(TypeError):
        sequence_edit_distances([5], ["a"])


def test_the_64_character_rule_of_edit_distances_stands():
    from manuscript_ocr_amd.recognizers import edit_distances
    with pytest.raises(ValueError):
        edit_distances(["x" * 65], ["x"])


def test_word_error_rate_and_text_error_rates_by_hand():
    from manuscript_ocr_amd.recognizers import text_error_rates, word_error_rate
    assert word_error_rate("a b c", "a c b") == 2 / 3
    assert word_error_rate("a b c", "a b c") == 0.0 and word_error_rate("a  b\tc\n", "a b c") == 0.0
    assert word_error_rate("", "") == 0.0 and word_error_rate("  ", "a") == float("inf") and word_error_rate("a b", "") == 1.0
    r = text_error_rates(["a b c", "", " ", "one   two\nthree ", "x y"], ["a c b", "", "w", "one two three", ""])
    assert r["word_dist"].tolist() == [2, 0, 1, 0, 2] and r["ref_words"].tolist() == [3, 0, 0, 3, 2]
    assert r["bag_errors"].tolist() == [0, 0, 1, 0, 2]
    assert r["char_dist"].tolist() == [2, 0, 1, 0, 3] and r["ref_chars"].tolist() == [5, 0, 0, 13, 3]
    assert r["cer"].tolist() == [2 / 5, 0.0, float("inf"), 0.0, 1.0] and r["wer"].tolist() == [2 / 3, 0.0, float("inf"), 0.0, 1.0]
    assert r["n"] == 5 and r["cer_micro"] == 6 / 21 and r["wer_micro"] == 5 / 8 and r["bag_error_rate"] == 3 / 8
    assert r["cer_mean"] == float("inf") and r["wer_mean"] == float("inf")
    r = text_error_rates(["a b c", "d e"], ["a b", "d x e"])
    assert (r["cer_mean"], r["wer_mean"]) == ((2 / 5 + 2 / 3) / 2, (1 / 3 + 1 / 2) / 2) and r["wer_micro"] == 2 / 5
    empty = text_error_rates([], [])
    assert empty["n"] == 0 and empty["cer_micro"] == empty["wer_micro"] == empty["cer_mean"] == empty["wer_mean"] == 0.0
    assert text_error_rates([""], ["a"])["wer_micro"] == float("inf")
    with pytest.raises(ValueError):
        text_error_rates(["a"], [])
    with pytest.raises(TypeError):
        text_error_rates([["a"]], ["a"])


def random_page_text(rng, n_words, vocab=300):
    return " ".join(f"w{int(k)}" for k in rng.integers(0, vocab, n_words))


def test_bag_errors_bound_the_word_distance_on_random_pages():
    from manuscript_ocr_amd.recognizers import text_error_rates
    rng = np.random.default_rng(3)
    refs, hyps = [], []
    for k in range(12):
        words = random_page_text(rng, 150 + 20 * k).split()
        hyp = list(words)
        for _ in range(k):  # a few substitutions, one dropped line, then two columns read across
            hyp[int(rng.integers(0, len(hyp)))] = "zz"
        del hyp[10:10 + k]
        if k % 2:
            half = len(hyp) // 2
            hyp = [w for pair in zip(hyp[:half], hyp[half:2 * half]) for w in pair] + hyp[2 * half:]
        refs.append(" ".join(words))
        hyps.append(" ".join(hyp))
    r = text_error_rates(refs, hyps)
    assert np.all(r["bag_errors"] <= r["word_dist"]) and np.all(r["word_dist"] <= np.maximum(r["ref_words"], [len(h.split()) for h in hyps]))
    assert np.all(r["word_dist"][1::2] > r["bag_errors"][1::2] + 20)  # the interleaved pages: the order costs what the bag does not see
    assert r["word_dist"].tolist() == [ref_words_distance(a, b) for a, b in zip(refs, hyps)]


def ref_words_distance(a, b):
    ids = {}
    ia = [ids.setdefault(w, len(ids)) for w in a.split()]
    ib = [ids.setdefault(w, len(ids)) for w in b.split()]
    return ref_distance(ia, ib, len(ids))


def test_pipeline_evaluate_text_on_stand_in_plugins():
    """Four words on two lines.  The pipeline's own text as the transcription gives zeros; the same words reversed leave the bag
    intact and cost word errors; a transcription with other whitespace is the same transcription."""
    from manuscript_ocr_amd import Pipeline
    from test_quad_match_cpu import StandInDetector, StandInRecognizer, rect
    det = [rect(10, 10, 50, 30), rect(104, 10, 144, 30), rect(10, 60, 50, 80), rect(120, 60, 160, 80)]
    img = np.full((140, 260, 3), 255, dtype=np.uint8)
    for k, q in enumerate(det):
        img[q[0][1]: q[2][1], q[0][0]: q[2][0]] = 10 + k
    pipe = Pipeline(detector=StandInDetector(det), recognizer=StandInRecognizer({10: "alpha", 11: "beta", 12: "", 13: "delta"}))
    own = " ".join(w.text for b in pipe.predict(img).blocks for w in b.words if w.text)
    assert sorted(own.split()) == ["alpha", "beta", "delta"]  # the word without text is skipped
    r = pipe.evaluate_text([img, img], [own, "  " + own.replace(" ", "\n ")])
    assert r["hypotheses"] == [own, own] and r["n"] == 2
    for key in ("char_dist", "word_dist", "bag_errors", "cer", "wer"):
        assert r[key].tolist() == [0, 0], key
    assert r["ref_words"].tolist() == [3, 3] and r["cer_micro"] == r["wer_micro"] == r["cer_mean"] == r["wer_mean"] == 0.0
    r = pipe.evaluate_text([img], [" ".join(reversed(own.split()))])
    assert r["word_dist"].tolist() == [2] and r["wer"][0] == 2 / 3 and r["wer_micro"] > 0 and r["bag_errors"].tolist() == [0]
    assert r["char_dist"][0] > 0
    assert pipe.evaluate_text([], [])["n"] == 0
    with pytest.raises(ValueError):
        pipe.evaluate_text([img], [])


# ------------------------------------------------------------------------------------------------ the sanitizers
def test_header_under_the_sanitizers(tmp_path):
    """csrc/edit_distance_long.h (recurrence, host twin, argument check) in a plain C++ program of its own
    (tests/native/edit_distance_long_fuzz.cpp) with the address and undefined-behaviour sanitizers: garbage tokens and offsets, every
    array in a heap block of its exact size.  Run as a child process; nothing is loaded into this one."""
    cxx = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cxx):
        pytest.skip("the ROCm clang++ is not available")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "edit_distance_long_fuzz"
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(root, "manuscript_ocr_amd", "csrc"),
                           os.path.join(root, "tests", "native", "edit_distance_long_fuzz.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe), "400"], capture_output=True, text=True, timeout=600, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.startswith("rounds 400 checked 400")
