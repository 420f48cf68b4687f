"""Character n-gram language model, the parts that need no GPU: CharLM.from_texts against a slow dict-based
interpolated Witten-Bell written here, walk / logp against hand-computed values, the strict and lenient character rules, the
constructor's refusals and the new C-ABI symbols."""
import math
from collections import defaultdict

import numpy as np
import pytest

from manuscript_ocr_amd import _native as nat
from manuscript_ocr_amd.recognizers import CharLM

ITOS = ["<PAD>", "<SOS>", "<EOS>", "<BLANK>"] + [chr(ord("a") + i) for i in range(8)]  # 12 tokens
STOI = {s: i for i, s in enumerate(ITOS)}
STOI["_"] = STOI["<BLANK>"]  # a character the charset maps to the blank token
V = len(ITOS)
PAD, SOS, EOS, BLANK = 0, 1, 2, 3
EMIT = [v for v in range(V) if v not in (PAD, SOS, BLANK)]
TEXTS = ["abc", "abd", "bca", "a", "", "hgf", "abcabc", "cab", "dddd", "abc", "ge", "fa"]


def _encode(s):
    return [STOI[ch] for ch in s]


def _slow_witten_bell(texts, order):
    """P(v | h) for every context tuple h of length order - 1, by the recursion of the docstring of from_texts, with dicts."""
    cnt = [defaultdict(lambda: defaultdict(float)) for _ in range(order)]  # cnt[k][h of length k][v]
    for s in texts:
        seq = [SOS] * (order - 1) + _encode(s) + [EOS]
        for p in range(order - 1, len(seq)):
            for k in range(order):
                cnt[k][tuple(seq[p - k:p])][seq[p]] += 1.0

    def prob(h, v):
        if h is None:
            return 1.0 / len(EMIT) if v in EMIT else 0.0
        lower = prob(h[1:] if len(h) else None, v)
        c = cnt[len(h)].get(h)
        if not c:
            return lower
        tot, distinct = sum(c.values()), len(c)
        return (c.get(v, 0.0) + distinct * lower) / (tot + distinct)

    return prob


def _ctx_index(h):
    i = 0
    for t in h:
        i = i * V + t
    return i


@pytest.mark.parametrize("order", [1, 2, 3])
def test_from_texts_equals_a_slow_witten_bell(order):
    lm = CharLM.from_texts(TEXTS, STOI, order=order)
    assert lm.order == order and lm.num_classes == V and lm.n_ctx == V ** (order - 1) and lm.sos_id == SOS and lm.eos_id == EOS
    assert lm.table.dtype == np.float32 and lm.table.flags["C_CONTIGUOUS"] and lm.table.shape == (lm.n_ctx, V)
    prob = _slow_witten_bell(TEXTS, order)
    contexts = [()] if order == 1 else [(a,) for a in range(V)] if order == 2 else [(a, b) for a in range(V) for b in range(V)]
    want = np.array([[prob(h, v) for v in range(V)] for h in contexts])
    rows = [_ctx_index(h) for h in contexts]
    assert rows == list(range(lm.n_ctx))
    np.testing.assert_allclose(lm.prob64, want, rtol=1e-13, atol=0)
    # every row is a distribution over the emittable tokens, in float64 before the cast
    assert np.abs(lm.prob64[:, EMIT].sum(axis=1) - 1.0).max() < 1e-12
    assert (lm.prob64[:, [PAD, SOS, BLANK]] == 0).all()
    # the table is its logarithm, the three non-emittable columns hold the floor
    np.testing.assert_array_equal(lm.table[:, EMIT], np.log(want[:, EMIT]).astype(np.float32))
    assert (lm.table[:, [PAD, SOS, BLANK]] == np.float32(-30.0)).all() and np.isfinite(lm.table).all()
    assert (CharLM.from_texts(TEXTS, STOI, order=order, floor_logp=-12.5).table[:, [PAD, SOS, BLANK]] == np.float32(-12.5)).all()


def test_unseen_contexts_equal_their_backoff_row():
    lm1, lm2, lm3 = (CharLM.from_texts(TEXTS, STOI, order=o) for o in (1, 2, 3))
    h, g = STOI["h"], STOI["g"]
    # "e" is only ever followed by EOS; nothing follows PAD: an order-2 row that was never seen is the order-1 row
    np.testing.assert_array_equal(lm2.prob64[PAD], lm1.prob64[0])
    # (a, h) never occurs, h does: the order-3 row backs off to the order-2 row of h; (PAD, PAD) goes down to order 1
    a = STOI["a"]
    np.testing.assert_array_equal(lm3.prob64[a * V + h], lm2.prob64[h])
    np.testing.assert_array_equal(lm3.prob64[PAD * V + PAD], lm1.prob64[0])
    # a seen context differs from its back-off row
    assert np.abs(lm3.prob64[h * V + g] - lm2.prob64[g]).max() > 1e-3
    # no text at all: every row is the uniform distribution over the emittable tokens
    lm0 = CharLM.from_texts([], STOI, order=2)
    np.testing.assert_array_equal(lm0.prob64[:, EMIT], np.full((V, len(EMIT)), 1.0 / len(EMIT)))


def test_walk_and_logp_by_hand():
    a, b, c = STOI["a"], STOI["b"], STOI["c"]
    lm = CharLM.from_texts(TEXTS, STOI, order=3)
    assert lm.ctx0 == SOS * V + SOS
    # the all-SOS start; a word that ends early keeps its context from the EOS on
    assert lm.walk([]) == []
    assert lm.walk([a, b, EOS, EOS, c]) == [SOS * V + a, a * V + b, a * V + b, a * V + b, a * V + b]
    assert lm.walk([a, b, c, a]) == [SOS * V + a, a * V + b, b * V + c, c * V + a]
    t = lm.table.astype(np.float64)
    want = t[SOS * V + SOS, a] + t[SOS * V + a, b] + t[a * V + b, EOS]
    got = lm.logp([a, b, EOS, c, c])
    assert isinstance(got, float) and got == want
    assert lm.logp([a, b, EOS]) == want and lm.logp([a, b, EOS, -1, -1]) == want
    assert lm.logp([a, b]) == t[SOS * V + SOS, a] + t[SOS * V + a, b]  # no EOS: all of it
    assert lm.logp([]) == 0.0
    lm2 = CharLM.from_texts(TEXTS, STOI, order=2)
    assert lm2.ctx0 == SOS and lm2.walk([a, b, EOS, c]) == [a, b, b, b]
    assert lm2.logp([b, EOS]) == float(lm2.table[SOS, b]) + float(lm2.table[b, EOS])
    lm1 = CharLM.from_texts(TEXTS, STOI, order=1)
    assert lm1.ctx0 == 0 and lm1.n_ctx == 1 and lm1.walk([a, b, c, EOS, a]) == [0, 0, 0, 0, 0]
    assert lm1.logp([a, c, EOS, a]) == float(lm1.table[0, a]) + float(lm1.table[0, c]) + float(lm1.table[0, EOS])
    # the unigram of "a": 8 of the 39 training tokens (27 letters, 12 EOS), 9 distinct tokens seen, uniform 1 / 9 below
    n_tok = sum(len(s) + 1 for s in TEXTS)
    n_a = sum(s.count("a") for s in TEXTS)
    distinct = len(set("".join(TEXTS))) + 1
    assert math.isclose(lm1.prob64[0, a], (n_a + distinct / len(EMIT)) / (n_tok + distinct), rel_tol=1e-14)
    # a table of one's own, without an eos_id: nothing ends the walk
    own = CharLM(np.zeros((V, V)), V, 2, SOS)
    assert own.eos_id is None and own.walk([a, EOS, b]) == [a, EOS, b] and own.logp([a, EOS, b]) == 0.0
    assert CharLM.from_table(np.zeros((V, V)), {s: i for i, s in enumerate(ITOS)}, 2).walk([a, EOS, b]) == [a, a, a]
    with pytest.raises(ValueError, match="outside"):
        lm.walk([a, V])


def test_strict_and_lenient_characters():
    with pytest.raises(ValueError, match=r"texts\[1\] = 'a!b'.*'!' is not in the charset"):
        CharLM.from_texts(["ab", "a!b"], STOI)
    with pytest.raises(ValueError, match=r"texts\[0\].*'_' is the <BLANK> token"):
        CharLM.from_texts(["a_b"], STOI)
    with pytest.raises(TypeError):
        CharLM.from_texts(["ab", 3], STOI)
    lenient = CharLM.from_texts(["ab", "a!b", "a_b"], STOI, order=2, strict=False)
    np.testing.assert_array_equal(lenient.table, CharLM.from_texts(["ab", "ab", "ab"], STOI, order=2).table)
    with pytest.raises(ValueError, match="<EOS>"):
        CharLM.from_texts(["ab"], {"<PAD>": 0, "<SOS>": 1, "a": 2, "b": 3})
    with pytest.raises(ValueError, match="finite"):
        CharLM.from_texts(["ab"], STOI, floor_logp=-np.inf)


def test_constructor_refusals():
    ok = np.zeros((V * V, V), dtype=np.float64)
    lm = CharLM(ok, V, 3, SOS)
    assert lm.table.dtype == np.float32 and lm.table.shape == (V * V, V)
    lm_t = CharLM(np.asfortranarray(np.arange(V * V, dtype=np.float64).reshape(V, V)), V, 2, SOS)
    assert lm_t.table.flags["C_CONTIGUOUS"] and lm_t.table[1, 2] == V + 2
    for bad in (np.nan, np.inf, -np.inf):
        t = ok.copy()
        t[5, 3] = bad
        with pytest.raises(ValueError, match="non-finite"):
            CharLM(t, V, 3, SOS)
    with pytest.raises(ValueError, match="float32 range"):
        CharLM(np.full((1, V), -1e300), V, 1, SOS)
    for shape in ((V, V), (V * V, V + 1), (V * V * V,), (V * V, V, 1)):
        with pytest.raises(ValueError, match="shape"):
            CharLM(np.zeros(shape), V, 3, SOS)
    for order in (0, 4, -1, 2.0, None):
        with pytest.raises(ValueError, match="order"):
            CharLM(ok, V, order, SOS)
        with pytest.raises(ValueError, match="order"):
            CharLM.from_texts(TEXTS, STOI, order=order)
    for sos in (-1, V):
        with pytest.raises(ValueError, match="sos_id"):
            CharLM(ok, V, 3, sos)
    # the size cap: 512^3 = 2^27 elements is refused before the table is looked at (none is allocated here), 406^3 <= 2^26 < 407^3
    with pytest.raises(ValueError, match="2\\^26"):
        CharLM(None, 512, 3, SOS)
    with pytest.raises(ValueError, match="2\\^26"):
        CharLM(None, 407, 3, SOS)
    with pytest.raises(ValueError, match="shape"):  # under the cap: the (absent) table is looked at
        CharLM(None, 406, 3, SOS)
    big = {**{s: i for i, s in enumerate(ITOS)}, "z": 511}
    with pytest.raises(ValueError, match="2\\^26"):
        CharLM.from_texts(["az"], big, order=3)
    assert CharLM.from_texts(["az"], big, order=2).table.shape == (512, 512)


def test_new_symbols_are_exported():
    L = nat.lib()
    for name in ("msocr_attn_beam_slots_bytes", "msocr_attn_decode"):
        assert hasattr(L, name)
    assert L.msocr_attn_beam_slots_bytes(37, 9, 8) == 37 * 9 * 8 * 4
    assert L.msocr_attn_beam_slots_bytes(0, 9, 8) == 0
    st = nat.CharLMTable()
    st.table, st.order, st.V, st.n_ctx = 16, 3, 194, 194 * 194
    assert (st.order, st.V, st.n_ctx) == (3, 194, 37636)
