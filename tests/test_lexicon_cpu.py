"""Lexicon-constrained decode, the parts that need no GPU: the Lexicon class's trie arrays against a
dict-of-dicts trie built here, its strict and lenient word rules, msocr_lexicon_check_host on the built trie and on single corruptions
of it, and the new C-ABI symbols."""
import numpy as np
import pytest

from manuscript_ocr_amd import _native as nat
from manuscript_ocr_amd.recognizers import Lexicon
from manuscript_ocr_amd.recognizers._trba.transforms import pack_targets

E_ARG = -1
ITOS = ["<PAD>", "<SOS>", "<EOS>", "<BLANK>"] + [chr(ord("a") + i) for i in range(12)]
STOI = {s: i for i, s in enumerate(ITOS)}
STOI["_"] = STOI["<BLANK>"]  # a character the charset maps to the blank token
V = len(ITOS)
EOS = STOI["<EOS>"]
MAX_LEN = 9


def _words(seed=11, n=300):
    """Seeded word list, lengths 1 .. MAX_LEN - 1 over 12 letters (4 in the first two places: shared prefixes), with duplicates and a
    word that is a prefix of another."""
    rng = np.random.default_rng(seed)
    letters = ITOS[4:]
    out = []
    for _ in range(n - 6):
        L = int(rng.integers(1, MAX_LEN))
        out.append("".join(letters[int(rng.integers(0, 4 if k < 2 else 12))] for k in range(L)))
    out += ["abcd", "abcdefgh", "abcd", out[0], out[5], "l"]
    return out


def _dict_trie(words):
    """(root dict-of-dicts with "$" -> index into the deduplicated list, deduplicated list)."""
    root, uniq, seen = {}, [], set()
    for w in words:
        if w in seen:
            continue
        seen.add(w)
        d = root
        for ch in w:
            d = d.setdefault(ch, {})
        d["$"] = len(uniq)
        uniq.append(w)
    return root, uniq


@pytest.fixture(scope="module")
def lex():
    return Lexicon(_words(), STOI, MAX_LEN)


def test_arrays_equal_a_dict_trie(lex):
    words = _words()
    root, uniq = _dict_trie(words)
    assert len(uniq) < len(words) and lex.words == uniq and len(lex) == len(uniq)
    assert lex.edge_begin.dtype == lex.edge_tok.dtype == lex.edge_child.dtype == lex.word_of_node.dtype == np.int32
    assert lex.terminal.dtype == np.uint8
    assert lex.edge_begin.shape == (lex.n_nodes + 1,) and lex.edge_tok.shape == lex.edge_child.shape == (lex.n_edges,)
    assert lex.n_edges == lex.n_nodes - 1  # a tree
    # walk both tries together, breadth-first: node ids come out as 0, 1, 2, ... in that order
    queue, nxt = [(0, root)], 1
    while queue:
        node, d = queue.pop(0)
        lo, hi = lex.edge_begin[node], lex.edge_begin[node + 1]
        keys = sorted((STOI[ch], ch) for ch in d if ch != "$")
        assert lex.edge_tok[lo:hi].tolist() == [k for k, _ in keys]
        assert (np.diff(lex.edge_tok[lo:hi]) > 0).all()
        assert lex.edge_child[lo:hi].tolist() == list(range(nxt, nxt + len(keys))), "breadth-first numbering"
        assert (lex.edge_child[lo:hi] > node).all()
        assert lex.word_of_node[node] == d.get("$", -1) and lex.terminal[node] == ("$" in d)
        queue += [(nxt + i, d[ch]) for i, (_, ch) in enumerate(keys)]
        nxt += len(keys)
    assert nxt == lex.n_nodes
    leaves = np.flatnonzero(np.diff(lex.edge_begin) == 0)
    assert lex.terminal[leaves].all()
    # word_of_node is a bijection between terminal nodes and words
    assert sorted(lex.word_of_node[lex.word_of_node >= 0].tolist()) == list(range(len(uniq)))


def test_find_members_non_members_and_padding(lex):
    _, uniq = _dict_trie(_words())
    rng = np.random.default_rng(3)
    assert "abcd" in uniq and "abcdefgh" in uniq
    for i, w in enumerate(uniq):
        ids = [STOI[c] for c in w]
        assert lex.find(ids) == i
        assert lex.find(ids + [EOS]) == i
        assert lex.find(np.array(ids + [EOS] + [-1] * 3, dtype=np.int32)) == i
        assert lex.find(ids + [-1, STOI["a"]]) == i  # nothing behind the first -1 is read
        assert lex.find(ids + [EOS, STOI["a"]]) == i
    # the ids pack_targets gives a word are found too (target row: ids, EOS, PAD...)
    _, target, _, _ = pack_targets(uniq[:20], STOI, MAX_LEN)
    assert [lex.find(row) for row in target] == list(range(20))
    members, misses = set(uniq), 0
    for _ in range(400):
        w = "".join(ITOS[4 + int(rng.integers(0, 12))] for _ in range(int(rng.integers(1, MAX_LEN))))
        if w not in members:
            misses += 1
            assert lex.find([STOI[c] for c in w]) == -1, w
    assert misses > 100
    assert lex.find([]) == -1 and lex.find([EOS]) == -1 and lex.find([-1]) == -1      # the empty word is none
    assert lex.find([STOI["a"], STOI["b"], STOI["c"]]) == (uniq.index("abc") if "abc" in members else -1)  # a proper prefix
    assert lex.find([STOI["<PAD>"]]) == -1 and lex.find([500]) == -1


def test_strict_names_the_word_and_lenient_drops_it():
    good = ["ab", "ba"]
    for bad, why in (("aXb", "not in the charset"), ("a_b", "<BLANK>"), ("", "empty"), ("a" * MAX_LEN, "max_len")):
        with pytest.raises(ValueError) as e:
            Lexicon(good + [bad], STOI, MAX_LEN)
        assert repr(bad) in str(e.value) and why in str(e.value), str(e.value)
        lenient = Lexicon(good + [bad], STOI, MAX_LEN, strict=False)
        assert lenient.words == good
    assert Lexicon(["a" * (MAX_LEN - 1)], STOI, MAX_LEN).words == ["a" * (MAX_LEN - 1)]  # the longest word that leaves room for EOS
    with pytest.raises(ValueError, match="empty"):
        Lexicon([], STOI, MAX_LEN)
    with pytest.raises(ValueError, match="empty"):
        Lexicon(["X", ""], STOI, MAX_LEN, strict=False)
    with pytest.raises(TypeError):
        Lexicon([3], STOI, MAX_LEN)
    # the charset as a list of tokens is the same lexicon
    a, b = Lexicon(good, STOI, MAX_LEN), Lexicon(good, ITOS, MAX_LEN)
    assert a.edge_tok.tolist() == b.edge_tok.tolist() and a.eos_id == b.eos_id == EOS and a.num_classes == b.num_classes == V


def _check(lex, begin=None, tok=None, child=None, term=None, nv=None, depth=None, n_nodes=None, n_edges=None):
    arrs = [np.ascontiguousarray(x if x is not None else d) for x, d in
            ((begin, lex.edge_begin), (tok, lex.edge_tok), (child, lex.edge_child), (term, lex.terminal))]
    return nat.lib().msocr_lexicon_check_host(*(a.ctypes.data for a in arrs), lex.n_nodes if n_nodes is None else n_nodes,
                                              lex.n_edges if n_edges is None else n_edges, V if nv is None else nv,
                                              MAX_LEN - 1 if depth is None else depth)


def test_check_host_accepts_the_trie_and_refuses_single_corruptions(lex):
    assert _check(lex) == 0
    node = int(np.flatnonzero(np.diff(lex.edge_begin) >= 2)[3])  # a node with two children or more, not the root
    lo = int(lex.edge_begin[node])
    c = lambda a: a.copy()
    b = c(lex.edge_begin); b[node + 1] = b[node] - 1
    assert _check(lex, begin=b) == E_ARG, "non-monotone begin"
    b = c(lex.edge_begin); b[0] = 1
    assert _check(lex, begin=b) == E_ARG, "begin[0] != 0"
    b = c(lex.edge_begin); b[-1] -= 1
    assert _check(lex, begin=b) == E_ARG, "begin[n_nodes] != n_edges"
    t = c(lex.edge_tok); t[lo], t[lo + 1] = t[lo + 1], t[lo]
    assert _check(lex, tok=t) == E_ARG, "unsorted tokens"
    t = c(lex.edge_tok); t[lo + 1] = t[lo]
    assert _check(lex, tok=t) == E_ARG, "equal tokens"
    t = c(lex.edge_tok); t[lo + 1] = V
    assert _check(lex, tok=t) == E_ARG, "token >= V"
    assert _check(lex, nv=int(lex.edge_tok.max())) == E_ARG, "token >= V (smaller V)"
    t = c(lex.edge_tok); t[lo] = -1
    assert _check(lex, tok=t) == E_ARG, "negative token"
    ch = c(lex.edge_child); ch[lo] = node
    assert _check(lex, child=ch) == E_ARG, "child == parent"
    ch = c(lex.edge_child); ch[lo] = node - 1
    assert _check(lex, child=ch) == E_ARG, "child < parent"
    ch = c(lex.edge_child); ch[lo] = lex.n_nodes
    assert _check(lex, child=ch) == E_ARG, "child >= n_nodes"
    ch = c(lex.edge_child); ch[lo] = ch[lo + 1]
    assert _check(lex, child=ch) == E_ARG, "two parents, and a node with none"
    leaf = int(np.flatnonzero(np.diff(lex.edge_begin) == 0)[0])
    z = c(lex.terminal); z[leaf] = 0
    assert _check(lex, term=z) == E_ARG, "non-terminal leaf"
    assert _check(lex, depth=MAX_LEN - 2) == E_ARG, "depth over the limit"  # "abcdefgh" has MAX_LEN - 1 symbols
    assert _check(lex, depth=MAX_LEN - 1) == 0
    assert _check(lex, n_nodes=0) == E_ARG and _check(lex, n_edges=-1) == E_ARG
    L = nat.lib()
    p = [a.ctypes.data for a in (lex.edge_begin, lex.edge_tok, lex.edge_child, lex.terminal)]
    for k in range(4):
        q = list(p)
        q[k] = None
        assert L.msocr_lexicon_check_host(*q, lex.n_nodes, lex.n_edges, V, MAX_LEN) == E_ARG, k
    # an interior terminal node switched off is still a valid (other) lexicon: the validator checks structure, not content
    inner = int(np.flatnonzero((np.diff(lex.edge_begin) > 0) & (lex.terminal[:] == 1))[0])
    z = c(lex.terminal); z[inner] = 0
    assert _check(lex, term=z) == 0


def test_new_symbols_are_bound():
    L = nat.lib()
    for name in ("msocr_attn_beam_slots_bytes", "msocr_attn_decode", "msocr_lexicon_check_host"):
        assert name in nat.exported_symbols() and hasattr(L, name)
    assert L.msocr_attn_beam_slots_bytes(37, 9, 8) == 37 * 9 * 8 * 4
    assert L.msocr_attn_beam_slots_bytes(0, 9, 8) == 0 and L.msocr_attn_beam_slots_bytes(3, 9, 0) == 0
    assert ctypes_sizeof_lexicon() == 4 * 8 + 2 * 4
    hdr = open(__file__.replace("tests/test_lexicon_cpu.py", "include/msocr.h"), encoding="utf-8").read()
    for name in ("msocr_lexicon;", "msocr_attn_decode(", "msocr_lexicon_check_host(", "msocr_attn_beam_slots_bytes("):
        assert name in hdr, name


def ctypes_sizeof_lexicon():
    import ctypes
    return ctypes.sizeof(nat.LexiconArrays)
