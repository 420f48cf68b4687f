"""Lexicon: a closed vocabulary as a prefix tree (trie) the beam decode is constrained to.

The host class encodes the words with the recogniser's charset (transforms.encode_text, the rule pack_targets packs a forced-decode
target by), builds the trie as CSR arrays in breadth-first node order, has them checked once by msocr_lexicon_check_host and uploads
them per device.  The kernels (csrc/attn_general_lexicon.hip, csrc/attn_lexicon_mfma.hip) read edge_begin / edge_tok / edge_child /
terminal; word_of_node stays on the host and turns a decoded word back into its index.  No minimisation to a DAWG: a node stands for
one prefix, which is what word_of_node relies on.
"""
import ctypes

import numpy as np

from ... import _native as nat
from .transforms import encode_text


class Lexicon:
    """Lexicon(words, charset, max_len, *, strict=True)

    words: an iterable of str, the forms to admit exactly as they are to be read (the detector's "words" carry their punctuation: a
    lexicon of bare word forms forbids "слово," — supply the forms you want).  charset: the recogniser's token table, as its `stoi`
    dict or its `itos` list (TRBA.stoi / TRBA.itos).  max_len: the recogniser's max_len, i.e. the steps of its beam decode; a word
    needs its EOS inside them, so it may have at most max_len - 1 symbols.
    strict=True: a character outside the charset, <BLANK>'s character, an empty word or a word that is too long raises ValueError
    naming the word; strict=False drops such words.  Duplicates collapse to their first occurrence; `words` is the deduplicated list
    and every index this class returns points into it.  An empty result is a ValueError.

    Arrays (numpy, host): edge_begin [n_nodes + 1] i32, edge_tok [n_edges] i32 (strictly ascending inside a node), edge_child
    [n_edges] i32, terminal [n_nodes] u8, word_of_node [n_nodes] i32 (-1 where no word ends).  Nodes are numbered breadth-first: the
    root is node 0 and child > parent.
    Building 100 000 random words of mean length 8 over 58 symbols (582 000 nodes) took 1.7 s of plain Python / NumPy on one core of
    the development machine's CPU, of which the validator took 4 ms."""

    def __init__(self, words, charset, max_len, *, strict=True):
        stoi = charset if isinstance(charset, dict) else {s: i for i, s in enumerate(charset)}
        for name in ("<PAD>", "<SOS>", "<EOS>"):
            if name not in stoi:
                raise ValueError(f"the charset has no {name} token")
        self.num_classes = max(stoi.values()) + 1
        self.max_len = int(max_len)
        self.eos_id = stoi["<EOS>"]
        if self.max_len < 2:
            raise ValueError(f"max_len must be at least 2 (one symbol and its EOS), got {max_len}")
        seen, kept_words, encoded = {}, [], []
        for w in words:
            if not isinstance(w, str):
                raise TypeError(f"lexicon words must be str, got {type(w).__name__}")
            ids, _kept, rejected = encode_text(w, stoi)
            why = None
            if rejected:
                why = f"character {rejected[0][0]!r} is {rejected[0][1]}"
            elif not ids:
                why = "the word is empty"
            elif len(ids) > self.max_len - 1:
                why = f"{len(ids)} symbols, at most max_len - 1 = {self.max_len - 1} fit beside the EOS"
            if why is not None:
                if strict:
                    raise ValueError(f"lexicon word {w!r}: {why}")
                continue
            key = tuple(ids)
            if key not in seen:
                seen[key] = len(kept_words)
                kept_words.append(w)
                encoded.append(key)
        if not kept_words:
            raise ValueError("the lexicon is empty")
        self.words = kept_words
        self._build(encoded)
        rc = nat.lib().msocr_lexicon_check_host(self.edge_begin.ctypes.data, self.edge_tok.ctypes.data, self.edge_child.ctypes.data,
                                                self.terminal.ctypes.data, self.n_nodes, self.n_edges, self.num_classes, self.max_len - 1)
        if rc != 0:
            raise RuntimeError(f"msocr_lexicon_check_host refused the trie this class built (code {rc})")
        self._device = {}

    def _build(self, encoded):
        # insertion-order trie as a list of dicts, then a breadth-first renumbering with every node's edges sorted by token
        children, word_at = [{}], [-1]
        for wi, ids in enumerate(encoded):
            n = 0
            for t in ids:
                d = children[n]
                m = d.get(t)
                if m is None:
                    m = d[t] = len(children)
                    children.append({})
                    word_at.append(-1)
                n = m
            word_at[n] = wi
        n_nodes = len(children)
        order = [0]  # old ids in breadth-first order; position = new id
        begin = np.zeros(n_nodes + 1, dtype=np.int32)
        tok, child = [], []
        for new, old in enumerate(order):  # `order` grows while it is walked
            for t in sorted(children[old]):
                tok.append(t)
                child.append(len(order))
                order.append(children[old][t])
            begin[new + 1] = len(tok)
        order = np.asarray(order, dtype=np.int64)
        self.n_nodes, self.n_edges = n_nodes, len(tok)
        self.edge_begin = begin
        self.edge_tok = np.asarray(tok, dtype=np.int32)
        self.edge_child = np.asarray(child, dtype=np.int32)
        self.word_of_node = np.asarray(word_at, dtype=np.int32)[order]
        self.terminal = (self.word_of_node >= 0).astype(np.uint8)

    def __len__(self):
        return len(self.words)

    def walk(self, node, token):
        """The child of `node` along `token`, or -1 (also for node -1): the kernels' child lookup on the host."""
        if node < 0:
            return -1
        lo, hi = int(self.edge_begin[node]), int(self.edge_begin[node + 1])
        k = lo + int(np.searchsorted(self.edge_tok[lo:hi], token))
        return int(self.edge_child[k]) if k < hi and self.edge_tok[k] == token else -1

    def find(self, ids):
        """The index (into `words`) of the word whose token ids are `ids` up to the first EOS or -1, or -1 if it is no lexicon word."""
        node = 0
        for t in ids:
            t = int(t)
            if t == self.eos_id or t == -1:
                break
            node = self.walk(node, t)
            if node < 0:
                return -1
        return int(self.word_of_node[node])

    def to(self, device):
        """The four device arrays as tensors on `device` and the msocr_lexicon struct that points at them, cached per device:
        (edge_begin, edge_tok, edge_child, terminal, struct)."""
        import torch
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if dev not in self._device:
            # edge arrays of a one-node trie cannot occur (the lexicon is not empty); empty tensors would have no address
            ts = tuple(torch.from_numpy(a).to(dev) for a in (self.edge_begin, self.edge_tok, self.edge_child, self.terminal))
            la = nat.LexiconArrays()
            la.edge_begin, la.edge_tok, la.edge_child, la.terminal = (t.data_ptr() for t in ts)
            la.n_nodes, la.n_edges = self.n_nodes, self.n_edges
            self._device[dev] = ts + (la,)
        return self._device[dev]

    def struct(self, device):
        return ctypes.byref(self.to(device)[4])
