"""Lexicon: a closed vocabulary as a prefix tree (trie) the beam decode is constrained to.

The host class encodes the words with the recogniser's charset (transforms.encode_text, the rule pack_targets packs a forced-decode
target by), builds the trie as CSR arrays in breadth-first node order, has them checked once by msocr_lexicon_check_host and uploads
them per device.  The kernels (csrc/attn_general_lexicon.hip, csrc/attn_lexicon_mfma.hip) read edge_begin / edge_tok / edge_child /
terminal; word_of_node stays on the host and turns a decoded word back into its index.  No minimisation to a DAWG: a node stands for
one prefix, which is what word_of_node relies on.

The encodings are also kept as a CSR word list (word_begin, word_tok) for the nearest-word lookup:
`nearest` / `nearest_texts` give, for rows of ids or strings, the k words with the smallest Levenshtein distance and the distances,
through msocr_lexicon_nearest on a device or its host twin without one; msocr_wordlist_check_host validates the list once.
With `costs=EditCosts(...)` the same calls rank by the confusion-weighted distance (msocr_lexicon_nearest_weighted, DESIGN.md section
4.26); distances and max_distance are then in cost units.
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
        self._stoi = stoi
        self.pad_id = stoi["<PAD>"]
        self.blank_id = stoi.get("<BLANK>", -1)
        # the encodings as a CSR word list beside the trie, for the nearest-word lookup: word i = words[i]
        self.word_begin = np.zeros(len(encoded) + 1, dtype=np.int32)
        np.cumsum([len(e) for e in encoded], out=self.word_begin[1:])
        self.word_tok = np.fromiter((t for e in encoded for t in e), dtype=np.int32, count=int(self.word_begin[-1]))
        self._build(encoded)
        rc = nat.lib().msocr_lexicon_check_host(self.edge_begin.ctypes.data, self.edge_tok.ctypes.data, self.edge_child.ctypes.data,
                                                self.terminal.ctypes.data, self.n_nodes, self.n_edges, self.num_classes, self.max_len - 1)
        if rc != 0:
            raise RuntimeError(f"msocr_lexicon_check_host refused the trie this class built (code {rc})")
        self._device = {}
        self._wordlist = {}
        self._wordlist_ok = False

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
        return ctypes.pointer(self.to(device)[4])  # what the field AttnDesc.lexicon takes

    # ------------------------------------------------------------------------------------- nearest words
    def _check_wordlist(self):
        """msocr_wordlist_check_host over the host arrays, once; the lookup's envelope (charset <= 512 tokens, words <= 63) on the way."""
        if self._wordlist_ok:
            return
        if self.num_classes > 512 or self.max_len - 1 > 63:
            raise ValueError(f"the nearest-word lookup takes charsets of at most 512 tokens and words of at most 63 symbols; this "
                             f"lexicon has {self.num_classes} tokens and max_len {self.max_len}")
        rc = nat.lib().msocr_wordlist_check_host(self.word_begin.ctypes.data, self.word_tok.ctypes.data, len(self.words),
                                                 len(self.word_tok), self.num_classes, self.max_len - 1)
        if rc != 0:
            raise RuntimeError(f"msocr_wordlist_check_host refused the word list this class built (code {rc})")
        self._wordlist_ok = True

    def wordlist(self, device):
        """The word list on `device` and the msocr_wordlist struct that points at it, cached per device: (word_begin, word_tok,
        struct[, by_length]).  The device copy is stored in ascending (length, index) order with by_length, the word index of every
        position, so that a wave's lanes hold words of one length in adjacent memory; results are in the original index either way.
        device None: the host arrays themselves, in the original order (for the host twin)."""
        if device is None:
            key = None
        else:
            import torch
            key = torch.device(device)
            if key.type == "cuda" and key.index is None:
                key = torch.device("cuda", torch.cuda.current_device())
        if key not in self._wordlist:
            self._check_wordlist()
            wl = nat.WordList()
            if key is None:
                ts = (self.word_begin, self.word_tok)
                wl.word_begin, wl.word_tok = self.word_begin.ctypes.data, self.word_tok.ctypes.data
            else:
                import torch
                ts = tuple(torch.from_numpy(a).to(key) for a in self.sorted_wordlist())
                wl.word_begin, wl.word_tok, wl.by_length = (t.data_ptr() for t in ts)
            wl.n_words, wl.n_tok = len(self.words), len(self.word_tok)
            self._wordlist[key] = (ts[0], ts[1], wl) + tuple(ts[2:])  # the struct third; by_length kept alive behind it
        return self._wordlist[key]

    def sorted_wordlist(self):
        """(word_begin, word_tok, by_length) of the list stored in ascending (length, index) order: position p holds word by_length[p]."""
        lens = np.diff(self.word_begin)
        by_length = np.argsort(lens, kind="stable").astype(np.int32)
        begin = np.zeros(len(lens) + 1, dtype=np.int32)
        np.cumsum(lens[by_length], out=begin[1:])
        src = np.repeat(self.word_begin[:-1][by_length] - begin[:-1], lens[by_length]) + np.arange(len(self.word_tok), dtype=np.int32)
        return begin, np.ascontiguousarray(self.word_tok[src]), by_length

    @staticmethod
    def _check_k_bound(k, max_distance):
        if not 1 <= int(k) <= 16:
            raise ValueError(f"k must be between 1 and 16, got {k}")
        if max_distance is not None and int(max_distance) < 0:
            raise ValueError(f"max_distance must not be negative, got {max_distance}")
        return int(k), -1 if max_distance is None else int(max_distance)

    def _check_costs(self, costs):
        if costs is None:
            return
        if not hasattr(costs, "struct") or not hasattr(costs, "num_classes"):
            raise TypeError(f"costs must be an EditCosts, got {type(costs).__name__}")
        if costs.num_classes != self.num_classes:
            raise ValueError(f"the costs were built for a charset of {costs.num_classes} tokens, this lexicon's has {self.num_classes}")

    def nearest_device(self, ids_dev, trun_dev, k=3, max_distance=None, costs=None):
        """msocr_lexicon_nearest (with costs: msocr_lexicon_nearest_weighted) on the current stream over ids [N, steps] / t_run [N]
        int32 tensors on one device, without any synchronisation -> (index [N, k], distance [N, k]) int32 tensors on that device."""
        import torch
        from ... import ops
        k, bound = self._check_k_bound(k, max_distance)
        self._check_costs(costs)
        N, steps = (int(v) for v in ids_dev.shape)
        if not 1 <= steps <= 64:
            raise ValueError(f"rows of 1 to 64 steps, got {steps}")
        dev = ids_dev.device
        wl = self.wordlist(dev)[2]
        index = torch.empty((N, k), dtype=torch.int32, device=dev)
        dist = torch.empty((N, k), dtype=torch.int32, device=dev)
        if N == 0:
            return index, dist
        ids_dev, trun_dev = ids_dev.contiguous(), trun_dev.contiguous()
        ws = torch.empty((max(int(nat.lib().msocr_lexicon_nearest_ws_bytes(N, len(self.words), k)), 8),), dtype=torch.uint8, device=dev)
        if costs is not None:  # the same workspace: msocr_lexicon_nearest_weighted_ws_bytes is that number
            nat.check(nat.lib().msocr_lexicon_nearest_weighted(ids_dev.data_ptr(), trun_dev.data_ptr(), N, steps, self.num_classes,
                                                               self.eos_id, self.pad_id, self.blank_id, ctypes.byref(wl), costs.struct(dev),
                                                               k, bound, index.data_ptr(), dist.data_ptr(), ws.data_ptr(), ops._stream()),
                      "lexicon_nearest_weighted")
            return index, dist
        nat.check(nat.lib().msocr_lexicon_nearest(ids_dev.data_ptr(), trun_dev.data_ptr(), N, steps, self.num_classes, self.eos_id,
                                                  self.pad_id, self.blank_id, ctypes.byref(wl), k, bound, index.data_ptr(),
                                                  dist.data_ptr(), ws.data_ptr(), ops._stream()), "lexicon_nearest")
        return index, dist

    def nearest(self, ids, t_run=None, k=3, max_distance=None, device=None, costs=None):
        """For every row of ids [N, steps] (a host array or a device tensor of token ids, steps <= 64), the k lexicon words with the
        smallest Levenshtein distance to the row's text (what TRBA.texts decodes: up to the first EOS among the first t_run ids, PAD
        and BLANK removed; t_run None = all steps) -> host arrays (index [N, k] int32 into `words`, distance [N, k] int32), nearest
        first, equal distances by ascending index.  max_distance: words further away are dropped (None = no bound); unfilled ranks
        hold -1, -1.  device None: the host twin (no GPU needed); otherwise msocr_lexicon_nearest on that device.
        costs (an EditCosts over this lexicon's charset, else ValueError): the confusion-weighted distance of DESIGN.md section 4.26
        instead, what it costs to turn the row into the word; distances and max_distance are then in cost units."""
        k, bound = self._check_k_bound(k, max_distance)
        self._check_costs(costs)
        is_tensor = hasattr(ids, "data_ptr")
        if device is None and not is_tensor:
            ids = np.ascontiguousarray(ids, dtype=np.int32)
            if ids.ndim != 2 or not 1 <= ids.shape[1] <= 64:
                raise ValueError(f"ids must be [N, steps] with 1 <= steps <= 64, got shape {ids.shape}")
            N, steps = ids.shape
            trun = np.full(N, steps, dtype=np.int32) if t_run is None else np.ascontiguousarray(t_run, dtype=np.int32)
            if trun.shape != (N,):
                raise ValueError(f"t_run must be [{N}]")
            index, dist = np.empty((N, k), dtype=np.int32), np.empty((N, k), dtype=np.int32)
            wl = self.wordlist(None)[2]
            if costs is not None:
                nat.check(nat.lib().msocr_lexicon_nearest_weighted_host(ids.ctypes.data, trun.ctypes.data, N, steps, self.num_classes,
                                                                        self.eos_id, self.pad_id, self.blank_id, ctypes.byref(wl),
                                                                        costs.struct(None), k, bound, index.ctypes.data,
                                                                        dist.ctypes.data), "lexicon_nearest_weighted_host")
                return index, dist
            nat.check(nat.lib().msocr_lexicon_nearest_host(ids.ctypes.data, trun.ctypes.data, N, steps, self.num_classes, self.eos_id,
                                                           self.pad_id, self.blank_id, ctypes.byref(wl), k, bound, index.ctypes.data,
                                                           dist.ctypes.data), "lexicon_nearest_host")
            return index, dist
        import torch
        dev = ids.device if device is None else torch.device(device)
        ids_dev = ids.to(dev, torch.int32) if is_tensor else torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int32)).to(dev)
        if ids_dev.ndim != 2:
            raise ValueError(f"ids must be [N, steps], got shape {tuple(ids_dev.shape)}")
        N, steps = ids_dev.shape
        if t_run is None:
            trun_dev = torch.full((N,), steps, dtype=torch.int32, device=dev)
        elif hasattr(t_run, "data_ptr"):
            trun_dev = t_run.to(dev, torch.int32)
        else:
            trun_dev = torch.from_numpy(np.ascontiguousarray(t_run, dtype=np.int32)).to(dev)
        if tuple(trun_dev.shape) != (N,):
            raise ValueError(f"t_run must be [{N}]")
        with torch.cuda.device(dev):
            index, dist = self.nearest_device(ids_dev, trun_dev, k, bound if bound >= 0 else None, costs)
            return index.cpu().numpy(), dist.cpu().numpy()

    def encode_rows(self, texts):
        """Strings -> (ids [N, steps] int32, t_run [N] int32) for `nearest`: encode_text's ids, except that a character outside the
        charset (or <BLANK>'s) becomes -1, an id that matches no lexicon token — an error of the reading, not of the call.  A text
        longer than 64 symbols is a ValueError."""
        rows = []
        for t in texts:
            if not isinstance(t, str):
                raise TypeError(f"texts must be str, got {type(t).__name__}")
            row = [self._stoi.get(ch, -1) for ch in t]
            row = [-1 if v in (self.blank_id, self.pad_id, self.eos_id) else v for v in row]
            if len(row) > 64:
                raise ValueError(f"text {t!r}: {len(row)} symbols, the lookup takes at most 64")
            rows.append(row)
        steps = max([len(r) for r in rows] + [1])
        ids = np.full((len(rows), steps), self.eos_id, dtype=np.int32)
        for i, r in enumerate(rows):
            ids[i, :len(r)] = r
        return ids, np.array([len(r) for r in rows], dtype=np.int32)

    def nearest_texts(self, texts, k=3, max_distance=None, device=None, costs=None):
        """`nearest` for strings (encode_rows) -> (index [N, k], distance [N, k])."""
        ids, trun = self.encode_rows(list(texts))
        return self.nearest(ids, trun, k, max_distance, device, costs)

    def suggestions(self, index, distance):
        """(index, distance) rows of `nearest` -> per row a list of {"text", "lexicon_index", "distance"}, nearest first; unfilled
        ranks are left out."""
        words = self.words
        return [[{"text": words[i], "lexicon_index": i, "distance": d} for i, d in zip(ri, rd) if i >= 0]
                for ri, rd in zip(np.asarray(index).tolist(), np.asarray(distance).tolist())]
