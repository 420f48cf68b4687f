"""Approximate search of short patterns in a corpus of texts (this package's extension; include/msocr.h, "approximate text search";
DESIGN.md section 4.24): where does a name occur in ten thousand recognised pages, given that the recogniser may have read a
character wrong, dropped one or added one?

  TextCorpus(texts, device=None)      encodes the texts once; with a device the tokens stay there, uploaded once, searched many times
  TextCorpus.search(patterns, ...)    -> [TextHit(pattern, text, start, end, distance)] in canonical order (pattern, text, end)
  search_texts(patterns, texts, ...)  the one-shot form

A hit says: texts[text][start:end] is within `distance` edits (unit costs) of patterns[pattern], `distance` being the least any
substring ending at `end` attains and [start, end) the shortest substring that attains it.  Characters compare by equality: case
folding and Unicode normalisation are the caller's, on both sides.  device None: the host twin msocr_text_search_host (no GPU
needed); a device: msocr_text_search there.  The two routes agree bit for bit.

With costs=EditCosts(...) the search runs under confusion-weighted costs (msocr_text_search_weighted and its host twin; DESIGN.md
section 4.27): the text is the recognised side and the pattern the true word, bounds and distances are in cost units, and many cheap
confusions are accepted where one implausible edit is not.  With costs=None every route runs the unit-cost code.
"""
from typing import List, NamedTuple, Optional, Sequence, Union

import numpy as np

from ... import ops


class TextHit(NamedTuple):
    pattern: int   # index into the patterns of the call
    text: int      # index into the corpus
    start: int     # texts[text][start:end] is the match
    end: int
    distance: int  # edits between the pattern and the match


def pattern_bounds(lengths, max_distance=None, max_error_rate=None):
    """The error bound k of every pattern from exactly one of max_distance (an int, or one per pattern) and max_error_rate
    (k = min(floor(rate * m), m - 1)); ValueError for a length outside 1..64 and a bound outside [0, m)."""
    if (max_distance is None) == (max_error_rate is None):
        raise ValueError("give exactly one of max_distance and max_error_rate")
    lengths = [int(m) for m in lengths]
    for q, m in enumerate(lengths):
        if m < 1 or m > ops.SEARCH_MAX_PATTERN:
            raise ValueError(f"pattern {q} has {m} characters; a pattern has 1 to {ops.SEARCH_MAX_PATTERN}")
    if max_error_rate is not None:
        rate = float(max_error_rate)
        if not rate >= 0.0:
            raise ValueError("max_error_rate >= 0")
        return [min(int(np.floor(rate * m)), m - 1) for m in lengths]
    if isinstance(max_distance, (int, np.integer)):
        ks = [int(max_distance)] * len(lengths)
    else:
        ks = [int(k) for k in max_distance]
        if len(ks) != len(lengths):
            raise ValueError(f"{len(ks)} bounds for {len(lengths)} patterns")
    for q, (k, m) in enumerate(zip(ks, lengths)):
        if k < 0 or k >= m:
            raise ValueError(f"pattern {q} has {m} characters: its bound {k} lies outside [0, {m})")
    return ks


def weighted_bounds(lengths, sums, dmin, max_distance=None, max_error_rate=None):
    """`pattern_bounds` in cost units: sums[q] = what it costs to supply all of pattern q (the sum of its insert costs), the bound lies
    in [0, sums[q]) and max_error_rate gives k = min(floor(rate * sums[q]), sums[q] - 1); ValueError also where the window
    m + k // dmin of a pattern exceeds ops.SEARCH_W_MAX_WINDOW (dmin: the cheapest delete)."""
    if (max_distance is None) == (max_error_rate is None):
        raise ValueError("give exactly one of max_distance and max_error_rate")
    lengths, sums = [int(m) for m in lengths], [int(s) for s in sums]
    for q, m in enumerate(lengths):
        if m < 1 or m > ops.SEARCH_MAX_PATTERN:
            raise ValueError(f"pattern {q} has {m} characters; a pattern has 1 to {ops.SEARCH_MAX_PATTERN}")
    if max_error_rate is not None:
        rate = float(max_error_rate)
        if not rate >= 0.0:
            raise ValueError("max_error_rate >= 0")
        ks = [min(int(np.floor(rate * s)), s - 1) for s in sums]
    elif isinstance(max_distance, (int, np.integer)):
        ks = [int(max_distance)] * len(lengths)
    else:
        ks = [int(k) for k in max_distance]
        if len(ks) != len(lengths):
            raise ValueError(f"{len(ks)} bounds for {len(lengths)} patterns")
    for q, (k, m, s) in enumerate(zip(ks, lengths, sums)):
        if k < 0 or k >= s:
            raise ValueError(f"pattern {q} costs {s} to supply in full: its bound {k} lies outside [0, {s})")
        if m + k // dmin > ops.SEARCH_W_MAX_WINDOW:
            raise ValueError(f"pattern {q}: {m} characters and a bound of {k} at a cheapest delete of {dmin} span {m + k // dmin} "
                             f"characters of text; at most {ops.SEARCH_W_MAX_WINDOW} are scanned")
    return ks


class TextCorpus:
    def __init__(self, texts: Sequence[str], device=None):
        texts = list(texts)
        for t in texts:
            if not isinstance(t, str):
                raise TypeError(f"a text is a str, got {type(t).__name__}")
        total = sum(len(t) for t in texts)
        if total > 2**31 - 1:
            raise ValueError(f"{total} characters: a corpus holds at most 2^31 - 1")
        off = np.concatenate([[0], np.cumsum([len(t) for t in texts], dtype=np.int64)]).astype(np.int32)
        code = np.frombuffer("".join(texts).encode("utf-32-le", "surrogatepass"), dtype="<u4")  # one code point per character
        chars, first, inverse = np.unique(code, return_index=True, return_inverse=True)
        order = np.argsort(first, kind="stable")  # the distinct characters are numbered by first occurrence
        rank = np.empty(len(chars), dtype=np.int32)
        rank[order] = np.arange(len(chars), dtype=np.int32)
        tok = rank[inverse.reshape(-1)] if total else np.zeros(0, dtype=np.int32)
        self.stoi = {chr(int(c)): k for k, c in enumerate(chars[order].tolist())}
        if len(self.stoi) > ops.SEARCH_MAX_ALPHABET:
            raise ValueError(f"{len(self.stoi)} distinct characters: a corpus holds at most {ops.SEARCH_MAX_ALPHABET}")
        self.v = max(len(self.stoi), 1)
        self.offsets = off
        self.device = None
        self.tokens = tok
        self._classes = {}  # EditCosts -> the cost class of every corpus character (on the corpus' device), -1 outside its charset
        if device is not None:
            import torch
            self.device = torch.device(device)
            self.tokens = torch.from_numpy(tok).to(self.device)

    def __len__(self):
        return len(self.offsets) - 1

    def search(self, patterns: Sequence[str], max_distance: Union[None, int, Sequence[int]] = None,
               max_error_rate: Optional[float] = None, overlapping: bool = False, costs=None) -> List[TextHit]:
        """Every place where a pattern occurs in a text within its bound.  overlapping=False: the occurrences, i.e. per (pattern,
        text) the hits that remain when they are taken best first ((distance, end) ascending) and one that intersects a taken one
        is dropped; overlapping=True: every end position within the bound (a match of distance 0 inside a bound of 2 is then
        reported at up to five ends).  A pattern character the corpus does not hold matches nothing.

        costs (a recognizers.EditCosts): the confusion-weighted search.  The text is what was read, the pattern the true word:
        costs.sub[t, p] prices reading text character t as pattern character p, costs.delete[t] dropping t, costs.insert[p]
        supplying p; equal characters match at 0 whether or not the charset holds them, and any other edit of a character outside
        the charset, or of a pattern character the corpus does not hold, costs costs.unknown.  max_distance is then in cost units
        and lies below what the pattern costs to supply in full (the sum of its insert costs, S); max_error_rate gives
        k = min(floor(rate * S), S - 1); `distance` is in cost units.  ValueError where the corpus has more than
        ops.SEARCH_W_MAX_ALPHABET distinct characters or a pattern's window len + k // min(costs.min_del, costs.unknown) exceeds
        ops.SEARCH_W_MAX_WINDOW."""
        patterns = list(patterns)
        for p in patterns:
            if not isinstance(p, str):
                raise TypeError(f"a pattern is a str, got {type(p).__name__}")
        pat_off = np.concatenate([[0], np.cumsum([len(p) for p in patterns])]).astype(np.int32)
        pat_tok = np.array([self.stoi.get(ch, -1) for p in patterns for ch in p], dtype=np.int32)
        if costs is not None:
            hits = self._search_weighted(patterns, pat_tok, pat_off, max_distance, max_error_rate, costs)
        else:
            hits = self._search_unit(patterns, pat_tok, pat_off, max_distance, max_error_rate)
        if overlapping:
            hits = hits[np.lexsort((hits[:, 3], hits[:, 1], hits[:, 0]))] if len(hits) else hits
        else:
            hits = ops.text_search_select(hits)
        return [TextHit(*row) for row in hits.tolist()]

    def _search_unit(self, patterns, pat_tok, pat_off, max_distance, max_error_rate):
        ks = pattern_bounds([len(p) for p in patterns], max_distance, max_error_rate)
        if self.device is None:
            hits, _count = ops.text_search_host(pat_tok, pat_off, ks, self.tokens, self.offsets, self.v)
        else:
            import torch
            with torch.cuda.device(self.device):
                hits = ops.text_search(torch.from_numpy(pat_tok).to(self.device), pat_off, ks, self.tokens, self.offsets, self.v)
        return hits

    def token_classes(self, costs):
        """(host, on the corpus' device) int32 [v]: the class in costs' charset of every corpus character, -1 outside it; cached"""
        if costs not in self._classes:
            cls = np.full(self.v, -1, dtype=np.int32)
            for ch, k in self.stoi.items():
                cls[k] = costs.stoi.get(ch, -1)
            dev = cls
            if self.device is not None:
                import torch
                dev = torch.from_numpy(cls).to(self.device)
            self._classes[costs] = (cls, dev)
        return self._classes[costs]

    def _search_weighted(self, patterns, pat_tok, pat_off, max_distance, max_error_rate, costs):
        from .edit_costs import EditCosts
        if not isinstance(costs, EditCosts):
            raise TypeError(f"costs must be an EditCosts, got {type(costs).__name__}")
        if len(self.stoi) > ops.SEARCH_W_MAX_ALPHABET:
            raise ValueError(f"{len(self.stoi)} distinct characters: the weighted search takes at most {ops.SEARCH_W_MAX_ALPHABET}")
        cls, cls_dev = self.token_classes(costs)
        pat_cls = np.where(pat_tok >= 0, cls[np.maximum(pat_tok, 0)], -1)
        w_ins = np.where(pat_cls >= 0, costs.insert[np.maximum(pat_cls, 0)].astype(np.int64), costs.unknown)
        sums = [int(w_ins[pat_off[q]:pat_off[q + 1]].sum()) for q in range(len(patterns))]
        ks = weighted_bounds([len(p) for p in patterns], sums, min(costs.min_del, costs.unknown), max_distance, max_error_rate)
        if self.device is None:
            hits, _count = ops.text_search_weighted_host(pat_tok, pat_off, ks, self.tokens, self.offsets, self.v, cls, costs)
        else:
            import torch
            with torch.cuda.device(self.device):
                hits = ops.text_search_weighted(torch.from_numpy(pat_tok).to(self.device), pat_off, ks, self.tokens, self.offsets, self.v,
                                                cls_dev, costs)
        return hits


def search_texts(patterns, texts, max_distance=None, max_error_rate=None, overlapping=False, device=None, costs=None) -> List[TextHit]:
    """TextCorpus(texts, device).search(patterns, ...) in one call."""
    return TextCorpus(texts, device=device).search(patterns, max_distance=max_distance, max_error_rate=max_error_rate,
                                                   overlapping=overlapping, costs=costs)
