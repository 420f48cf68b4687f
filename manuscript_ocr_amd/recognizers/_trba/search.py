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
        if device is not None:
            import torch
            self.device = torch.device(device)
            self.tokens = torch.from_numpy(tok).to(self.device)

    def __len__(self):
        return len(self.offsets) - 1

    def search(self, patterns: Sequence[str], max_distance: Union[None, int, Sequence[int]] = None,
               max_error_rate: Optional[float] = None, overlapping: bool = False) -> List[TextHit]:
        """Every place where a pattern occurs in a text within its bound.  overlapping=False: the occurrences, i.e. per (pattern,
        text) the hits that remain when they are taken best first ((distance, end) ascending) and one that intersects a taken one
        is dropped; overlapping=True: every end position within the bound (a match of distance 0 inside a bound of 2 is then
        reported at up to five ends).  A pattern character the corpus does not hold matches nothing."""
        patterns = list(patterns)
        for p in patterns:
            if not isinstance(p, str):
                raise TypeError(f"a pattern is a str, got {type(p).__name__}")
        ks = pattern_bounds([len(p) for p in patterns], max_distance, max_error_rate)
        pat_off = np.concatenate([[0], np.cumsum([len(p) for p in patterns])]).astype(np.int32)
        pat_tok = np.array([self.stoi.get(ch, -1) for p in patterns for ch in p], dtype=np.int32)
        if self.device is None:
            hits, _count = ops.text_search_host(pat_tok, pat_off, ks, self.tokens, self.offsets, self.v)
        else:
            import torch
            with torch.cuda.device(self.device):
                hits = ops.text_search(torch.from_numpy(pat_tok).to(self.device), pat_off, ks, self.tokens, self.offsets, self.v)
        if overlapping:
            hits = hits[np.lexsort((hits[:, 3], hits[:, 1], hits[:, 0]))] if len(hits) else hits
        else:
            hits = ops.text_search_select(hits)
        return [TextHit(*row) for row in hits.tolist()]


def search_texts(patterns, texts, max_distance=None, max_error_rate=None, overlapping=False, device=None) -> List[TextHit]:
    """TextCorpus(texts, device).search(patterns, ...) in one call."""
    return TextCorpus(texts, device=device).search(patterns, max_distance=max_distance, max_error_rate=max_error_rate,
                                                   overlapping=overlapping)
