"""Approximate search over recognised pages (this package's extension): PageCorpus turns Pages into a
recognizers.TextCorpus of their running texts and maps every hit back to the words it touches.  Searching needs neither the
networks nor a GPU: device None runs the host twin, a device runs msocr_text_search there, bit for bit the same."""
from bisect import bisect_right
from typing import List, Optional, Sequence, Union

from .detectors._types import Page, SearchHit
from .recognizers._trba.search import TextCorpus


class PageCorpus:
    """pages: Pages as Pipeline.predict returns them.  A page's text is the texts of its words that have one, in the order
    Pipeline.evaluate_text flattens them (block by block, word by word), joined by one space.  With a device the corpus is
    uploaded once and stays there for every later `search`."""

    def __init__(self, pages: Sequence[Page], device=None):
        self.texts: List[str] = []
        self._starts: List[List[int]] = []   # per page: the first character of every word that has a text, ascending
        self._ends: List[List[int]] = []     # ... and one past its last
        self._where: List[List[tuple]] = []  # ... and its (block index, word index)
        for page in pages:
            parts, starts, ends, where, at = [], [], [], [], 0
            for b, block in enumerate(page.blocks):
                for w, word in enumerate(block.words):
                    if word.text:
                        starts.append(at)
                        ends.append(at + len(word.text))
                        where.append((b, w))
                        parts.append(word.text)
                        at += len(word.text) + 1
            self.texts.append(" ".join(parts))
            self._starts.append(starts)
            self._ends.append(ends)
            self._where.append(where)
        self.corpus = TextCorpus(self.texts, device=device)

    def __len__(self):
        return len(self.texts)

    def words_of(self, page: int, start: int, end: int) -> List[tuple]:
        """(block index, word index) of the words of `page` whose characters intersect [start, end) of its text"""
        starts, ends = self._starts[page], self._ends[page]
        k = bisect_right(ends, start)  # the first word that ends behind `start`
        out = []
        while k < len(starts) and starts[k] < end:
            out.append(self._where[page][k])
            k += 1
        return out

    def search(self, queries: Sequence[str], max_distance: Union[None, int, Sequence[int]] = None,
               max_error_rate: Optional[float] = None, overlapping: bool = False, costs=None) -> List[SearchHit]:
        """Occurrences of the queries in the pages, in canonical order (query, page, end).  A query is whitespace-normalised as the
        pages' texts are (" ".join(q.split())), so it may span words, lines and blocks.  The bounds, `overlapping` and `costs` (an
        EditCosts: bounds and distances in cost units; the space between words costs `unknown` to add or drop unless the charset
        holds it): as for recognizers.TextCorpus.search."""
        queries = [" ".join(q.split()) for q in queries]
        out = []
        for h in self.corpus.search(queries, max_distance=max_distance, max_error_rate=max_error_rate, overlapping=overlapping,
                                    costs=costs):
            out.append(SearchHit(page=h.text, query=h.pattern, query_text=queries[h.pattern], matched_text=self.texts[h.text][h.start:h.end],
                                 distance=h.distance, start=h.start, end=h.end, words=self.words_of(h.text, h.start, h.end)))
        return out
