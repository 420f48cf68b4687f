"""Result objects exchanged across the plugin boundary.

Field names, optionality and the [0, 1] range checks are those of the reference DTOs
(/root/reference/src/manuscript/detectors/_types.py:5-33) so that code written against
`manuscript.detectors._types` keeps working; everything else here is this package's own.
"""
from typing import List, Optional, Tuple

from pydantic import BaseModel, ConfigDict, Field

_UNIT = dict(ge=0.0, le=1.0)


class Word(BaseModel):
    """One detected word: outline in page pixels, detector score, and (after recognition) its transcription."""

    polygon: List[Tuple[float, float]] = Field(..., description="(x, y) vertices of the word outline, page pixel coordinates")
    detection_confidence: float = Field(..., description="EAST score of the kept quad", **_UNIT)
    text: Optional[str] = Field(None, description="transcription written by Pipeline; None until recognised")
    recognition_confidence: Optional[float] = Field(None, description="mean per-step token probability from the recogniser", **_UNIT)


class Char(BaseModel):
    """One recognised symbol of a word (this package's extension; the reference has no symbol-level output)."""

    char: str = Field(..., description="the symbol, one charset token")
    confidence: float = Field(..., description="probability the recogniser gave the token at its decode step", **_UNIT)
    x: float = Field(..., description="estimated horizontal centre in pixels of the image the word came from (attention centroid)")


class CharWord(Word):
    """A Word with its symbols, written by Pipeline when `char_details` is on.  Block.words is declared as List[Word], so a
    default model_dump() of a Page serialises a CharWord as a Word: dumps do not change with the flag."""

    chars: List[Char] = Field(default_factory=list, description="one entry per symbol of `text`, in order")


class Alternative(BaseModel):
    """One reading of a word from the recogniser's beam search (this package's extension; the reference returns one per word)."""

    text: str = Field(..., description="the hypothesis's transcription")
    confidence: float = Field(..., description="mean per-step token probability along the hypothesis, as recognition_confidence", **_UNIT)
    logp: float = Field(..., description="summed log-probability of the hypothesis's tokens up to its EOS: the score the search ranks by")


class AltWord(CharWord):
    """A Word with the beam search's best final readings, written by Pipeline when `n_best` is on: alternatives[0] is the word's own
    text and confidence, the others follow in the search's order.  `chars` stays empty unless `char_details` is also on, and
    describes the best reading only.  As for CharWord, a default model_dump() of a Page does not change with the switch."""

    alternatives: List[Alternative] = Field(default_factory=list, description="distinct readings, best first")


class LexAlternative(Alternative):
    """An Alternative of a lexicon-constrained decode: a lexicon word, with its index."""

    lexicon_index: int = Field(..., description="index of `text` in Lexicon.words")


class LexWord(AltWord):
    """A Word read under a lexicon, written by Pipeline when `lexicon` is set: `text` is a lexicon word and `lexicon_index` its index
    in Lexicon.words (-1 only where the decoder's logits were not finite).  `alternatives` (LexAlternatives, lexicon words only) are
    filled when `n_best` is also on, `chars` when `char_details` is.  As for CharWord, a default model_dump() of a Page does not change."""

    lexicon_index: int = Field(..., description="index of `text` in Lexicon.words, -1 if it is none")


class LmAlternative(Alternative):
    """An Alternative of a decode fused with a character language model, with the language model's own score of it."""

    lm_logp: float = Field(..., description="unweighted language-model log-probability of `text`, its EOS included")


class LmWord(AltWord):
    """A Word read under a character language model, written by Pipeline when `lm` is set: `lm_logp` is the language model's
    unweighted log-probability of `text`; `recognition_confidence` stays the recogniser's own.  `alternatives` (LmAlternatives, in
    fused-score order) are filled when `n_best` is also on, `chars` when `char_details` is.  As for CharWord, a default model_dump()
    of a Page does not change."""

    lm_logp: float = Field(..., description="unweighted language-model log-probability of `text`, its EOS included")


class Suggestion(BaseModel):
    """One lexicon word near a recognised word (this package's extension): approximate dictionary lookup on the decoded text."""

    text: str = Field(..., description="the lexicon word")
    lexicon_index: int = Field(..., description="index of `text` in Lexicon.words")
    distance: int = Field(..., description="Levenshtein distance (unit costs) between the recognised text and `text`", ge=0)


class SuggestWord(AltWord):
    """A Word with the lexicon words nearest to its text, written by Pipeline when `suggest` is set: nearest first, equal distances
    by ascending lexicon index; distance 0 means `text` is a lexicon word, an empty list that nothing lies within the bound.  The
    decode is the open one: `text` is the recogniser's own reading.  `alternatives` are filled when `n_best` is also on, `chars` when
    `char_details` is.  As for CharWord, a default model_dump() of a Page does not change."""

    suggestions: List[Suggestion] = Field(default_factory=list, description="nearest lexicon words, nearest first")


class SuggestLmWord(LmWord):
    """A SuggestWord of a decode fused with a character language model (`suggest` and `lm` both set): an LmWord with `suggestions`."""

    suggestions: List[Suggestion] = Field(default_factory=list, description="nearest lexicon words, nearest first")


class TransferWord(AltWord):
    """A recognised Word with the transcription word that Pipeline.transfer_text aligned to it (this package's extension): the
    page's words in reading order against the words of a plain transcription, by the alignment of msocr_edit_alignment.  A word
    paired as a hit or a substitution carries the three fields; a word the alignment left without a partner (or un-paired by
    `max_cer`) has None in all three.  The word keeps every field of the class it came as (`chars`, `alternatives`, and, as extra
    fields, `lexicon_index`, `lm_logp` or `suggestions` where it had them).  As for CharWord, a default model_dump() of a Page does
    not change."""

    model_config = ConfigDict(extra="allow")

    gt_text: Optional[str] = Field(None, description="the transcription word paired with this word, None if it has none")
    gt_index: Optional[int] = Field(None, description="index of `gt_text` in the transcription's str.split()", ge=0)
    char_distance: Optional[int] = Field(None, description="Levenshtein distance (unit costs) between `text` and `gt_text`", ge=0)


class SearchHit(BaseModel):
    """One occurrence of a query in the running text of a page (this package's extension: PageCorpus.search, Pipeline.search).  A
    page's text is the texts of its words that have one, in reading order, joined by one space; `start` and `end` count its
    characters, and `words` are the words whose characters the match touches (a separator alone counts for no word)."""

    page: int = Field(..., description="index of the page in the corpus", ge=0)
    query: int = Field(..., description="index of the query in the call", ge=0)
    query_text: str = Field(..., description="the query as it was searched, whitespace-normalised")
    matched_text: str = Field(..., description="the page's text from `start` to `end`")
    distance: int = Field(..., description="Levenshtein distance (unit costs) between `query_text` and `matched_text`", ge=0)
    start: int = Field(..., description="first character of the match in the page's text", ge=0)
    end: int = Field(..., description="one past its last character", ge=0)
    words: List[Tuple[int, int]] = Field(default_factory=list, description="(block index, word index) of the words the match touches, in order")


class SpotHit(BaseModel):
    """One neighbour of a query word in a WordIndex (this package's extension: WordIndex.spot, Pipeline.spot).  The hits of one query
    come in ascending `distance`, equal distances by the order the words entered the index; `rank` counts them from 0."""

    query: int = Field(..., description="index of the query in the call", ge=0)
    page: int = Field(..., description="index of the page the word was added with", ge=0)
    block: int = Field(..., description="index of the word's block on its page", ge=0)
    word: int = Field(..., description="index of the word in its block", ge=0)
    distance: float = Field(..., description="DTW distance between the unit frames of query and word, divided by the sum of their lengths")
    rank: int = Field(..., description="0 for the nearest word of this query", ge=0)
    text: Optional[str] = Field(None, description="the indexed word's text, if it has one")


class PartSpotHit(SpotHit):
    """A SpotHit of a partial search (WordIndex.spot(..., partial=True)): the query was matched against a stretch of the word's
    frames (msocr_dtw_subsequence), and the hit says which.  Nothing constrains the stretch's length: a query may collapse onto one
    frame of the word."""

    distance: float = Field(..., description="subsequence DTW distance: the cost of the best path from the query's first frame to its "
                                             "last, starting and ending anywhere in the word, divided by the QUERY's length")
    frame_start: int = Field(..., description="first frame of the word the query was matched to", ge=0)
    frame_end: int = Field(..., description="one past the last such frame", ge=1)
    fraction: Tuple[float, float] = Field(..., description="(frame_start / L, frame_end / L) for the word's L frames: where along "
                                                           "the word the match lies")


class Block(BaseModel):
    """A group of words; the detector emits exactly one block per page."""

    words: List[Word]


class TextLine(Block):
    """One text line of a page in reading order, written by Pipeline when `group_lines` is on (this package's extension).
    Page.blocks is declared as List[Block], so a default model_dump() of a Page serialises a TextLine as a Block."""

    bbox: Tuple[int, int, int, int] = Field(..., description="(x_min, y_min, x_max, y_max): union of the words' integer boxes "
                                                             "as the reading order sees them (np.array(polygon, int32) truncation)")


class Region(Block):
    """One region of a page in reading order (a column, a heading, a paragraph cut off by wide empty bands), written by Pipeline
    when `columns` is on (this package's extension): its words in reading order.  As for TextLine, a default model_dump() of a Page
    serialises a Region as a Block."""

    bbox: Tuple[int, int, int, int] = Field(..., description="(x_min, y_min, x_max, y_max): union of the words' integer boxes")
    index: int = Field(..., description="0-based index of the region in the page's reading order", ge=0)


class RegionLine(TextLine):
    """A TextLine with the region it lies in, written by Pipeline when `columns` and `group_lines` are both on.  A line never spans
    two regions, and the lines come region by region."""

    region: int = Field(..., description="0-based index of the line's region in the page's reading order", ge=0)


class Page(BaseModel):
    """All blocks of one page image."""

    blocks: List[Block]


class SkewPage(Page):
    """A Page whose reading order and text lines were computed in the deskewed frame, written by Pipeline when `deskew` is on (this
    package's extension).  The words, their polygons and the TextLine boxes stay in page coordinates.  Declared where a Page is
    expected (List[Page], a field of type Page), a default model_dump() serialises it as a Page."""

    skew_deg: float = Field(0.0, description="estimated skew of the page's text lines in degrees, positive = lines descend to the right "
                                             "(y points down); 0.0 where no rotation was applied")
