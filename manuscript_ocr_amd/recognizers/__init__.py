from ._trba import TRBA
from ._trba.charlm import CharLM
from ._trba.edit_costs import EditCosts
from ._trba.lexicon import Lexicon
from ._trba.metrics import (Alignment, accuracy, character_error_rate, edit_distances, error_breakdown, sequence_alignments,
                            sequence_edit_distances, text_error_rates, word_error_rate)
from ._trba.search import TextCorpus, TextHit, search_texts

__all__ = ["TRBA", "Lexicon", "EditCosts", "CharLM", "edit_distances", "character_error_rate", "accuracy", "sequence_edit_distances",
           "word_error_rate", "text_error_rates", "Alignment", "sequence_alignments", "error_breakdown",
           "TextCorpus", "TextHit", "search_texts"]
