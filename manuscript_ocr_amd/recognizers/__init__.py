from ._trba import TRBA
from ._trba.lexicon import Lexicon

__all__ = ["TRBA", "Lexicon"]
