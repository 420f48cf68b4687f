from ._trba import TRBA
from ._trba.charlm import CharLM
from ._trba.lexicon import Lexicon

__all__ = ["TRBA", "Lexicon", "CharLM"]
