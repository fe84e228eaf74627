from .cross_encoder import CrossEncoder
from .word_encoder import WordEncoder

__all__ = ["CrossEncoder", "WordEncoder"]
