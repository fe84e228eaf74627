from .cross_encoder import CrossEncoder

__all__ = ["CrossEncoder"]
