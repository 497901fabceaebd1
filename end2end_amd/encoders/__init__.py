from .text_encoders import ASGEncoder, CTCEncoder

__all__ = ["CTCEncoder", "ASGEncoder"]
