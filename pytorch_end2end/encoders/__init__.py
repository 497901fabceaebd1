from .text_encoders import ASGEncoder, CTCEncoder  # noqa: F401
