from end2end_amd.encoders.text_encoders import ASGEncoder, CTCEncoder  # noqa: F401
