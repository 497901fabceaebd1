"""Utilities computed on the GPU: forced alignment, word segmentation, per-frame label pruning."""
from .pruning import label_cut  # noqa: F401
