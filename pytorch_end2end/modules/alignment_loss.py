from end2end_amd.modules.alignment_loss import AlignedTargetsLoss  # noqa: F401
