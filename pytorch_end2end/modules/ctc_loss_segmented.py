from end2end_amd.modules.ctc_loss_segmented import CTCLossSegmented  # noqa: F401
