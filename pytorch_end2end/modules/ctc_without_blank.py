from end2end_amd.modules.ctc_without_blank import CTCWithoutBlankLoss  # noqa: F401
