from end2end_amd.functions.ctc_without_blank import CTCWithoutBlankLossFunction  # noqa: F401
