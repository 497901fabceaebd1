from end2end_amd.decoders.gram_ctc_decoder import GramCTCDecoder, GramGreedyResults, GramNBestResults  # noqa: F401
