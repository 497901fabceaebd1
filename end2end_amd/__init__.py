"""end2end_amd -- MI355X-native CTC loss and decoder with the pytorch_end2end API.

    from end2end_amd import CTCLoss, CTCDecoder, CTCEncoder

is a drop-in for `from pytorch_end2end import CTCLoss, CTCDecoder, CTCEncoder`
(pytorch_end2end/__init__.py:1-6): same constructors, call signatures and results, computed
by hand-written HIP kernels (end2end_amd/csrc, C ABI in include/e2e_ctc.h).
"""
from .decoders.asg_decoder import ASGDecoder, ASGPathResults
from .decoders.ctc_decoder import CTCDecoder, CTCDecoderError, DecoderResults, NBestResults
from .decoders.gram_ctc_decoder import GramCTCDecoder, GramGreedyResults, GramNBestResults
from .encoders.text_encoders import ASGEncoder, CTCEncoder
from .modules.alignment_loss import AlignedTargetsLoss
from .modules.asg_loss import ASGLoss, asg_loss
from .modules.ctc_loss import CTCLoss, GramCTCLoss
from .modules.ctc_loss_segmented import CTCLossSegmented
from .modules.ctc_without_blank import CTCWithoutBlankLoss

__all__ = ["CTCLoss", "CTCDecoder", "CTCEncoder", "CTCDecoderError", "DecoderResults", "NBestResults", "CTCWithoutBlankLoss",
           "AlignedTargetsLoss", "GramCTCLoss", "GramCTCDecoder", "GramNBestResults", "GramGreedyResults",
           "CTCLossSegmented", "ASGLoss", "asg_loss", "ASGDecoder", "ASGPathResults", "ASGEncoder"]
