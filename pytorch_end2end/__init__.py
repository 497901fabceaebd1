"""`pytorch_end2end` -- the reference's package name, served by the MI355X implementation in `end2end_amd`.

    from pytorch_end2end import CTCLoss, CTCDecoder, CTCEncoder

works unchanged (pytorch_end2end/__init__.py:1-6 upstream), and so do the sub-module paths the reference's users and
tests import (`pytorch_end2end.modules.ctc_loss`, `.decoders.ctc_decoder`, `.encoders.text_encoders`,
`.functions.forward_backward`, `.modules.ctc_without_blank`, `.functions.ctc_without_blank`,
`.modules.alignment_loss`, `.utils.alignment`).  The numba back-ends of CTC without blank and of the alignment run as HIP
kernels here, and so does Gram-CTC (`.modules.ctc_loss.GramCTCLoss`, an empty stub upstream).
Segmented CTC (`.modules.ctc_loss_segmented.CTCLossSegmented`, not importable upstream: a broken import) runs on the GPU
too.  ASG, which upstream names and leaves unimplemented (`.encoders.ASGEncoder`), is served as
`.encoders.ASGEncoder`, `.modules.asg_loss.ASGLoss` and `.decoders.ASGDecoder`.
"""
from end2end_amd import CTCDecoder, CTCDecoderError, CTCEncoder, CTCLoss, DecoderResults

__all__ = ["CTCLoss", "CTCDecoder", "CTCEncoder"]
