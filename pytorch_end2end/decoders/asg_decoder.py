from end2end_amd.decoders.asg_decoder import ASGDecoder, ASGPathResults  # noqa: F401
from end2end_amd.decoders.ctc_decoder import CTCDecoderError, NBestResults  # noqa: F401
