from .asg_decoder import ASGDecoder  # noqa: F401
from .ctc_decoder import CTCDecoder  # noqa: F401
from .gram_ctc_decoder import GramCTCDecoder  # noqa: F401
