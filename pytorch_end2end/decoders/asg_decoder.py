from end2end_amd.decoders.asg_decoder import ASGDecoder, ASGPathResults  # noqa: F401
