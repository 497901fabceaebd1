"""CTCWithoutBlankLossFunction with the reference's call signature
(pytorch_end2end/functions/ctc_without_blank.py:108-138), computed on the MI355X by e2e_ctc_noblank_fwd_bwd.

    losses = CTCWithoutBlankLossFunction.apply(logprobs, targets, logits_lengths, targets_lengths, space_idx=-1)

`logprobs` is (batch, time, alphabet) AFTER log-softmax.  The kept gradient is upstream's: exp(lp) - posterior on the
frames t < logits_lengths[b], 0 on padded frames; backward multiplies it by grad_output.view(-1, 1, 1).  Differences:
nothing is copied to the host, and the losses come back in the input's dtype and device (upstream: always float32), so
that an f64 gradcheck works -- as CTCLoss does (quirk Q3).
"""
from ..engines import CTCWithoutBlankLossEngine
from .forward_backward import ForwardBackwardLossFunction

_engines = {}


def _engine(space_idx):
    eng = _engines.get(space_idx)
    if eng is None:
        eng = _engines[space_idx] = CTCWithoutBlankLossEngine(space_idx)
    return eng


class CTCWithoutBlankLossFunction(ForwardBackwardLossFunction):
    """The generic forward-backward Function bound to the blank-free engine, with upstream's `apply` arguments."""

    @staticmethod
    def forward(ctx, logits, targets, logits_lengths, targets_lengths, space_idx=-1):
        return ForwardBackwardLossFunction.forward(ctx, _engine(int(space_idx)), logits, targets, logits_lengths,
                                                   targets_lengths)

    @staticmethod
    def backward(ctx, grad_output):
        return ForwardBackwardLossFunction.backward(ctx, grad_output)[1:6]
