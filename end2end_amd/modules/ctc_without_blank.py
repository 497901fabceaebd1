"""CTCWithoutBlankLoss with the reference's constructor and call signature
(pytorch_end2end/modules/ctc_without_blank.py:7-30), computing on the MI355X (e2e_ctc_noblank_fwd_bwd).

Differences that do not change results:
  * with after_softmax=False the log-softmax (and its backward) is fused into the HIP kernel instead of running
    LogSoftmax before the loss (`fused=False` restores the reference's two-step structure);
  * with reduce=True the sum is written by the loss call itself, and the kept gradient needs no scaling afterwards;
  * nothing is copied to the host; the losses keep the input's dtype (upstream: float32).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ..engines import CTCWithoutBlankLossEngine
from ..functions.forward_backward import ForwardBackwardLossFunction


class CTCWithoutBlankLoss(nn.Module):
    """
    CTC without the blank label (ASG-style lattice: a frame stays on its label or moves to the next one).

    :param reduce: return the sum of the losses (there is no mean, as upstream) instead of the ``(batch,)`` vector
    :param after_softmax: inputs are probabilities (``torch.log`` is taken) instead of logits (log-softmax is taken)
    :param space_idx: label wrapped around every target (``[sp] + target + [sp]``), or -1 for none
    :param fused: (extension) fuse log-softmax into the kernel when ``after_softmax`` is False
    """

    def __init__(self, reduce=True, after_softmax=False, space_idx=-1, fused=True):
        super().__init__()
        self._space_idx = space_idx
        self._reduce = reduce
        self._after_softmax = after_softmax
        self._fused = fused
        self._engine = CTCWithoutBlankLossEngine(space_idx)

    def forward(self, logits, targets, logits_lengths, targets_lengths):
        """
        :param logits: ``(batch, time, alphabet)`` logits, or probabilities with ``after_softmax``
        :param targets: ``(batch, max_target_length)`` integer tensor
        :param logits_lengths: ``(batch,)`` frame counts
        :param targets_lengths: ``(batch,)`` target lengths
        :return: ``(batch,)`` losses, or their sum with ``reduce``
        """
        fuse = self._fused and not self._after_softmax
        if self._after_softmax:
            x = torch.log(logits)          # autograd then gives upstream's (p - posterior) / p
        elif fuse:
            x = logits
        else:
            x = F.log_softmax(logits, dim=2)
        return ForwardBackwardLossFunction.apply(self._engine, x, targets, logits_lengths, targets_lengths, fuse,
                                                 "sum" if self._reduce else None)
