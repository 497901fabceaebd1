"""ASGLoss: the Auto Segmentation Criterion (Collobert et al. 2016, arXiv:1609.03193) with its learned transition matrix,
computed on the MI355X (e2e_asg_fwd_bwd; the definition is in include/e2e_ctc.h).  Upstream names ASG and stops at
``ASGEncoder``'s NotImplementedError; the call signature here is ``CTCWithoutBlankLoss``'s.

The emissions are unnormalised scores: no softmax is taken anywhere, the criterion normalises over the fully connected
graph.  ``transitions[j, i]`` is the score of label ``j`` following label ``i`` (row = to, column = from, the wav2letter
layout).  A blank-free model cannot emit a doubled letter; ``ASGEncoder`` packs those into repeat labels.
"""
import torch
import torch.nn as nn

from ..engines import ASGLossEngine
from ..functions.asg import ASGLossFunction

_engine = None


def asg_loss(emissions, transitions, targets, logits_lengths, targets_lengths):
    """The ``(batch,)`` ASG losses for callers who keep the transition matrix elsewhere; differentiable in ``emissions``
    (batch, time, alphabet) and ``transitions`` (alphabet, alphabet)."""
    global _engine
    if _engine is None:
        _engine = ASGLossEngine()
    return ASGLossFunction.apply(_engine, emissions, transitions, targets, logits_lengths, targets_lengths)


class ASGLoss(nn.Module):
    """
    :param num_labels: V, the number of columns of the emissions (1 to 128); sizes ``self.transitions``, a ``(V, V)``
        parameter that starts at zero
    :param reduce: return the sum of the losses instead of the ``(batch,)`` vector
    :param time_major: emissions are ``(time, batch, alphabet)``
    """

    def __init__(self, num_labels, reduce=True, time_major=False):
        super().__init__()
        self._engine = ASGLossEngine(num_labels)           # (refuses an alphabet the kernels do not serve, naming the limit)
        self._reduce = reduce
        self._time_major = time_major
        self.transitions = nn.Parameter(torch.zeros(int(num_labels), int(num_labels)))

    def forward(self, logits, targets, logits_lengths, targets_lengths):
        """
        :param logits: ``(batch, time, alphabet)`` emissions (unnormalised scores)
        :param targets: ``(batch, max_target_length)`` integer tensor, no two equal ids adjacent unless meant as such
        :param logits_lengths: ``(batch,)`` frame counts
        :param targets_lengths: ``(batch,)`` target lengths, at least 1
        :return: ``(batch,)`` losses, or their sum with ``reduce``
        """
        if self._time_major:
            logits = logits.transpose(0, 1)
        losses = ASGLossFunction.apply(self._engine, logits, self.transitions, targets, logits_lengths, targets_lengths)
        return losses.sum() if self._reduce else losses
