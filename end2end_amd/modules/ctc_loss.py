"""CTCLoss module with the reference's constructor and call signature
(pytorch_end2end/modules/ctc_loss.py:15-75), computing on the MI355X.

Differences that do not change results:
  * with after_logsoftmax=False the log-softmax (and its backward) is fused into the HIP
    kernel instead of running F.log_softmax before the engine (`fused=False` restores the
    reference's two-step structure);
  * nothing is copied to the host.
"""
import torch.nn as nn
import torch.nn.functional as F

from ..engines import CTCLossEngine, GramCTCLossEngine
from ..functions.forward_backward import ForwardBackwardLossFunction


class ForwardBackwardLossBase(nn.Module):
    def __init__(self, size_average=None, reduce=None, after_logsoftmax=False, time_major=False, blank_idx=0):
        super().__init__()
        self._blank_idx = blank_idx
        self._reduce = reduce
        self._size_average = size_average
        self._after_logsoftmax = after_logsoftmax
        self._time_major = time_major
        self._engine = None
        self._fused = True

    def forward(self, logits, targets, logits_lengths, targets_lengths):
        """
        :param logits: float tensor, ``(time, batch, alphabet)`` if ``time_major`` else ``(batch, time, alphabet)``
        :param targets: ``(batch, max_target_length)`` integer tensor
        :param logits_lengths: ``(batch,)`` frame counts
        :param targets_lengths: ``(batch,)`` target lengths
        :return: ``(batch,)`` losses when ``reduce`` is falsy, else their mean (``size_average``) or sum
        """
        fuse = self._fused and not self._after_logsoftmax
        x = logits
        if not self._after_logsoftmax and not fuse:
            x = F.log_softmax(x, dim=2)
        if self._time_major:
            x = x.permute(1, 0, 2)          # a strided view; the kernel reads through the strides
        # reduce: the sum / mean is written by the tail of the engine's last kernel (no separate reduction) and the
        # kept gradient is already scaled, so `loss.backward()` finds nothing left to multiply
        reduction = ("mean" if self._size_average else "sum") if self._reduce else None
        return ForwardBackwardLossFunction.apply(self._engine, x, targets, logits_lengths, targets_lengths, fuse,
                                                 reduction)


class CTCLoss(ForwardBackwardLossBase):
    """
    Connectionist Temporal Classification loss (Graves et al., 2006).

    :param size_average: average (instead of sum) over the batch; only with ``reduce``
    :param reduce: reduce to a scalar; ``None`` returns the ``(batch,)`` vector
    :param after_logsoftmax: inputs are already log-probabilities
    :param time_major: inputs are ``(time, batch, alphabet)``
    :param blank_idx: index of the blank label
    :param fused: fuse log-softmax into the kernel when ``after_logsoftmax`` is False
    :param f32_chains: (extension, default off) let the lattice chains of long-target batches run in packed f32:
        ~10 % faster at B=256, T=1000, V=29, S<=200; gradient elements within 2e-5 absolute of the reference's
        instead of 2e-6 (``e2e_ctc_loss_opts.chains`` in include/e2e_ctc.h)
    """

    def __init__(self, size_average=None, reduce=None, after_logsoftmax=False, time_major=False, blank_idx=0,
                 fused=True, f32_chains=False):
        super().__init__(size_average, reduce, after_logsoftmax, time_major, blank_idx)
        self._fused = fused
        self._engine = CTCLossEngine(self._blank_idx, f32_chains=f32_chains)


class GramCTCLoss(CTCLoss):
    """
    Gram-CTC loss (Liu et al., ICML 2017, `<https://arxiv.org/abs/1703.00096>`_): the model may emit whole n-grams of
    base labels as single columns.  A path's labelling collapses runs of one column, drops blanks and concatenates the
    grams' base sequences; the loss is -log of the total probability of the paths that spell the target.  Computed by
    e2e_gram_ctc_fwd_bwd (definition and limits: include/e2e_ctc.h).

    :param blank_idx: id of the blank label, only ``0`` supported
    :param num_base_labels: R, the base labels with the blank counted: targets hold ids ``1 .. R-1``
    :param total_labels: V, the columns of the logits: ``1 .. R-1`` the unigrams, ``R .. V-1`` the grams
    :param label2ids: ``{column: [base ids]}`` for every column ``>= R`` (1 to 8 ids each); entries for ``c < R`` must be
        ``[c]``
    :param size_average: average (instead of sum) over the batch; only with ``reduce``
    :param reduce: reduce to a scalar; ``None`` returns the ``(batch,)`` vector
    :param after_logsoftmax: inputs are already log-probabilities
    :param time_major: inputs are ``(time, batch, alphabet)``
    :param fused: (extension) fuse log-softmax into the kernel when ``after_logsoftmax`` is False
    """

    def __init__(self, blank_idx, num_base_labels, total_labels, label2ids,
                 size_average=None, reduce=None, after_logsoftmax=False, time_major=False, fused=True):
        ForwardBackwardLossBase.__init__(self, size_average, reduce, after_logsoftmax, time_major, blank_idx)
        if self._blank_idx != 0:
            raise NotImplementedError("Gram-CTC supports blank_idx=0 only (as upstream)")
        self._fused = fused
        self._num_base_labels = num_base_labels
        self._total_labels = total_labels
        self._label2ids = label2ids
        self._engine = GramCTCLossEngine(self._blank_idx, self._num_base_labels, self._total_labels, self._label2ids)
