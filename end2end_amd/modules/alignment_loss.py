"""AlignedTargetsLoss with the reference's constructor and call signature
(pytorch_end2end/modules/alignment_loss.py:7-33): the NLL of the Viterbi alignment, averaged over each utterance's frames.

The alignment comes from e2e_ctc_align (utils.alignment.get_alignment_3d with keep_on_device=True), so nothing goes
through the host; the rest is upstream's arithmetic in torch.
"""
import torch.nn as nn
import torch.nn.functional as F

from ..utils.alignment import get_alignment_3d


class AlignedTargetsLoss(nn.Module):
    def __init__(self, is_ctc, ignore_blank=False):
        super().__init__()
        self._is_ctc = is_ctc
        self._ignore_blank = ignore_blank

    def forward(self, log_probs, targets, input_lengths, target_lengths):
        """
        :param log_probs: batch_size * sequence_length * num_labels
        :param targets: batch_size * max_target_length
        :param input_lengths: batch_size
        :param target_lengths: batch_size
        :return: ``(batch,)`` mean NLL per frame of the aligned labels
        """
        targets_new = get_alignment_3d(log_probs, targets, input_lengths, target_lengths, is_ctc=self._is_ctc,
                                       keep_on_device=True).to(log_probs.device)
        batch_size, sequence_length, _ = log_probs.shape
        if self._ignore_blank:
            targets_new[targets_new == 0] = -100
        loss = F.nll_loss(log_probs.reshape(batch_size * sequence_length, -1),
                          targets_new.reshape(batch_size * sequence_length),
                          reduction="none", ignore_index=-100).reshape(batch_size, sequence_length)
        return loss.sum(dim=-1) / input_lengths
