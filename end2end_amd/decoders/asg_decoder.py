"""ASGDecoder: best-path decoding for models trained with ASGLoss -- the Viterbi path through emissions and learned
transitions (e2e_asg_viterbi; the definition is in include/e2e_ctc.h), its repeats merged and its repeat labels expanded.
Upstream has no ASG decoder; the return conventions are CTCDecoder's.

Not provided for ASG: beam search, a language model, a lexicon.
"""
from collections import namedtuple

import torch

from ..engines import ASGViterbiEngine
from .ctc_decoder import CTCDecoderError, DecoderResults

# decode_path(): the label of every frame, -100 past an utterance's length (as get_alignment_3d pads), and the paths' scores
ASGPathResults = namedtuple("ASGPathResults", ["paths", "scores"])

PATH_PAD = -100


class ASGDecoder:
    """
    :param labels: the character strings of the columns ``0 .. V - num_replabels - 1`` (a list of all V columns is taken
        too: the repeat labels' entries are not read); ``None``: sentences are empty
    :param num_replabels: R: the last R columns are repeat labels, column ``V - R + r - 1`` meaning "the character
        before, r more times" (``ASGEncoder``'s ids)
    :param time_major: emissions are ``(time, batch, alphabet)``
    :param keep_on_device: leave the decoded ids, lengths, paths and scores on the GPU
    """

    def __init__(self, labels=None, num_replabels=0, time_major=False, keep_on_device=False):
        if int(num_replabels) < 0:
            raise CTCDecoderError("num_replabels must be >= 0")
        self._labels = list(labels) if labels is not None else None
        self._num_replabels = int(num_replabels)
        self._time_major = time_major
        self._decoder = ASGViterbiEngine(PATH_PAD, keep_on_device=keep_on_device)

    def _batch_major(self, emissions, logits_lengths):
        if self._time_major:
            emissions = emissions.transpose(1, 0)
        emissions = emissions.detach()
        if logits_lengths is None:
            logits_lengths = torch.full((emissions.size(0),), emissions.size(1), dtype=torch.long, device=emissions.device)
        return emissions, logits_lengths

    def _sentence(self, ids, num_chars):
        out = []
        for i in ids:
            if i < num_chars:
                out.append(self._labels[i])
            elif out:                          # (a leading repeat label has nothing to repeat)
                out.extend([out[-1]] * (i - num_chars + 1))
        return "".join(out)

    def decode_path(self, emissions, transitions, logits_lengths=None):
        """:return: ``ASGPathResults(paths (batch, time) int64, -100 past the length; scores (batch,) float64)``"""
        emissions, logits_lengths = self._batch_major(emissions, logits_lengths)
        paths, scores, _, _ = self._decoder.compute(emissions, transitions, logits_lengths)
        return ASGPathResults(paths, scores)

    def decode(self, emissions, transitions, logits_lengths=None):
        """:return: ``DecoderResults(decoded_targets (batch, time) -- the best path with consecutive repeats merged, zero
            padded as greedy decoding pads --, decoded_targets_lengths, decoded_sentences)``; the sentences have the
            repeat labels expanded"""
        emissions, logits_lengths = self._batch_major(emissions, logits_lengths)
        V = emissions.size(2)
        num_chars = V - self._num_replabels
        if num_chars < 1:
            raise CTCDecoderError("%d columns leave no characters beside %d repeat labels" % (V, self._num_replabels))
        if self._labels is not None and len(self._labels) not in (num_chars, V):
            raise CTCDecoderError("the decoder has %d labels but the emissions have %d columns, %d of them repeat labels"
                                  % (len(self._labels), V, self._num_replabels))
        _, _, ids, lengths = self._decoder.compute(emissions, transitions, logits_lengths)
        if self._labels is None:
            sentences = ["" for _ in range(ids.size(0))]
        else:
            sentences = [self._sentence(row[:n], num_chars) for row, n in zip(ids.tolist(), lengths.tolist())]
        return DecoderResults(ids, lengths, sentences)
