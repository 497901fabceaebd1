"""ASGDecoder: decoding for models trained with ASGLoss or CTCWithoutBlankLoss.  As constructed: the Viterbi path
through emissions and learned transitions (e2e_asg_viterbi), its repeats merged and its repeat labels expanded.
After ``configure(beam_width > 1, ...)``: n-best prefix beam search with the transitions and, optionally, a word language model
(e2e_asg_beam_nbest).  ``restrict_to_vocabulary()`` restricts that search to the language model's words or to a word list,
``decode_nbest(..., timesteps=True)`` says at which frame each label entered the beam (e2e_asg_beam_nbest_opt).
``prune(cutoff_top_n=K)`` makes a frame expand its K highest-scoring labels alone (e2e_asg_beam_nbest_cut; flashlight's
``beam_size_token``); there is no ``cutoff_prob``, because ASG emissions are scores, not probabilities.
``open_stream(transitions, batch_size, max_frames)`` is the same search fed in chunks, the beams kept on the GPU in between
(e2e_asg_beam_stream): after every chunk the result of ``decode`` / ``decode_nbest`` on everything fed so far.  The
definitions are in include/e2e_ctc.h; upstream has no ASG decoder; the return conventions are CTCDecoder's.

With ``num_replabels=0`` (a ``CTCWithoutBlankLoss`` model) a word with a doubled letter cannot be spelled -- equal neighbours
merge --, so a restricted search never produces it.

Not provided for ASG: custom transcriptions, a lexicon together with a language model, widths or alphabets
above 128, -inf transitions.
"""
import os
from collections import namedtuple

import torch

from ..engines import ASGBeamEngine, ASGViterbiEngine
from .ctc_decoder import CTCDecoderError, DecoderResults, NBestResults, _DecoderStream, read_lexicon

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

    The constructor is the best-path decoder's; the beam search is set up with ``configure()``, as ``CTCDecoderEngine``
    sets up what goes beyond upstream's constructor.
    """

    def __init__(self, labels=None, num_replabels=0, time_major=False, keep_on_device=False):
        if int(num_replabels) < 0:
            raise CTCDecoderError("num_replabels must be >= 0")
        self._labels = list(labels) if labels is not None else None
        self._num_replabels = int(num_replabels)
        self._time_major = time_major
        self._keep_on_device = keep_on_device
        self._decoder = ASGViterbiEngine(PATH_PAD, keep_on_device=keep_on_device)
        self._beam_width = 1
        self._beam = None

    def configure(self, beam_width=1, lm_path=None, lmwt=1.0, wip=1.0, oov_penalty=-10, case_sensitive=True):
        """Set up the beam search, once, before decoding; returns self.  The names and defaults are ``CTCDecoder``'s.

        :param beam_width: number of hypotheses kept; ``1`` (the default) means best-path (Viterbi) decoding, unchanged
        :param lm_path: ARPA (optionally gzipped) language model, for ``beam_width > 1``; a word is looked up with its repeat
            labels expanded
        :param lmwt: language-model weight
        :param wip: word insertion penalty
        :param oov_penalty: penalty per out-of-vocabulary word
        :param case_sensitive: look words up in the language model with their case

        A width above the limit is refused here, an alphabet above it at the first call: both before any launch.
        """
        beam_width = int(beam_width)
        lm_path = os.path.abspath(lm_path) if lm_path else ""
        if beam_width < 1:
            raise CTCDecoderError("beam_width must be >= 1")
        if lm_path:
            if beam_width == 1:
                raise CTCDecoderError("lm_path needs beam_width > 1: best-path decoding has no language model")
            if not os.path.isfile(lm_path):
                raise CTCDecoderError("Can't find a model: {}".format(lm_path))
            if self._labels is None:
                raise CTCDecoderError("a language model needs labels: the alphabet spells its words")
        self._beam = None
        if beam_width > 1:
            self._beam = ASGBeamEngine(self._labels, self._num_replabels, beam_width, lm_path, lmwt, wip, oov_penalty,
                                       case_sensitive, keep_on_device=self._keep_on_device)
        self._beam_width = beam_width
        return self

    def restrict_to_vocabulary(self, lexicon=None):
        """Restrict the beam search to a vocabulary, after ``configure(beam_width > 1, ...)``; returns self.  The search then
        only forms words of the vocabulary: a label is taken only if the last word, repeat labels expanded, is still the
        beginning of a word, and a space only after a whole word (the last word of a result may still be an unfinished
        prefix of one, counted as out of vocabulary).

        :param lexicon: ``None``: the words of the configured language model (``lm_path``).  Otherwise an iterable of words, or
            the path of a text file with one entry per line whose first white-space separated token is the word: the search
            is restricted to them without a language model; ``lmwt`` and ``oov_penalty`` then count as 0, ``wip`` applies.
            Not together with ``lm_path``.

        A later ``configure()`` builds a new search and drops the restriction.
        """
        if self._labels is None:
            raise CTCDecoderError("restrict_to_vocabulary needs labels: the alphabet spells the vocabulary's words")
        if self._beam is None:
            raise CTCDecoderError("restrict_to_vocabulary needs beam_width > 1: best-path decoding has no vocabulary")
        try:
            self._beam.restrict(None if lexicon is None else read_lexicon(lexicon))
        except ValueError as e:
            raise CTCDecoderError(str(e))
        return self

    def prune(self, cutoff_top_n=None):
        """Per-frame label pruning of the beam search, after ``configure(beam_width > 1, ...)``; returns self.

        :param cutoff_top_n: a frame expands only its ``cutoff_top_n`` highest-scoring labels (ties: the lower id), and a
            hypothesis whose last label is not among them does not stay in that frame: it lives on only in its extensions.
            ``None`` (or a value that is no less than the alphabet): not pruned.

        There is no ``cutoff_prob``: ASG emissions are scores, not probabilities.  Works in either order with
        ``restrict_to_vocabulary()``; streams opened afterwards use it; ``decode_path`` and best-path decoding ignore it.
        A later ``configure()`` builds a new search and drops the setting.
        """
        if cutoff_top_n is not None and (isinstance(cutoff_top_n, bool) or not isinstance(cutoff_top_n, int) or cutoff_top_n < 1):
            raise CTCDecoderError("cutoff_top_n must be an integer >= 1 (or None), got {!r}".format(cutoff_top_n))
        if self._beam is None:
            if cutoff_top_n is None:
                return self
            raise CTCDecoderError("cutoff_top_n needs beam_width > 1: best-path decoding expands nothing")
        self._beam.prune(cutoff_top_n)
        return self

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
            repeat labels expanded.  ``beam_width > 1``: hypothesis 0 of ``decode_nbest``, the ids packed to the longest
            result; ``transitions`` may then be ``None`` (all zero)"""
        emissions, logits_lengths = self._batch_major(emissions, logits_lengths)
        if self._beam is not None:
            return DecoderResults(*self._beam.decode(emissions, transitions, logits_lengths))
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

    def decode_nbest(self, emissions, transitions, logits_lengths=None, nbest=None, timesteps=False):
        """The hypotheses the beam search ends with, best first (``beam_width > 1``).  ``transitions=None`` means zero
        transitions: a ``CTCWithoutBlankLoss`` model is decoded by passing its log-softmax output, ``num_replabels=0``.

        :param nbest: how many to return per utterance, at most ``beam_width`` (the default)
        :param timesteps: also return ``timesteps (batch, nbest, longest)`` int64: for every label the frame at which the
            sequence ending in it last entered the beam, ``-1`` behind a sequence.  In a wide beam a sequence can enter the beam
            before its last label becomes likely
        :return: ``CTCDecoder``'s ``NBestResults``: ``decoded_targets (batch, nbest, longest)`` -- the merged labels, repeat
            labels as they are --, ``decoded_targets_lengths``, ``decoded_sentences`` (repeat labels expanded), ``scores``,
            ``ctc_scores`` (the acoustic score: log of the summed path scores of the labelling, within the beam),
            ``lm_scores``, ``num_words``, ``num_oov_words``, ``num_hypotheses``, ``timesteps`` (``None`` unless asked for);
            ``scores = ctc_scores + lmwt * lm_scores - wip * num_words + oov_penalty * num_oov_words``.
        """
        if self._beam is None:
            raise CTCDecoderError("decode_nbest needs beam_width > 1: best-path decoding has no beam")
        emissions, logits_lengths = self._batch_major(emissions, logits_lengths)
        return NBestResults(*self._beam.decode_nbest(emissions, transitions, logits_lengths, nbest=nbest, timesteps=timesteps))

    def open_stream(self, transitions, batch_size, max_frames, timesteps=False):
        """Streaming beam search, after ``configure(beam_width > 1, ...)``: an ``ASGDecoderStream`` that is fed the emissions in
        chunks and keeps the beams of ``batch_size`` utterances of up to ``max_frames`` frames on the GPU in between.  After
        every chunk the result is that of ``decode`` / ``decode_nbest`` on everything fed so far; the decoder's settings,
        a restriction set with ``restrict_to_vocabulary()`` included, apply as they do there.

        :param transitions: the ``(V, V)`` transitions of every chunk, given once; ``None``: all zero
        :param timesteps: ``feed_nbest`` also returns the frames of the labels, counted from the stream's start
        """
        if self._beam is None:
            raise CTCDecoderError("a stream needs configure(beam_width > 1): best-path decoding has no beam to keep")
        try:
            return ASGDecoderStream(self, self._beam.open_stream(transitions, batch_size, max_frames, timesteps=timesteps))
        except ValueError as e:
            raise CTCDecoderError(str(e))


class ASGDecoderStream(_DecoderStream):
    """What ``ASGDecoder.open_stream`` returns: ``_DecoderStream`` (``CTCDecoderStream``'s surface), fed emissions as they
    are."""

    def _chunk(self, emissions, logits_lengths):
        emissions, logits_lengths = self._owner._batch_major(emissions, logits_lengths)
        self._stream.check_chunk(tuple(emissions.shape))          # (before any device work)
        return emissions, logits_lengths
