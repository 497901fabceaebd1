"""GramCTCDecoder: greedy and prefix beam-search decoding for models trained with GramCTCLoss.  The constructor takes the
loss's table (``num_base_labels, total_labels, label2ids``) and CTCDecoder's decoding arguments; the return conventions are
CTCDecoder's.  Upstream has no such decoder (its Gram-CTC engine is empty); the definition is in include/e2e_ctc.h.
After ``configure(lm_path=..., lmwt=..., wip=..., oov_penalty=...)`` the beam search ranks by the acoustic score together
with a word language model, a word insertion penalty and an out-of-vocabulary penalty (e2e_gram_ctc_beam_nbest_lm): the
base labels spell the words, the space among them separates them, and a gram may end one word and begin the next.
``restrict_to_vocabulary()`` then restricts the search to the model's words or to a word list, and
``decode_nbest(..., timesteps=True)`` also returns the frame at which each id entered the beam (e2e_gram_ctc_beam_nbest_opt).
``open_stream(batch_size, max_frames)`` is the same search, configured or not, fed in chunks with the beams kept on the GPU in
between (e2e_gram_ctc_beam_stream): after every chunk the result of ``decode`` / ``decode_nbest`` on everything fed so far.

Not provided for Gram-CTC: custom transcriptions, a word list together with a language model, a column
segmentation per beam hypothesis (several segmentations spell one hypothesis), ``blank_idx != 0``.
"""
import os
from collections import namedtuple

import torch

from ..engines import GramCTCDecoderEngine
from .ctc_decoder import CTCDecoderError, DecoderResults, NBestResults, _DecoderStream

# decode_nbest(): (B, N, ...) per utterance and hypothesis, ranked by `scores` (the log-probability of the labelling within
# the beam); `decoded_sentences[b]` lists the num_hypotheses[b] sentences of utterance b
GramNBestResults = namedtuple("GramNBestResults", ["decoded_targets", "decoded_targets_lengths", "decoded_sentences",
                                                   "scores", "num_hypotheses"])

# decode_greedy(return_columns=True): also the collapsed columns -- the gram segmentation the model chose
GramGreedyResults = namedtuple("GramGreedyResults", ["decoded_targets", "decoded_targets_lengths", "decoded_sentences",
                                                     "columns", "columns_lengths"])


class GramCTCDecoder:
    """
    :param blank_idx: index of the blank column; only ``0`` is supported (as for ``GramCTCLoss``)
    :param num_base_labels: R, the blank counted: base ids are ``1 .. R-1``
    :param total_labels: V, the number of columns of the logits
    :param label2ids: ``{column: [base ids]}`` for the gram columns ``R .. V-1`` (grams of 1 to 8 base ids)
    :param beam_width: number of hypotheses kept; ``1`` makes ``decode`` greedy (argmax) decoding, as for ``CTCDecoder``
    :param labels: the R base-label strings including the blank's, e.g. ``["_", "a", "b"]``
    :param after_logsoftmax: inputs are log-probabilities (greedy ignores this)
    :param time_major: inputs are ``(time, batch, alphabet)``
    :param keep_on_device: leave the decoded ids and lengths on the GPU
    :param cutoff_top_n: per-frame label pruning, ``CTCDecoder``'s: a frame expands at most this many columns (unigrams and
        grams alike), the likeliest (ties to the lower column), and the blank.  ``None`` or a value that is no less than
        ``total_labels``: no limit.  At most 1024 columns can be kept; needs ``beam_width > 1``.  A pruned search's width
        limit is ``min(128, 131072 / (min(cutoff_top_n, total_labels) + 1))``, whatever the alphabet.
    :param cutoff_prob: ... and of those the fewest whose probabilities sum to this, in ``(0, 1]``; ``1.0``: all.  With both
        at their defaults the decoder is the unpruned one.  ``configure()`` and ``restrict_to_vocabulary()`` keep the two;
        a stream takes those the decoder has at ``open_stream``; ``decode_greedy`` ignores them.
    """

    def __init__(self, blank_idx=0, num_base_labels=None, total_labels=None, label2ids=None, beam_width=100, labels=None,
                 after_logsoftmax=False, time_major=False, keep_on_device=False, transcriptions=None,
                 cutoff_top_n=None, cutoff_prob=1.0):
        if transcriptions is not None:
            raise CTCDecoderError("GramCTCDecoder does not support custom transcriptions: its search spells words from the base labels")
        if num_base_labels is None or total_labels is None:
            raise CTCDecoderError("GramCTCDecoder needs num_base_labels and total_labels (the arguments of GramCTCLoss)")
        self._beam_width = beam_width
        self._after_logsoftmax = after_logsoftmax
        self._time_major = time_major
        # (CTCDecoder._check_params' tests and texts)
        if cutoff_top_n is not None and (isinstance(cutoff_top_n, bool) or int(cutoff_top_n) != cutoff_top_n or cutoff_top_n < 1):
            raise CTCDecoderError("cutoff_top_n must be an integer >= 1 (or None), got {!r}".format(cutoff_top_n))
        if not isinstance(cutoff_prob, (int, float)) or not 0.0 < cutoff_prob <= 1.0:
            raise CTCDecoderError("cutoff_prob must be in (0, 1], got {!r}".format(cutoff_prob))
        if (cutoff_top_n is not None or cutoff_prob != 1.0) and beam_width == 1:
            raise CTCDecoderError("cutoff_top_n / cutoff_prob need beam_width > 1: greedy decoding expands nothing")
        pruned = cutoff_top_n is not None or cutoff_prob != 1.0
        try:
            self._decoder = GramCTCDecoderEngine(blank_idx, num_base_labels, total_labels, label2ids or {}, beam_width,
                                                 labels, keep_on_device=keep_on_device, cutoff_top_n=cutoff_top_n,
                                                 cutoff_prob=cutoff_prob)
        except ValueError as e:
            if not pruned:
                raise
            raise CTCDecoderError(str(e)) from e

    def configure(self, lm_path=None, lmwt=1.0, wip=1.0, oov_penalty=-10, case_sensitive=True):
        """Set up the beam search with a word language model, before decoding; returns self.  The names and defaults are
        ``CTCDecoder``'s.  A decoder that was never configured searches on the labellings' probabilities alone.

        :param lm_path: ARPA (optionally gzipped) language model; ``None``: no model, ``wip`` still applies per word
        :param lmwt: language-model weight
        :param wip: word insertion penalty
        :param oov_penalty: penalty per out-of-vocabulary word
        :param case_sensitive: look words up in the language model with their case

        The decoder needs ``labels`` (they spell the words; ``" "`` among them separates the words, without it a hypothesis
        is one word) and ``beam_width > 1``: a ``ValueError`` otherwise.  A later ``configure()`` replaces the former one
        and drops a restriction to a vocabulary.
        """
        lm_path = os.path.abspath(lm_path) if lm_path else ""
        if lm_path and not os.path.isfile(lm_path):
            raise CTCDecoderError("Can't find a model: {}".format(lm_path))
        self._decoder.configure(lm_path, lmwt, wip, oov_penalty, case_sensitive)
        return self

    def restrict_to_vocabulary(self, lexicon=None):
        """Restrict the beam search to a vocabulary, after ``configure()``; returns self.  Only sequences whose every word is
        a word of the vocabulary, the last one possibly unfinished (a prefix of a word), are formed; a gram is taken only if
        all its ids may follow, a gram with an inner space only if the word it closes is one.

        :param lexicon: ``None``: the words of the language model given to ``configure(lm_path=...)``.  A path to a text file
            of words or an iterable of words: the vocabulary without a model -- ``lmwt`` and ``oov_penalty`` then count as 0,
            ``wip`` applies; not together with ``lm_path``.

        A ``ValueError`` before ``configure()``, without any vocabulary, or with both.  A later ``configure()`` drops the
        restriction.  ``decode`` then returns hypothesis 0 of the restricted search.
        """
        if not self._decoder.configured:
            raise ValueError("restrict_to_vocabulary() comes after configure(): configure(lm_path=...) for a model's words, "
                             "configure(wip=...) and a lexicon for a word list")
        self._decoder.restrict(lexicon)
        return self

    def _batch_major(self, logits, logits_lengths):
        if self._time_major:
            logits = logits.transpose(1, 0)
        logits = logits.detach()
        if logits_lengths is None:
            logits_lengths = torch.full((logits.size(0),), logits.size(1), dtype=torch.int32, device=logits.device)
        return logits, logits_lengths

    def _logprobs(self, logits):
        with torch.no_grad():
            if not self._after_logsoftmax:
                logits = torch.log_softmax(logits, -1)
        return logits

    def decode_greedy(self, logits, logits_lengths=None, return_columns=False):
        """Arg-max column per frame, runs collapsed, blanks dropped, grams expanded: raw logits or log-probabilities.

        :return: ``DecoderResults(decoded_targets (batch, time * max_order) zero padded, decoded_targets_lengths,
            decoded_sentences)``; with ``return_columns`` a ``GramGreedyResults`` that also has ``columns (batch, time)``
            zero padded and ``columns_lengths``
        """
        logits, logits_lengths = self._batch_major(logits, logits_lengths)
        r = self._decoder.decode_greedy(logits_=logits, logits_lengths_=logits_lengths, return_columns=return_columns)
        return GramGreedyResults(*r) if return_columns else DecoderResults(*r)

    def decode(self, logits, logits_lengths=None):
        """Prefix beam search over base-label sequences; ``beam_width == 1`` routes to greedy decoding.

        :return: ``DecoderResults(decoded_targets (batch, longest), decoded_targets_lengths, decoded_sentences)``
        """
        if self._beam_width == 1:
            return self.decode_greedy(logits, logits_lengths)
        logits, logits_lengths = self._batch_major(self._logprobs(logits), logits_lengths)
        return DecoderResults(*self._decoder.decode(logits_=logits, logits_lengths_=logits_lengths))

    def decode_nbest(self, logits, logits_lengths=None, nbest=None, timesteps=False):
        """The hypotheses the beam search ends with, best first.

        :param nbest: how many to return per utterance, at most ``beam_width`` (the default)
        :param timesteps: after ``configure()`` only: also fill ``NBestResults.timesteps``, ``(batch, nbest, longest)``,
            -1 padded -- for every id the frame at which the sequence that ends in its gram entered the beam (the ids of one
            gram share it; in a wide beam that can be before the label is heard).  An unconfigured decoder returns
            ``GramNBestResults``, which has no such field: a ``ValueError`` that names ``configure(wip=0)``
        :return: ``GramNBestResults(decoded_targets (batch, nbest, longest), decoded_targets_lengths (batch, nbest),
            decoded_sentences (a list per utterance), scores (batch, nbest), num_hypotheses (batch))``; hypothesis 0 is
            what ``decode`` returns, slots beyond ``num_hypotheses[b]`` are empty (length 0, score -inf).  After
            ``configure()``: ``CTCDecoder``'s ``NBestResults`` -- ``scores = ctc_scores + lmwt * lm_scores - wip * num_words +
            oov_penalty * num_oov_words``, ``ctc_scores`` what ``scores`` is without ``configure()``, ``timesteps`` ``None``
            unless asked for
        """
        if timesteps and not self._decoder.configured:
            raise ValueError("timesteps are a field of NBestResults, which a configured decoder returns: call configure(wip=0) "
                             "for the same search with timesteps")
        logits, logits_lengths = self._batch_major(self._logprobs(logits), logits_lengths)
        r = self._decoder.decode_nbest(logits_=logits, logits_lengths_=logits_lengths, nbest=nbest, timesteps=timesteps)
        return NBestResults(*r) if self._decoder.configured else GramNBestResults(*r)

    def open_stream(self, batch_size, max_frames, device=None, timesteps=False):
        """Streaming beam search (``beam_width > 1``): a ``GramCTCDecoderStream`` that is fed the logits in chunks and keeps
        the beams of ``batch_size`` utterances of up to ``max_frames`` frames on the GPU in between.  After every chunk the
        result is that of ``decode`` / ``decode_nbest`` on everything fed so far; the decoder's settings at this moment --
        ``configure()`` and ``restrict_to_vocabulary()`` included -- are the stream's.

        :param device: the GPU of the state; by default that of the first chunk
        :param timesteps: after ``configure()`` only: ``feed_nbest`` returns the frames of the ids, counted from the stream's
            start, unless told otherwise per call
        """
        if self._beam_width == 1:
            raise CTCDecoderError("a stream needs beam_width > 1: greedy decoding has no beam to keep")
        try:
            return GramCTCDecoderStream(self, self._decoder.open_stream(batch_size, max_frames, device=device, timesteps=timesteps))
        except ValueError as e:
            raise CTCDecoderError(str(e))


class GramCTCDecoderStream(_DecoderStream):
    """What ``GramCTCDecoder.open_stream`` returns: ``_DecoderStream`` (``CTCDecoderStream``'s surface), fed logits -- the
    log-softmax is per frame, so it is applied per chunk.  ``feed_nbest`` returns ``GramNBestResults``, after ``configure()``
    ``NBestResults``, and takes ``timesteps`` per read-out."""

    @property
    def _nbest_type(self):
        return NBestResults if self._stream.scored else GramNBestResults

    def _chunk(self, logits, logits_lengths):
        if logits.dim() != 3:
            raise ValueError("logits must be (batch, time, alphabet)")
        logits, logits_lengths = self._owner._batch_major(logits, logits_lengths)
        self._stream.check_chunk(tuple(logits.shape))             # (before any device work)
        return self._owner._logprobs(logits), logits_lengths

    def feed_nbest(self, logits, logits_lengths=None, nbest=None, timesteps=None):
        if timesteps and not self._stream.scored:
            raise ValueError("timesteps are a field of NBestResults, which a configured decoder returns: call configure(wip=0) "
                             "for the same search with timesteps")
        return self._read_out(logits, logits_lengths, nbest=nbest, timesteps=timesteps)
