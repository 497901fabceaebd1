"""CTCDecoder wrapper with the reference's constructor, defaults and return type
(pytorch_end2end/decoders/ctc_decoder.py:25-149).  The inputs stay on the GPU instead of being copied to
the host (`.cpu()` at :100,:137 upstream); the results are CPU tensors as upstream unless
``keep_on_device=True`` (an extension: ids and lengths then stay on the GPU that decoded them).
"""
import os
from collections import namedtuple

import torch

from ..engines import CTCDecoderEngine


class CTCDecoderError(Exception):
    pass


DecoderResults = namedtuple("DecoderResults", ["decoded_targets", "decoded_targets_lengths", "decoded_sentences"])

# decode_nbest(): (B, N, ...) per utterance and hypothesis, ranked by `scores`; `decoded_sentences[b]` lists the
# num_hypotheses[b] sentences of utterance b; `timesteps` is None unless asked for
NBestResults = namedtuple("NBestResults", ["decoded_targets", "decoded_targets_lengths", "decoded_sentences", "scores",
                                           "ctc_scores", "lm_scores", "num_words", "num_oov_words", "num_hypotheses",
                                           "timesteps"])


def read_lexicon(lexicon):
    """The words of a lexicon, in order and once each: from an iterable of entries, or from the text file at a path with
    one entry per line.  Of every entry the first white-space separated token counts; empty lines are skipped."""
    if isinstance(lexicon, (str, bytes, os.PathLike)):
        path = os.fsdecode(lexicon)
        if not os.path.isfile(path):
            raise CTCDecoderError("Can't find a lexicon: {}".format(path))
        with open(path, encoding="utf-8") as f:
            entries = f.read().splitlines()
    else:
        entries = [str(e) for e in lexicon]
    words = list(dict.fromkeys(e.split()[0] for e in entries if e.split()))
    if not words:
        raise CTCDecoderError("the lexicon is empty")
    return words


class CTCDecoder:
    """
    :param beam_width: number of hypotheses kept; ``1`` means greedy (argmax) decoding
    :param after_logsoftmax: inputs are log-probabilities (greedy ignores this)
    :param blank_idx: index of the blank label
    :param time_major: inputs are ``(time, batch, alphabet)``
    :param labels: label strings including the blank, e.g. ``["_", "a", "b", " "]``
    :param lm_path: ARPA (optionally gzipped) language model
    :param lmwt: language-model weight
    :param wip: word insertion penalty
    :param oov_penalty: penalty per out-of-vocabulary word
    :param case_sensitive: look words up in the language model with their case
    :param keep_on_device: (extension) leave the decoded ids and lengths on the GPU
    :param restrict_to_vocabulary: (extension) with ``lm_path``: the beam search only forms words of the language
        model's vocabulary (the last word of a result may still be an unfinished prefix of one)
    :param lexicon: (extension) restrict the beam search to these words without a language model: an iterable of words,
        or the path of a text file with one entry per line whose first white-space separated token is the word (so a
        pronunciation dictionary works).  ``lmwt`` and ``oov_penalty`` then count as 0; ``wip`` applies.
    :param transcriptions: (extension) custom transcriptions for models whose labels do not spell the words letter by
        letter (phonemes, word pieces, multi-character labels): the path of a text file with one entry ``word tok tok ...``
        per line, a mapping ``word -> tokens`` (or ``-> [tokens, tokens, ...]`` for variants), or an iterable of
        ``(word, tokens)``; every token is one of ``labels``, neither the blank nor the space.  A word is then found by its
        sequence of labels; of several words with one transcription (homophones) the language model picks the likeliest in
        its context.  Goes with ``lm_path`` (entries whose word the model does not list are dropped, with a warning) or
        alone (nothing is scored, the first listed homophone wins), and with ``restrict_to_vocabulary=True``.
        ``decoded_sentences`` are the chosen words joined by single spaces, ``<unk>`` for a piece that is no word.
    :param cutoff_top_n: (extension) per-frame label pruning: a frame expands at most this many labels, the likeliest
        (ties to the lower id), and the blank.  ``None`` or a value that is no less than the alphabet: no limit.  At most
        1024 labels can be kept; needs ``beam_width > 1``.
    :param cutoff_prob: (extension) ... and of those the fewest whose probabilities sum to this, in ``(0, 1]``; ``1.0``: all.
        With both at their defaults the decoder is the unpruned one.
    """

    def __init__(self, beam_width=100, after_logsoftmax=False, blank_idx=0, time_major=False, labels=None,
                 lm_path=None, lmwt=1.0, wip=1.0, oov_penalty=-10, case_sensitive=True, keep_on_device=False,
                 restrict_to_vocabulary=False, lexicon=None, transcriptions=None, cutoff_top_n=None, cutoff_prob=1.0):
        self._beam_width = beam_width
        self._blank_idx = blank_idx
        self._after_logsoftmax = after_logsoftmax
        self._labels = labels or []
        self._lm_path = os.path.abspath(lm_path) if lm_path else ""
        self._lmwt = lmwt
        self._wip = wip
        self._oov_penalty = oov_penalty
        self._time_major = time_major
        self._case_sensitive = case_sensitive
        self._restrict = bool(restrict_to_vocabulary) or lexicon is not None
        self._lexicon = lexicon
        self._transcriptions = transcriptions
        self._cutoff_top_n, self._cutoff_prob = cutoff_top_n, cutoff_prob
        self._check_params()
        # (a transcription model is loaded once, by configure: the engine's constructor would key it by spellings)
        self._decoder = CTCDecoderEngine(self._blank_idx, self._beam_width, self._labels,
                                         "" if transcriptions is not None else self._lm_path,
                                         self._lmwt, self._wip, self._oov_penalty, self._case_sensitive,
                                         keep_on_device=keep_on_device)
        cut = dict(cutoff_top_n=cutoff_top_n, cutoff_prob=cutoff_prob)
        if transcriptions is not None:
            try:
                self._decoder.configure(restrict_to_vocabulary=self._restrict, transcriptions=transcriptions,
                                        lm_path=self._lm_path or None, **cut)
            except ValueError as e:
                raise CTCDecoderError(str(e)) from e
        elif self._restrict or cutoff_top_n is not None or cutoff_prob != 1.0:
            try:
                self._decoder.configure(restrict_to_vocabulary=self._restrict, lexicon=self._lexicon, **cut)
            except ValueError as e:
                raise CTCDecoderError(str(e)) from e

    def _check_params(self):
        top_n, prob = self._cutoff_top_n, self._cutoff_prob
        if top_n is not None and (isinstance(top_n, bool) or int(top_n) != top_n or top_n < 1):
            raise CTCDecoderError("cutoff_top_n must be an integer >= 1 (or None), got {!r}".format(top_n))
        if not isinstance(prob, (int, float)) or not 0.0 < prob <= 1.0:
            raise CTCDecoderError("cutoff_prob must be in (0, 1], got {!r}".format(prob))
        if (top_n is not None or prob != 1.0) and self._beam_width == 1:
            raise CTCDecoderError("cutoff_top_n / cutoff_prob need beam_width > 1: greedy decoding expands nothing")
        if self._lm_path:
            # (upstream also tests `self._labels is None` here, which cannot hold after `labels or []`,
            # pytorch_end2end/decoders/ctc_decoder.py:53,69: a model without labels is accepted at construction;
            # decode() then fails because the alphabet cannot spell words)
            if not os.path.isfile(self._lm_path):
                raise CTCDecoderError("Can't find a model: {}".format(self._lm_path))
        if self._transcriptions is not None:
            if self._lexicon is not None:
                raise CTCDecoderError("lexicon together with transcriptions is not supported: restrict_to_vocabulary=True "
                                      "restricts the search to the transcriptions")
            if self._beam_width == 1:
                raise CTCDecoderError("transcriptions need beam_width > 1: greedy decoding forms no words")
            return
        if self._restrict:
            if self._lexicon is not None and self._lm_path:
                raise CTCDecoderError("lexicon together with lm_path is not supported: restrict_to_vocabulary=True "
                                      "uses the language model's own vocabulary")
            if self._lexicon is None and not self._lm_path:
                raise CTCDecoderError("restrict_to_vocabulary needs a vocabulary: lm_path or lexicon")
            if self._beam_width == 1:
                raise CTCDecoderError("a restricted search needs beam_width > 1: greedy decoding has no vocabulary")
            if self._lexicon is not None:
                self._lexicon = read_lexicon(self._lexicon)

    def _batch_major(self, logits, logits_lengths):
        if self._time_major:
            logits = logits.transpose(1, 0)
        logits = logits.detach()
        if not self._labels and self._beam_width > 1 and logits.dim() == 3:
            # (without labels the alphabet is known at the first call only: the pruning's limit is checked here)
            try:
                self._decoder.check_cut_limit(logits.shape[2], self._cutoff_top_n, float(self._cutoff_prob))
            except ValueError as e:
                raise CTCDecoderError(str(e)) from e
        if logits_lengths is None:
            logits_lengths = torch.full((logits.size(0),), logits.size(1), dtype=torch.int32, device=logits.device)
        return logits, logits_lengths

    def decode(self, logits, logits_lengths=None):
        """Prefix beam search (Hannun et al., 2014).  ``beam_width == 1`` routes to greedy decoding.

        :return: ``DecoderResults(decoded_targets (batch, longest), decoded_targets_lengths, decoded_sentences)``
        """
        if self._beam_width == 1:
            return self.decode_greedy(logits, logits_lengths)
        with torch.no_grad():
            if not self._after_logsoftmax:
                logits = torch.log_softmax(logits, -1)
        logits, logits_lengths = self._batch_major(logits, logits_lengths)
        return DecoderResults(*self._decoder.decode(logits_=logits, logits_lengths_=logits_lengths))

    def decode_nbest(self, logits, logits_lengths=None, nbest=None, timesteps=False):
        """The hypotheses the beam search ends with, best first (an extension: upstream returns the first only).

        :param nbest: how many to return per utterance, at most ``beam_width`` (the default)
        :param timesteps: also return, for every decoded label, the frame at which it entered the beam
        :return: ``NBestResults(decoded_targets (batch, nbest, longest), decoded_targets_lengths (batch, nbest),
            decoded_sentences (a list per utterance), scores, ctc_scores, lm_scores, num_words, num_oov_words
            (batch, nbest), num_hypotheses (batch), timesteps (batch, nbest, longest) or None)``;
            ``scores = ctc_scores + lmwt * lm_scores - wip * num_words + oov_penalty * num_oov_words``, hypothesis 0 is
            what ``decode`` returns, slots beyond ``num_hypotheses[b]`` are empty (length 0, score -inf).
        """
        if self._beam_width == 1:
            raise CTCDecoderError("decode_nbest needs beam_width > 1: greedy decoding has no beam")
        with torch.no_grad():
            if not self._after_logsoftmax:
                logits = torch.log_softmax(logits, -1)
        logits, logits_lengths = self._batch_major(logits, logits_lengths)
        return NBestResults(*self._decoder.decode_nbest(logits_=logits, logits_lengths_=logits_lengths, nbest=nbest,
                                                        timesteps=timesteps))

    def open_stream(self, batch_size, max_frames, device=None, timesteps=False):
        """Streaming beam search (an extension): a ``CTCDecoderStream`` that is fed the logits in chunks and keeps the beams of
        ``batch_size`` utterances of up to ``max_frames`` frames on the GPU in between.  After every chunk the result is that
        of ``decode`` / ``decode_nbest`` on everything fed so far; the decoder's settings apply as they do there.

        :param timesteps: keep the frames of the labels (``feed_nbest`` then returns them, counted from the stream's start)
        """
        if self._beam_width == 1:
            raise CTCDecoderError("a stream needs beam_width > 1: greedy decoding has no beam to keep")
        return CTCDecoderStream(self, self._decoder.open_stream(batch_size, max_frames, device=device, timesteps=timesteps))

    def transcribe(self, ids):
        """The words of a sequence of label ids as the search reads them: split at the space, every piece looked up by its
        labels, homophones chosen by the language model in the running context; ``<unk>`` for a piece that is no word.
        Needs ``transcriptions``."""
        lm = self._decoder.lm
        if lm is None or not lm.is_transcribed():
            raise CTCDecoderError("transcribe needs a decoder with transcriptions")
        return lm.transcribe([int(k) for k in ids if int(k) >= 0], self._decoder.space_id)

    def _print_scores_for_sentence(self, words):
        self._decoder.print_scores_for_sentence(words)

    def decode_greedy(self, logits, logits_lengths=None):
        """Greedy (argmax) decoding: works on raw logits or log-probabilities.

        :return: ``DecoderResults(decoded_targets (batch, time) zero padded, decoded_targets_lengths, decoded_sentences)``
        """
        logits, logits_lengths = self._batch_major(logits, logits_lengths)
        return DecoderResults(*self._decoder.decode_greedy(logits_=logits, logits_lengths_=logits_lengths))


class _DecoderStream:
    """What the decoders' ``open_stream`` return.  ``feed`` / ``feed_nbest`` take a chunk shaped as ``decode`` takes it
    (``logits_lengths``: the frames of this chunk per utterance, all by default, 0 allowed) and return ``DecoderResults`` /
    ``NBestResults`` for everything fed so far; ``frames`` are the per-utterance totals, ``state`` the (batch, row_bytes)
    uint8 tensor on the GPU that holds the beams, ``reset(rows=None)`` starts utterances anew.  A decoder's stream says how
    a chunk becomes what its engine's stream takes (``_chunk``)."""

    _nbest_type = NBestResults

    def __init__(self, decoder, stream):
        self._owner, self._stream = decoder, stream

    @property
    def frames(self):
        return self._stream.frames

    @property
    def state(self):
        return self._stream.state

    @property
    def row_bytes(self):
        return self._stream.row_bytes

    def reset(self, rows=None):
        self._stream.reset(rows)

    def feed(self, logits, logits_lengths=None):
        logits, logits_lengths = self._chunk(logits, logits_lengths)
        return DecoderResults(*self._stream.feed(logits, logits_lengths))

    def feed_nbest(self, logits, logits_lengths=None, nbest=None):
        return self._read_out(logits, logits_lengths, nbest=nbest)

    def _read_out(self, logits, logits_lengths, **read_out):
        logits, logits_lengths = self._chunk(logits, logits_lengths)
        r = self._stream.feed_nbest(logits, logits_lengths, **read_out)
        return None if r is None else self._nbest_type(*r)


class CTCDecoderStream(_DecoderStream):
    """What ``CTCDecoder.open_stream`` returns: ``_DecoderStream``, fed logits; the log-softmax is per frame, so it is applied
    per chunk."""

    def _chunk(self, logits, logits_lengths):
        d = self._owner
        logits, logits_lengths = d._batch_major(logits, logits_lengths)
        self._stream.check_chunk(tuple(logits.shape))             # (before any device work)
        with torch.no_grad():
            if not d._after_logsoftmax:
                logits = torch.log_softmax(logits, -1)            # per frame: the same numbers whatever the chunking
        return logits, logits_lengths
