"""CPU: what the pruned Gram-CTC search's GPU tests (tests/test_gpu_gram_cut.py) rest on -- the kept-loop restatement equals
the existing restatements on masked rows, the utterances left out of the comparison beyond the unpruned width limit are
recomputed and held to the cap, the decoder's constructor checks, and the width and workspace queries, which need no GPU."""
import math

import numpy as np
import pytest

import gram_cut_ref as CR
import gram_decode_lm_ref as LR
import gram_decode_ref as DR
import gram_ref as GR

CAP = 131072


def decoder(V, width, **kw):
    from end2end_amd.decoders import GramCTCDecoder
    R, l2i = (6, {}) if V == 6 else CR.eq_table(V) if V in CR.EQ_V else (CR.WIDE["R"], CR.wide_table())
    return GramCTCDecoder(0, R, V, l2i, beam_width=width, labels=CR.LABELS, after_logsoftmax=True, **kw)


# ---- the restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", CR.EQ_V)
def test_kept_loop_equals_the_restatement_on_masked_rows(V):
    """The masses exactly and the same hypotheses in the same order: an absent addend and an addend of exactly 0 are one sum."""
    R, l2i = CR.eq_table(V)
    grams = GR.grams_of(R, V, l2i)
    lp, lens = CR.eq_input(V)
    blank_alone = 0
    for top_n, prob, W in ((1, 1.0, 8), (3, 0.9, 2), (12, 0.5, 8), (12, 1.0, 32)):
        for b, n in enumerate(lens):
            x = lp[b, :n].astype(np.float64)
            got, _, _ = CR.beam_search(x, grams, top_n, prob, W)
            want, _ = DR.beam_search(CR.masked(x, top_n, prob), grams, W)
            assert got == want, (V, top_n, prob, W, b)
            blank_alone += sum(1 for t in range(n) if CR.LC.cut_frame(x[t], 0, top_n, prob) == [0])
    assert blank_alone > 0                       # cutoff_top_n = 1 with the blank as the arg-max


@pytest.mark.parametrize("with_lm", [False, True])
def test_kept_loop_equals_the_scored_restatement_on_masked_rows(with_lm):
    V = 40
    R, l2i = CR.eq_table(V)
    grams = GR.grams_of(R, V, l2i)
    lp, lens = CR.eq_input(V)
    fields = lambda: LR.Fields(CR.LABELS, LR.oracle_lm(CR.MODEL) if with_lm else None, True, **(CR.KNOBS if with_lm else dict(wip=0.4)))
    for top_n, prob, W in ((3, 1.0, 8), (12, 0.9, 8)):
        for b, n in enumerate(lens):
            x = lp[b, :n].astype(np.float64)
            got, _, _ = CR.beam_search(x, grams, top_n, prob, W, fields())
            want, _ = LR.beam_search(CR.masked(x, top_n, prob), grams, fields(), W)
            assert got == want, (with_lm, top_n, prob, W, b)


def test_no_pruning_is_the_restatement():
    R, l2i = CR.eq_table(40)
    grams = GR.grams_of(R, 40, l2i)
    lp, lens = CR.eq_input(40)
    x = lp[0].astype(np.float64)
    assert CR.beam_search(x, grams, 40, 1.0, 8)[0] == DR.beam_search(x, grams, 8)[0]
    assert CR.beam_search(x, grams, None, 1.0, 8)[0] == DR.beam_search(x, grams, 8)[0]


# ---- the utterances left out beyond the unpruned width limit -------------------------------------------------------------------
def test_left_out_utterances_are_the_listed_ones_and_within_the_cap():
    out, total = CR.wide_left_out()
    assert tuple(out) == tuple(CR.LEFT_OUT), out
    assert total == 8 and len(out) <= CR.LEFT_OUT_CAP * total
    assert CR.WIDE["W"] > min(128, CAP // CR.WIDE["V"]) == 64       # beyond the unpruned limit
    for prob in CR.WIDE_PROBS:
        for with_lm in (False, True):
            ref = CR.wide_reference(prob, with_lm)
            assert all(len(r[0]) == CR.WIDE["W"] for r in ref)       # the beam is full: the cut decides
            assert all(math.isinf(r[2]) for r in ref) == (prob == 1.0)


# ---- the constructor --------------------------------------------------------------------------------------------------------------
def test_constructor_takes_ctc_decoders_knobs_and_refuses_what_it_refuses():
    from end2end_amd.decoders import CTCDecoder, GramCTCDecoder
    from end2end_amd.decoders.ctc_decoder import CTCDecoderError
    d = decoder(40, 8, cutoff_top_n=3, cutoff_prob=0.9)
    assert d._decoder._cut() == (3, 0.9)
    d.configure(wip=0.4)
    assert d._decoder._cut() == (3, 0.9)                              # configure() keeps the knobs (restrict_to_vocabulary: GPU test)
    assert decoder(40, 8)._decoder._cut() is None
    assert decoder(40, 8, cutoff_top_n=40)._decoder._cut() is None    # no less than the table: nothing is pruned
    assert decoder(40, 8, cutoff_top_n=400, cutoff_prob=0.5)._decoder._cut() == (400, 0.5)   # (K = min(cutoff_top_n, V) is the library's)
    for kw, text in ((dict(cutoff_top_n=0), "cutoff_top_n must be an integer >= 1"),
                     (dict(cutoff_top_n=2.5), "cutoff_top_n must be an integer >= 1"),
                     (dict(cutoff_top_n=True), "cutoff_top_n must be an integer >= 1"),
                     (dict(cutoff_prob=0.0), r"cutoff_prob must be in \(0, 1\]"),
                     (dict(cutoff_prob=1.5), r"cutoff_prob must be in \(0, 1\]"),
                     (dict(cutoff_prob="0.5"), r"cutoff_prob must be in \(0, 1\]")):
        with pytest.raises(CTCDecoderError, match=text):
            decoder(40, 8, **kw)
        with pytest.raises(CTCDecoderError, match=text):              # CTCDecoder's texts
            CTCDecoder(beam_width=8, labels=CR.LABELS, **kw)
    for kw in (dict(cutoff_top_n=3), dict(cutoff_prob=0.5)):
        with pytest.raises(CTCDecoderError, match="need beam_width > 1: greedy decoding expands nothing"):
            decoder(40, 1, **kw)
    assert decoder(40, 1)._decoder.beam_width == 1


def test_width_limit_is_the_pruned_one_when_the_decoder_prunes():
    from end2end_amd.decoders import GramCTCDecoder
    from end2end_amd.decoders.ctc_decoder import CTCDecoderError
    l2i = {c: [1 + c % 28, 1 + (c // 28) % 28, 1 + (c // 784) % 28] for c in range(29, 8000)}
    d = GramCTCDecoder(total_labels=8000, num_base_labels=29, label2ids=l2i, beam_width=100, cutoff_top_n=40)
    assert d._decoder._cut() == (40, 1.0)
    with pytest.raises(ValueError, match="beam_width 100 is not supported for a Gram-CTC table of 8000 columns"):
        GramCTCDecoder(total_labels=8000, num_base_labels=29, label2ids=l2i, beam_width=100)          # as today
    with pytest.raises(CTCDecoderError, match="a pruned frame keeps at most 1024 labels"):
        GramCTCDecoder(total_labels=8000, num_base_labels=29, label2ids=l2i, beam_width=16, cutoff_prob=0.5)
    with pytest.raises(CTCDecoderError, match="with cutoff_top_n=1024: 1 to 127"):
        GramCTCDecoder(total_labels=8000, num_base_labels=29, label2ids=l2i, beam_width=128, cutoff_top_n=1024)


# ---- the queries ------------------------------------------------------------------------------------------------------------------
def test_cut_max_width():
    from end2end_amd import _lib
    L = _lib.load()
    for V in (29, 379, 2048, 8000):
        for top_n in (40, 1023):
            want = min(128, CAP // (min(top_n, V) + 1))
            assert L.e2e_gram_beam_cut_max_width(V, 3, top_n) == want == 128, (V, top_n)
    assert L.e2e_gram_beam_cut_max_width(8000, 3, 1024) == 127 and L.e2e_gram_beam_cut_max_width(8000, 3, 8000) == 16
    assert L.e2e_gram_beam_cut_max_width(29, 3, 1023) == L.e2e_gram_beam_max_width(29, 3) == 128
    assert L.e2e_gram_beam_cut_max_width(0, 3, 40) == 0 and L.e2e_gram_beam_cut_max_width(29, 9, 40) == 0
    assert L.e2e_gram_beam_cut_max_width(29, 3, 0) == 0


def test_workspace_queries_are_zero_exactly_where_the_calls_refuse():
    from end2end_amd import _lib
    L = _lib.load()
    q, qs, qr = L.e2e_gram_beam_cut_workspace_bytes, L.e2e_gram_beam_cut_stream_workspace_bytes, L.e2e_gram_beam_cut_stream_row_bytes
    B, T, K = 64, 256, 3
    for scored, with_lm in ((0, 0), (1, 0), (1, 1)):
        assert q(B, T, 8000, K, 100, scored, with_lm, 40) > 0 and qs(B, T, 8000, K, 100, scored, with_lm, 40) > 0
        assert q(B, T, 8000, K, 128, scored, with_lm, 1023) > 0
        assert q(B, T, 8000, K, 128, scored, with_lm, 1024) == 0          # the width limit at K = 1024 is 127
        assert q(B, T, 8000, K, 16, scored, with_lm, 1025) == 0           # K > e2e_ctc_label_cut_max()
        assert q(B, T, 8000, K, 16, scored, with_lm, 0) == 0 and q(B, 0, 8000, K, 16, scored, with_lm, 40) == 0
        assert q(B, T, 8000, 9, 16, scored, with_lm, 40) == 0 and q(B, T, 8000, K, 0, scored, with_lm, 40) == 0
        assert qs(B, T, 8000, K, 128, scored, with_lm, 1024) == 0 and qs(B, T, 8000, K, 16, scored, with_lm, 1025) == 0
        assert qr(100, 8000, K, 100, scored, with_lm, 40) == L.e2e_gram_beam_stream_row_bytes(100, 379, K, 100, scored, with_lm) > 0
        assert qr(100, 8000, K, 100, scored, with_lm, 1025) == 0 and qr(100, 8000, K, 128, scored, with_lm, 1024) == 0
    assert q(B, T, 8000, K, 16, 0, 1, 40) == 0                            # with_lm without scored
    # no answer rows and W * (K + 1) pairs: smaller than the unpruned query at V = 8000, at its width and at 100
    plain = L.e2e_gram_beam_workspace_bytes_lm(B, T, 8000, K, 16, 1)
    assert 0 < q(B, T, 8000, K, 16, 1, 1, 40) < q(B, T, 8000, K, 100, 1, 1, 40) < plain
    assert 0 < q(B, T, 8000, K, 16, 0, 0, 40) < L.e2e_gram_beam_workspace_bytes(B, T, 8000, K, 16)
    # cutoff_top_n >= V may be the unpruned call (cutoff_prob == 1): no less than its query
    assert q(2, 24, 40, K, 8, 1, 1, 40) >= L.e2e_gram_beam_workspace_bytes_lm(2, 24, 40, K, 8, 1)
    assert qs(2, 24, 40, K, 8, 1, 1, 40) >= L.e2e_gram_beam_stream_workspace_bytes(2, 40, K, 8, 1, 1)


def test_argument_errors_are_found_before_any_launch():
    """No GPU here: a call that got as far as a launch would fail on that, with another code."""
    from end2end_amd import _lib
    L = _lib.load()
    ARG, UNSUPPORTED = -1, -2

    def nbest(V, W, top_n, prob, scored=0):
        return L.e2e_gram_ctc_beam_nbest_cut(256, _lib.F32, 24 * V, V, 1, 256, 1, 24, V, 256, 256, 3, 6, W, scored, -1, None, 0.0, 0.0,
                                             0.0, 1, 256, 72, 256, 256, 256, 256 if scored else None, 256, 1 << 30, None, None, top_n, prob)

    def stream(V, W, top_n, prob):
        return L.e2e_gram_ctc_beam_stream_cut(256, _lib.F32, 24 * V, V, 1, 256, 1, 24, V, 256, 256, 3, 6, W, 0, -1, None, 0.0, 0.0, 0.0,
                                              256, 1 << 20, 100, 1, 256, 72, 256, 256, 256, None, 256, 256, 1 << 30, None, None, top_n, prob)
    for call in (nbest, stream):
        assert call(300, 8, 0, 1.0) == ARG and call(300, 8, -3, 0.5) == ARG
        assert call(300, 8, 3, 0.0) == ARG and call(300, 8, 3, 1.5) == ARG and call(300, 8, 3, float("nan")) == ARG
        assert call(2000, 8, 2000, 0.5) == UNSUPPORTED                    # K = 2000 > 1024
        assert call(8000, 128, 1024, 1.0) == UNSUPPORTED                  # the width limit at K = 1024 is 127
        assert call(8000, 129, 40, 1.0) == UNSUPPORTED
        assert call(8000, 100, 8000, 1.0) == UNSUPPORTED                  # no pruning: the unpruned entry's limit, 16
