"""CPU: per-frame label pruning (cutoff_top_n, cutoff_prob) -- the restatement's own properties, the argument errors of the
Python layer and of the C ABI (found before any launch), the workspace queries, and which frames and utterances the GPU tests
(tests/test_gpu_label_cut.py, tests/test_gpu_ctc_beam_cut.py) leave out, recomputed and held to the cap."""
import numpy as np
import pytest

import ctc_beam_fuzz_util as F
import label_cut_ref as LC
import lexicon_ref as LR

ERR_ARG, ERR_UNSUPPORTED = -1, -2


# ---- the restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_keep_everything_cut_is_the_unpruned_search(seed):
    rng = np.random.default_rng(73000 + seed)
    V, W, T = (4, 7, 12)[seed % 3], (2, 5)[seed % 2], 9
    labels = F.AF.plain_labels(V, 1 if seed % 2 else -1)
    lp = F.emissions(rng, 1, T, V, 2.0, seed == 3, "f32")[0].astype(np.float64)
    blank = (0, V - 1)[seed % 2]
    want = LR.Search(labels, blank, W, wip=0.4).run(lp, T)
    for top_n in (V, V + 5, None):
        got = LC.CutSearch(labels, blank, W, wip=0.4).set_cut(top_n, 1.0).run(lp, T)
        assert got == want, (seed, top_n)
    pruned = LC.CutSearch(labels, blank, W, wip=0.4).set_cut(1, 1.0).run(lp, T)
    assert pruned != want or V <= 2


def test_restatement_properties():
    rng = np.random.default_rng(73100)
    for V in (2, 5, 29, 65):
        lp = F.GF.log_softmax32(rng.standard_normal((40, V)).astype(np.float32)).astype(np.float64)
        lp[0] = lp[0, 0]                                                 # an all-equal row: ties by id
        for top_n in (1, 2, 40):
            for prob in LC.CUT_PROBS:
                for blank in (0, V - 1):
                    K = min(top_n, V)
                    for t in range(len(lp)):
                        kept = LC.cut_frame(lp[t], blank, top_n, prob)
                        assert blank in kept and 1 <= len(kept) <= K + 1
                        assert kept == sorted(set(kept))
                        if prob == 1.0:
                            assert len(kept) in (K, K + 1) and LC.boundary_margin(lp[t], top_n, prob) == np.inf
                        rest = [c for c in kept if c != blank]
                        out = [c for c in range(V) if c not in kept]
                        if rest and out:
                            assert min(lp[t][rest]) >= max(lp[t][out])  # nothing kept but the blank is below something dropped
                    assert LC.cut_frame(lp[0], blank, top_n, 1.0) == sorted(set(range(K)) | {blank})     # ties: the lower ids
    # ties by id: of bit-equal columns the lower ids are taken
    assert LC.cut_frame([-1.0, -1.0, -1.0, -1.0], 3, 2, 1.0) == [0, 1, 3]
    assert LC.cut_frame([-2.0, -1.0, -1.0, -1.0], 0, 2, 1.0) == [0, 1, 2]
    # NaN counts as -inf; the blank uses none of the K places; cutoff_prob stops at the first sum that reaches it
    assert LC.cut_frame([np.nan, -1.0, -3.0], 2, 1, 1.0) == [1, 2]
    assert LC.cut_frame(np.log([0.5, 0.3, 0.2]), 2, 3, 0.5) == [0, 2]
    assert LC.cut_frame(np.log([0.5, 0.3, 0.2]), 2, 3, 0.75) == [0, 1, 2]
    assert LC.cut_frame(np.log([0.5, 0.3, 0.2]), 0, 1, 0.99) == [0]
    assert LC.boundary_margin(np.log([0.5, 0.25, 0.25]), 3, 0.5) == 0.0


# ---- argument errors ---------------------------------------------------------------------------------------------------------
def test_python_layer_argument_errors():
    from end2end_amd import CTCDecoder, CTCDecoderError
    from end2end_amd.engines import CTCDecoderEngine
    labels = ["_", "a", "b", " "]
    for kw in (dict(cutoff_top_n=0), dict(cutoff_top_n=-3), dict(cutoff_prob=0.0), dict(cutoff_prob=1.5), dict(cutoff_prob=-0.1)):
        with pytest.raises(CTCDecoderError, match="cutoff"):
            CTCDecoder(beam_width=4, labels=labels, **kw)
    for kw in (dict(cutoff_top_n=2), dict(cutoff_prob=0.9)):
        with pytest.raises(CTCDecoderError, match="greedy"):
            CTCDecoder(beam_width=1, labels=labels, **kw)
    wide = [str(i) for i in range(LC.CUT_MAX + 10)]
    with pytest.raises(CTCDecoderError, match="at most %d" % LC.CUT_MAX):
        CTCDecoder(beam_width=4, labels=wide, cutoff_prob=0.9)           # K = V above the limit
    with pytest.raises(CTCDecoderError, match="at most %d" % LC.CUT_MAX):
        CTCDecoder(beam_width=4, labels=wide, cutoff_top_n=LC.CUT_MAX + 1)
    CTCDecoder(beam_width=4, labels=wide, cutoff_top_n=LC.CUT_MAX, cutoff_prob=0.9)
    # today's decoder: None, or no less than the alphabet, with cutoff_prob 1
    for kw in (dict(), dict(cutoff_top_n=None), dict(cutoff_top_n=4), dict(cutoff_top_n=100, cutoff_prob=1.0)):
        assert CTCDecoder(beam_width=4, labels=labels, **kw)._decoder._cut(4) is None
    assert CTCDecoder(beam_width=4, labels=labels, cutoff_top_n=3)._decoder._cut(4) == (3, 1.0)
    assert CTCDecoder(beam_width=4, labels=labels, cutoff_prob=0.5)._decoder._cut(4) == (4, 0.5)
    # the engine: configure() more than once, each call sets everything
    e = CTCDecoderEngine(0, 4, labels)
    assert e.configure(cutoff_top_n=2)._cut(4) == (2, 1.0) and e.configure()._cut(4) is None
    with pytest.raises(ValueError, match="cutoff_top_n"):
        e.configure(cutoff_top_n=0)
    with pytest.raises(ValueError, match="cutoff_prob"):
        e.configure(cutoff_prob=2.0)
    with pytest.raises(ValueError, match="greedy"):
        CTCDecoderEngine(0, 1, labels).configure(cutoff_top_n=2)


def test_c_abi_argument_errors_come_before_any_launch():
    from end2end_amd import _lib
    L = _lib.load()
    assert L.e2e_ctc_label_cut_max() == LC.CUT_MAX
    p = 256                                                              # (never dereferenced: every call below is refused)

    def cut(dtype=_lib.F32, B=1, T=2, V=5, blank=0, top_n=2, prob=1.0, lp=p, xl=p, ids=p, n=p):
        return L.e2e_ctc_label_cut(lp, dtype, T * V, V, 1, xl, B, T, V, blank, top_n, prob, ids, n, None, 0, None)
    for kw in (dict(dtype=9), dict(B=-1), dict(T=0), dict(V=0), dict(blank=-1), dict(blank=5), dict(top_n=0), dict(prob=0.0),
               dict(prob=1.0000001), dict(prob=float("nan")), dict(lp=None), dict(xl=None), dict(ids=None), dict(n=None)):
        assert cut(**kw) == ERR_ARG, kw
        assert L.e2e_last_error()
    assert cut(V=5000, top_n=1025) == ERR_UNSUPPORTED and cut(V=5000, top_n=5000, prob=0.5) == ERR_UNSUPPORTED
    assert cut(B=0) == 0                                                 # nothing to do, nothing launched

    def beam(top_n=2, prob=1.0, W=4, nbest=1, V=5, blank=0):
        return L.e2e_ctc_beam_nbest_cut(p, _lib.F32, 2 * V, V, 1, p, 1, 2, V, blank, W, -1, None, 0.0, 0.0, 0.0, nbest, p, 3, p, p,
                                        p, p, None, None, 0, None, None, top_n, prob)
    for kw in (dict(top_n=0), dict(prob=0.0), dict(prob=2.0), dict(nbest=5), dict(blank=7), dict(W=100000)):
        assert beam(**kw) == ERR_ARG, kw
    assert beam(V=5000, top_n=2000, W=2) == ERR_UNSUPPORTED
    assert beam() == -3                                                  # E2E_ERR_WORKSPACE: the last check before the launches

    def stream(top_n=2, prob=1.0, row_bytes=0):
        return L.e2e_ctc_beam_stream_cut(p, _lib.F32, 10, 5, 1, p, 1, 2, 5, 0, 4, -1, None, 0.0, 0.0, 0.0, p, row_bytes, 8, 0, 1,
                                         p, 9, p, p, p, p, None, p, None, 0, None, None, top_n, prob)
    assert stream(top_n=0) == ERR_ARG and stream(prob=0.0) == ERR_ARG and stream() == ERR_ARG     # (row_bytes too small)
    assert stream(row_bytes=L.e2e_ctc_beam_stream_row_bytes(8, 5, 4, 0, 0)) == -3


def test_workspace_queries():
    from end2end_amd import _C
    assert _C.ctc_label_cut_workspace_bytes(2, 16, 8000, 40) > 0
    for lm in (False, True):
        for ts in (False, True):
            last = 0
            for top_n in (1, 2, 40, 100, 1024):
                n = _C.ctc_beam_cut_workspace_bytes(16, 256, 8000, 100, lm, ts, top_n)
                assert n >= last > 0 or (last == 0 and n > 0)            # positive, monotone in cutoff_top_n
                last = n
        last = 0
        for top_n in (1, 40, 1024):
            n = _C.ctc_beam_cut_stream_workspace_bytes(16, 32, 8000, 100, lm, top_n)
            assert n > last
            last = n
        assert _C.ctc_beam_cut_stream_workspace_bytes(16, 64, 8000, 100, lm, 40) > _C.ctc_beam_cut_stream_workspace_bytes(16, 32, 8000, 100, lm, 40)
    # pruned, with a model, V = 8000, W = 100: far below the unpruned query (no LM answer rows, K + 2 keys per member, not V + 1)
    pruned = _C.ctc_beam_cut_workspace_bytes(16, 256, 8000, 100, True, False, 40)
    plain = _C.ctc_beam_nbest_workspace_bytes(16, 256, 8000, 100, True, False)
    assert pruned < plain / 10
    # cutoff_top_n >= V may be the unpruned call (cutoff_prob == 1): the query covers it
    assert _C.ctc_beam_cut_workspace_bytes(2, 10, 29, 8, True, True, 29) >= _C.ctc_beam_nbest_workspace_bytes(2, 10, 29, 8, True, True)
    assert _C.ctc_beam_cut_max_width(8000, True) >= 100 and _C.ctc_beam_cut_max_width(29, False) >= 100
    assert _C.ctc_beam_cut_workspace_bytes(1, 1, 5, 2, False, False, 0) == 0


# ---- what the GPU tests leave out --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", LC.CUT_V)
def test_frames_left_out_of_the_selection_test(V):
    for dtype in LC.CUT_DTYPES:
        out, frames = LC.cut_left_out(V, dtype)
        assert sorted(out) == sorted(LC.LEFT_OUT_FRAMES.get((V, dtype), ())), (V, dtype, out)
        assert len(out) <= LC.LEFT_OUT_CAP * frames, (V, dtype, len(out), frames)
        assert not [o for o in out if o[1] == 1.0]                       # cutoff_prob == 1 compares no sum: nothing left out


def test_random_frames_are_not_near_a_boundary():
    """Randn logits at scales 1 and 4 through an f32 or f16 log-softmax: no frame within BOUNDARY of any cutoff_prob, so the
    cap above is not what makes the selection test pass (the frames left out are constructed rows)."""
    rng = np.random.default_rng(73200)
    near = frames = 0
    for V in (5, 29, 257):
        for scale in (1.0, 4.0):
            for dtype in ("f32", "f16"):
                lp = F.rounded(F.GF.log_softmax32((rng.standard_normal((64, V)) * scale).astype(np.float32)), dtype).astype(np.float64)
                for prob in LC.CUT_PROBS:
                    for t in range(len(lp)):
                        frames += 1
                        near += LC.boundary_margin(lp[t], 40, prob) < LC.BOUNDARY
    assert near == 0 and frames == 3 * 2 * 2 * 6 * 64


@pytest.mark.parametrize("variant", LC.VARIANTS)
def test_utterances_left_out_of_the_search_test(variant):
    out, total = LC.search_left_out(variant)
    assert tuple(out) == tuple(LC.LEFT_OUT_UTTS[variant]), (variant, out)
    assert len(out) <= LC.LEFT_OUT_CAP * total, (variant, len(out), total)
    assert total == sum(len(LC.SEARCH_SHAPE[V][2]) for V in LC.SEARCH_V) * len(LC.SEARCH_W) * 4
    # the cases reach what they are for: beams that fill and are cut, words that form, homophones
    full = words = 0
    for V, W, ci in LC.search_cases(variant):
        for ranking, _, _ in LC.search_reference(variant, V, W, ci):
            full += len(ranking) == W
            words += any(r["words"] > 0 for r in ranking)
    assert full >= total // 3 and words >= total // 3, (variant, full, words, total)
