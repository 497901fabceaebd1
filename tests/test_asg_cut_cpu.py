"""No GPU: the cases and the restatement of ASGDecoder's per-frame label pruning (tests/asg_cut_ref.py), the Python surface and
the host side of e2e_asg_beam_nbest_cut / e2e_asg_beam_stream_cut.

1. The kept-loop restatement equals the plain restatement on -inf-masked emissions, exactly: the definition's CONSEQUENCE, on
   every case tests/test_gpu_asg_cut.py holds to a restatement and on the tied, NaN and restricted ones beside them.
2. The margins of those cases: what is left out of the GPU comparison is asg_cut_ref.LEFT_OUT, within LEFT_OUT_CAP.
3. ASGDecoder.prune / ASGBeamEngine.prune: texts, signature, configure() drops the setting, the pinned signatures.
4. With the library built: the four symbols, typed from the header, and the queries' zeros."""
import inspect
import math

import numpy as np
import pytest

import asg_cut_ref as CR


# ---- 1. the consequence, in the restatement -------------------------------------------------------------------------------------------
def same_rankings(a, b, what):
    assert len(a) == len(b), what
    for u, v in zip(a, b):
        assert [h["ids"] for h in u] == [h["ids"] for h in v], what
        for g, w in zip(u, v):
            for k in ("total", "ac", "lm", "words", "oov"):
                assert g[k] == w[k], (what, k, g, w)                       # exactly: the same operations in the same order
            if "frames" in g and "frames" in w:
                assert g["frames"] == w["frames"], what


EXACT = [(shape, inst, "randn") for shape, inst in CR.ORACLE] + \
        [(0, "lex_lm", "randn"), (1, "lex_words", "randn"), (0, "wip", "half"), (3, "plain", "half"), (3, "lm", "randn"),
         (4, "plain", "nan"), (4, "lex_words", "half"), (1, "plain", "nan")]


@pytest.mark.parametrize("shape,inst,kind", EXACT)
def test_kept_loop_equals_the_plain_restatement_on_masked_emissions(shape, inst, kind):
    x, A, lens = CR.case(shape, kind)
    K = CR.SHAPES[shape][5]
    x64 = x.astype(np.float64)
    At = A.tolist() if A is not None else None
    kept, _ = CR.run_all(CR.search_of(shape, inst, K), x64.tolist(), At, lens)
    plain, _ = CR.run_all(CR.search_of(shape, inst), CR.masked(x64, K).tolist(), At, lens)
    same_rankings(kept, plain, (shape, inst, kind))
    T = CR.SHAPES[shape][1]
    assert all(not r for r, n in zip(kept, lens) if not 1 <= n <= T)
    if kind == "randn" and inst in ("plain", "lm"):
        assert any(len(r) > 0 for r in kept)


def test_the_selection():
    k = CR.kept_of
    assert k([0.5, 2.0, 0.5, 2.0, -1.0], 3) == [0, 1, 3]                   # ties: the lower id
    assert k([0.5, 2.0, 0.5, 2.0, -1.0], 1) == [1]
    assert k([float("nan"), -math.inf, -5.0], 2) == [0, 2]                 # NaN counts as -inf: behind -5, before label 1 by id
    assert k([-0.0, 0.0, 0.0], 2) == [0, 1]                                # -0 and +0 are one number
    assert k([1.0, 2.0], 5) == [0, 1]                                      # K = min(cutoff_top_n, V)
    m = CR.masked(np.array([[1.0, 3.0, 2.0]]), 2)
    assert m.tolist() == [[-math.inf, 3.0, 2.0]]
    x, _, _ = CR.case(0, "half")
    K = CR.SHAPES[0][5]
    tied = sum(1 for row in x.reshape(-1, x.shape[-1]) if sorted(row, reverse=True)[K - 1] == sorted(row, reverse=True)[K])
    assert tied > 10                                                       # the K-th place is tied in many frames of `half`


def test_a_member_whose_label_is_dropped_does_not_stay():
    # V = 3 characters, no transitions; frame 1 keeps label 1 alone: member (0) cannot stay, its child (0, 1) lives
    s = CR.CutSearch(1, V=3, W=4)
    x = [[5.0, 0.0, 0.0], [0.0, 5.0, 0.0]]
    r = s.run(x, None, 2)
    assert [h["ids"] for h in r] == [(0, 1)] and r[0]["ac"] == 10.0


# ---- 2. margins -----------------------------------------------------------------------------------------------------------------------
def test_left_out_is_what_the_margins_say_and_within_the_cap():
    out, total = CR.oracle_left_out()
    assert tuple(out) == tuple(CR.LEFT_OUT)
    assert total >= 10 and len(out) <= CR.LEFT_OUT_CAP * total
    for shape, inst in CR.ORACLE:
        ranking, _ = CR.oracle_reference(shape, inst)
        W = CR.SHAPES[shape][4]
        assert any(len(r) == W for r in ranking), (shape, inst)              # a full beam: the cut is exercised


# ---- 3. the Python surface --------------------------------------------------------------------------------------------------------------
def test_prune_texts_signature_and_configure():
    from end2end_amd import ASGDecoder
    from end2end_amd.decoders.ctc_decoder import CTCDecoderError
    from end2end_amd.engines import ASGBeamEngine
    labels = CR.chars_of(0)
    d = ASGDecoder(labels=labels, num_replabels=2)
    with pytest.raises(CTCDecoderError, match="cutoff_top_n needs beam_width > 1: best-path decoding expands nothing"):
        d.prune(3)
    with pytest.raises(CTCDecoderError, match="cutoff_top_n needs beam_width > 1"):
        d.configure(beam_width=1).prune(cutoff_top_n=3)
    d.configure(beam_width=4)
    for bad in (0, -2, 2.5, True, "3"):
        with pytest.raises(CTCDecoderError, match=r"cutoff_top_n must be an integer >= 1 \(or None\), got"):
            d.prune(bad)
    assert d.prune(3) is d and d._beam.cutoff_top_n == 3 and d._beam._cut(7) == 3
    assert d._beam._cut(3) is None and d._beam._cut(2) is None              # K >= V: the unpruned entries
    assert d.prune(None) is d and d._beam.cutoff_top_n is None and d.prune() is d
    d.prune(3)
    d.configure(beam_width=4)                                              # a new engine: the setting is dropped
    assert d._beam.cutoff_top_n is None
    assert list(inspect.signature(ASGDecoder.prune).parameters) == ["self", "cutoff_top_n"]
    assert inspect.signature(ASGDecoder.prune).parameters["cutoff_top_n"].default is None
    assert list(inspect.signature(ASGBeamEngine.prune).parameters) == ["self", "cutoff_top_n"]
    e = ASGBeamEngine(labels, 2, 4)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="cutoff_top_n=.*: at least 1"):
            e.prune(bad)
    assert e.prune(5) is e and e.cutoff_top_n == 5 and e.prune(None).cutoff_top_n is None
    # the pinned signatures
    assert list(inspect.signature(ASGDecoder.__init__).parameters) == ["self", "labels", "num_replabels", "time_major", "keep_on_device"]
    assert list(inspect.signature(ASGDecoder.configure).parameters) == ["self", "beam_width", "lm_path", "lmwt", "wip", "oov_penalty",
                                                                        "case_sensitive"]
    assert list(inspect.signature(ASGDecoder.restrict_to_vocabulary).parameters) == ["self", "lexicon"]
    assert list(inspect.signature(ASGBeamEngine.restrict).parameters) == ["self", "lexicon"]
    assert list(inspect.signature(ASGBeamEngine.open_stream).parameters) == ["self", "transitions", "batch_size", "max_frames",
                                                                             "device", "timesteps"]


# ---- 4. the library's host side ---------------------------------------------------------------------------------------------------------
NAMES = ("e2e_asg_beam_cut_workspace_bytes", "e2e_asg_beam_cut_stream_workspace_bytes", "e2e_asg_beam_nbest_cut",
         "e2e_asg_beam_stream_cut")


def test_symbols_are_exported_and_typed_from_the_header():
    import ctypes as C
    from end2end_amd import _C, _lib
    L = _lib.load()
    for name in NAMES:
        fn = getattr(L, name)
        assert name in _C.SIGNATURES and fn.argtypes is not None, name
        assert not hasattr(_C, name[4:])                                   # (signatures only: _C's functions are a recording)
    assert L.e2e_asg_beam_cut_workspace_bytes.restype is C.c_size_t and len(L.e2e_asg_beam_cut_workspace_bytes.argtypes) == 6
    assert len(L.e2e_asg_beam_cut_stream_workspace_bytes.argtypes) == 6
    assert len(L.e2e_asg_beam_nbest_cut.argtypes) == len(L.e2e_asg_beam_nbest_opt.argtypes) + 1
    assert len(L.e2e_asg_beam_stream_cut.argtypes) == len(L.e2e_asg_beam_stream.argtypes) + 1
    assert L.e2e_asg_beam_nbest_cut.argtypes[-1] is C.c_int and L.e2e_asg_beam_stream_cut.argtypes[-1] is C.c_int


def test_workspace_queries():
    from end2end_amd import _lib
    L = _lib.load()
    q, qs = L.e2e_asg_beam_cut_workspace_bytes, L.e2e_asg_beam_cut_stream_workspace_bytes
    B, T = 64, 1000
    for with_lm in (0, 1):
        assert q(B, T, 129, 16, with_lm, 10) == 0 and qs(B, T, 129, 16, with_lm, 10) == 0      # V = 129
        assert q(B, T, 29, 16, with_lm, 0) == 0 and qs(B, T, 29, 16, with_lm, 0) == 0          # cutoff_top_n = 0
        assert q(B, T, 29, 129, with_lm, 10) == 0 and q(B, 0, 29, 16, with_lm, 10) == 0
        for top_n in (29, 30, 1000):                                                           # no pruning: the unpruned query
            assert q(B, T, 29, 100, with_lm, top_n) == L.e2e_asg_beam_workspace_bytes(B, T, 29, 100, with_lm) > 0
            assert qs(B, 100, 29, 100, with_lm, top_n) == L.e2e_asg_beam_stream_workspace_bytes(B, 29, 100, with_lm) > 0
        # the lists, (B,T,K) and (B,T) int32, and the pair buffers with K in V's place
        W, V, K = 100, 29, 10
        al = lambda n: (n + 255) // 256 * 256                                                  # noqa: E731
        pairs = lambda k: 2 * al(W * k * 8) + al(W * k * 4)                                    # noqa: E731
        plain = L.e2e_asg_beam_workspace_bytes(B, T, V, W, with_lm)
        assert q(B, T, V, W, with_lm, K) == plain + al(B * T * K * 4) + al(B * T * 4) - B * (pairs(V) - pairs(K))
        plain_s = L.e2e_asg_beam_stream_workspace_bytes(B, V, W, with_lm)
        assert qs(B, 100, V, W, with_lm, K) == plain_s + al(B * 100 * K * 4) + al(B * 100 * 4) - B * (pairs(V) - pairs(K))


def test_argument_errors_are_found_before_any_launch():
    """No GPU here: a call that got as far as a launch would fail on that, with another code."""
    from end2end_amd import _lib
    L = _lib.load()
    ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3

    def nbest(V, W, top_n, ws_bytes=1 << 30):
        return L.e2e_asg_beam_nbest_cut(256, _lib.F32, 24 * V, V, 1, None, 256, 1, 24, V, 0, W, -1, None, 0.0, 0.0, 0.0,
                                        1, 256, 24, 256, 256, 256, 256, 256, ws_bytes, None, None, top_n)

    def stream(V, W, top_n, ws_bytes=1 << 30):
        rb = L.e2e_asg_beam_stream_row_bytes(100, min(V, 128), min(W, 128), 0)
        return L.e2e_asg_beam_stream_cut(256, _lib.F32, 24 * V, V, 1, None, 256, 1, 24, V, 0, W, -1, None, 0.0, 0.0, 0.0,
                                         256, rb, 100, 1, 256, 24, 256, 256, 256, 256, 256, 256, ws_bytes, None, None, top_n)
    for call in (nbest, stream):
        assert call(29, 8, 0) == ARG and call(29, 8, -3) == ARG
        assert call(129, 8, 10) == UNSUPPORTED and call(129, 8, 200) == UNSUPPORTED
        assert call(29, 129, 10) == UNSUPPORTED
        assert call(29, 8, 10, ws_bytes=64) == WORKSPACE
