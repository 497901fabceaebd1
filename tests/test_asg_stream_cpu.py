"""No GPU: the host side of the streaming ASG beam search (e2e_asg_beam_stream): the state row's size against the header's
formula, every argument error the host can see -- returned with made-up device addresses, before any HIP call -- and the
refusals of ASGDecoder.open_stream."""
import math
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARPA = os.path.join(ROOT, "tests", "golden", "tiny_3gram.arpa")
E2E_ERR_ARG, E2E_ERR_UNSUPPORTED, E2E_ERR_WORKSPACE, E2E_ERR_HIP = -1, -2, -3, -4


def up(n, a=256):
    return math.ceil(n / a) * a


def row_formula(max_frames, W, with_lm):
    """include/e2e_ctc.h: header, members, the LM fields, the node pool; each part rounded up to 256."""
    return 256 + 4096 + (10240 if with_lm else 0) + up(8 * (W * (max_frames + 1) + 1))


def test_row_bytes():
    from end2end_amd import _lib
    f = _lib.load().e2e_asg_beam_stream_row_bytes
    for max_frames, V, W, with_lm in [(1, 1, 1, 0), (1000, 29, 100, 1), (30000, 29, 100, 0), (30000, 128, 128, 1), (1 << 22, 5, 7, 0)]:
        n = f(max_frames, V, W, with_lm)
        assert n == row_formula(max_frames, W, with_lm) and n % 256 == 0, (max_frames, V, W, with_lm, n)
    assert f(30000, 29, 100, 0) == 24005376 and f(30000, 29, 100, 1) == 24015616      # the header's worked example
    assert f(10, 29, 100, 0) < f(11, 29, 100, 0) < f(1000, 29, 100, 0)
    assert f(10, 29, 100, 1) - f(10, 29, 100, 0) == 10240
    # 0 for what the search does not take
    assert f(10, 129, 4, 0) == 0 and f(10, 0, 4, 0) == 0 and f(10, 29, 129, 0) == 0 and f(10, 29, 0, 0) == 0
    assert f(0, 29, 4, 0) == 0 and f((1 << 22) + 1, 29, 4, 0) == 0


def test_workspace_bytes_do_not_depend_on_the_frames():
    from end2end_amd import _lib
    L = _lib.load()
    B, V, W = 64, 29, 100
    pairs = W * V
    want = up(V * V * 8) + B * (2 * up(pairs * 8) + up(pairs * 4)) + 256
    assert L.e2e_asg_beam_stream_workspace_bytes(B, V, W, 0) == want == L.e2e_asg_beam_stream_workspace_bytes(B, V, W, 1)
    assert want < L.e2e_asg_beam_workspace_bytes(B, 1, V, W, 0)                          # (no node pool at all)
    assert L.e2e_asg_beam_stream_workspace_bytes(B, 129, W, 0) == 0 and L.e2e_asg_beam_stream_workspace_bytes(B, V, 129, 0) == 0


def test_argument_errors_come_before_any_launch():
    """Made-up device addresses throughout: a launch would fault, an argument error returns first."""
    import ctypes
    from end2end_amd import _lib
    from end2end_amd.engines import LanguageModel
    L = _lib.load()
    P = 256                                                              # an aligned address that is never read

    def call(V=29, W=4, R=2, space=0, nbest=1, dtype=_lib.F32, B=1, T=10, max_frames=100, row_bytes=None, lm=None, opts=None,
             ws_bytes=1 << 30, max_out=10, null=(), state=P):
        p = dict(x=P, chunk_len=P, out=P, out_len=P, n_hyp=P, scores=P, counts=P, frames_done=P, ws=P)
        p.update({k: None for k in null})
        if row_bytes is None:
            row_bytes = L.e2e_asg_beam_stream_row_bytes(max_frames, V, W, 1 if lm is not None else 0) or 1 << 20
        rc = L.e2e_asg_beam_stream(p["x"], dtype, T * V, V, 1, None, p["chunk_len"], B, T, V, R, W, space,
                                   lm._first.handle if lm is not None else None, 1.0, 0.0, 0.0, state, row_bytes, max_frames,
                                   nbest, p["out"], max_out, p["out_len"], p["n_hyp"], p["scores"], p["counts"], p["frames_done"],
                                   p["ws"], ws_bytes, None, ctypes.byref(opts) if opts is not None else None)
        return rc, L.e2e_last_error().decode()

    other_alphabet = LanguageModel(ARPA, ["a", "b", " "], True)          # 3 labels against V = 29
    fits = LanguageModel(ARPA, ["a", "b", " ", "<1>"], True)             # no lexicon, and (without a GPU) no device tables
    transcribed = LanguageModel(ARPA, ["a", "b", " ", "<1>"], True, transcriptions=[("a", "a"), ("ab", "a b")])
    restrict = _lib.AsgBeamOpts(1, None)
    need = L.e2e_asg_beam_stream_row_bytes(100, 29, 4, 0)
    cases = [
        (dict(dtype=_lib.F16), E2E_ERR_ARG, "dtype"), (dict(dtype=99), E2E_ERR_ARG, "dtype"),
        (dict(B=-1), E2E_ERR_ARG, "bad sizes"), (dict(T=0), E2E_ERR_ARG, "bad sizes"), (dict(V=0), E2E_ERR_ARG, "bad sizes"),
        (dict(max_out=-1), E2E_ERR_ARG, "bad sizes"),
        (dict(V=129), E2E_ERR_UNSUPPORTED, "e2e_asg_max_labels"),
        (dict(R=29), E2E_ERR_ARG, "num_replabels"), (dict(space=27), E2E_ERR_ARG, "space_id"),
        (dict(W=0), E2E_ERR_ARG, "at least 1"), (dict(W=129), E2E_ERR_UNSUPPORTED, "exceeds e2e_asg_beam_max_width"),
        (dict(nbest=-1), E2E_ERR_ARG, "nbest=-1 outside [0, beam_width=4]"), (dict(nbest=5), E2E_ERR_ARG, "nbest=5 outside"),
        (dict(max_frames=0), E2E_ERR_ARG, "max_frames"), (dict(max_frames=(1 << 22) + 1), E2E_ERR_ARG, "max_frames"),
        (dict(row_bytes=need - 8), E2E_ERR_ARG, "row_bytes"), (dict(row_bytes=need + 4), E2E_ERR_ARG, "multiple of 8"),
        (dict(lm=other_alphabet), E2E_ERR_ARG, "loaded with 3 labels"),
        (dict(V=4, R=1, space=2, lm=transcribed), E2E_ERR_UNSUPPORTED, "custom transcriptions"),
        (dict(opts=restrict), E2E_ERR_ARG, "restrict_to_lexicon needs a model"),
        (dict(V=4, R=1, space=2, lm=fits, opts=restrict), E2E_ERR_ARG, "has no lexicon"),
        (dict(null=("x",)), E2E_ERR_ARG, "null pointer"), (dict(null=("chunk_len",)), E2E_ERR_ARG, "null pointer"),
        (dict(state=None), E2E_ERR_ARG, "null pointer"), (dict(null=("frames_done",)), E2E_ERR_ARG, "null pointer"),
        (dict(null=("n_hyp",)), E2E_ERR_ARG, "null pointer"), (dict(null=("scores",)), E2E_ERR_ARG, "null pointer"),
        (dict(null=("out",)), E2E_ERR_ARG, "null pointer"),
        (dict(state=P + 4), E2E_ERR_ARG, "8-byte aligned"),
        (dict(ws_bytes=1024), E2E_ERR_WORKSPACE, "workspace too small"), (dict(null=("ws",)), E2E_ERR_WORKSPACE, "workspace too small"),
    ]
    for kw, code, text in cases:
        rc, err = call(**kw)
        assert rc == code and text in err, (kw, rc, err)
    if fits._first.device() < 0:                                         # (no GPU: the model has no device tables to search with)
        rc, err = call(V=4, R=1, space=2, lm=fits)
        assert rc == E2E_ERR_HIP and "no device tables" in err
    # feed only: the read-out's pointers may be NULL (the next error is the workspace's); an empty batch is no error and no launch
    rc, err = call(nbest=0, null=("out", "out_len", "n_hyp", "scores", "counts"), ws_bytes=1024)
    assert rc == E2E_ERR_WORKSPACE, err
    assert call(B=0, null=("x", "chunk_len", "frames_done", "ws"), state=None)[0] == 0


def test_open_stream_is_refused_without_a_beam():
    from end2end_amd import ASGDecoder
    from end2end_amd.decoders.ctc_decoder import CTCDecoderError
    labels = ["a", "b", " "]
    with pytest.raises(CTCDecoderError, match="beam_width > 1"):
        ASGDecoder(labels, 1).open_stream(None, 2, 100)
    with pytest.raises(CTCDecoderError, match="beam_width > 1"):
        ASGDecoder(labels, 1).configure(beam_width=1).open_stream(None, 2, 100)
    with pytest.raises(CTCDecoderError, match="at least 1"):
        ASGDecoder(labels, 1).configure(beam_width=4).open_stream(None, 0, 100)
    st = ASGDecoder(labels, 1).configure(beam_width=4).open_stream(None, 2, 100, timesteps=True)
    assert st.frames == [0, 0] and st.state is None and st.row_bytes == 0
    with pytest.raises(ValueError, match="2"):
        st._stream.check_chunk((3, 5, 4))
    with pytest.raises(ValueError, match="max_frames"):
        st._stream.check_chunk((2, 101, 4))


def test_symbols_and_surface():
    import inspect
    from end2end_amd import _lib
    from end2end_amd.engines import ASGBeamEngine, ASGBeamStream, CTCBeamStream
    L = _lib.load()
    for name in ("e2e_asg_beam_stream_row_bytes", "e2e_asg_beam_stream_workspace_bytes", "e2e_asg_beam_stream"):
        assert hasattr(L, name)
    assert L.e2e_ctc_abi_version() == 4
    assert list(inspect.signature(ASGBeamEngine.open_stream).parameters) == ["self", "transitions", "batch_size", "max_frames",
                                                                           "device", "timesteps"]
    for name in ("feed_nbest", "feed", "reset", "frames", "check_chunk"):    # a user of one stream can use the other
        assert hasattr(ASGBeamStream, name) and hasattr(CTCBeamStream, name)
    assert ASGBeamStream.HEADER_BYTES == CTCBeamStream.HEADER_BYTES == 256
