"""No GPU: the host side of the streaming Gram-CTC beam search (e2e_gram_ctc_beam_stream): the two size queries against the
header's formulas, every argument error the host can see -- returned with made-up device addresses, before any HIP call --
and the refusals of GramCTCDecoder.open_stream."""
import math
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARPA = os.path.join(ROOT, "tests", "golden", "tiny_3gram.arpa")
E2E_ERR_ARG, E2E_ERR_UNSUPPORTED, E2E_ERR_WORKSPACE, E2E_ERR_HIP = -1, -2, -3, -4
MEMBERS, LM_MEMBERS = 16896, 11776


def up(n, a=256):
    return math.ceil(n / a) * a


def row_formula(max_frames, W, scored):
    """include/e2e_ctc.h: header, members, the LM fields, the node pool; each part rounded up to 256."""
    return 256 + MEMBERS + (LM_MEMBERS if scored else 0) + up(8 * (W * (max_frames + 1) + 1))


def test_row_bytes():
    from end2end_amd import _lib
    f = _lib.load().e2e_gram_beam_stream_row_bytes
    for max_frames, V, K, W, scored, with_lm in [(1, 1, 1, 1, 0, 0), (1000, 379, 3, 100, 1, 1), (30000, 379, 3, 100, 0, 0),
                                                 (30000, 29, 8, 128, 1, 0), (1 << 22, 5, 2, 7, 0, 0)]:
        n = f(max_frames, V, K, W, scored, with_lm)
        assert n == row_formula(max_frames, W, scored) and n % 256 == 0, (max_frames, V, K, W, scored, with_lm, n)
    assert f(30000, 379, 3, 100, 1, 1) == 24029952 == f(30000, 29, 8, 100, 1, 0)     # the header's worked example: whatever the
    assert f(30000, 379, 3, 100, 0, 0) == 24029952 - LM_MEMBERS                      # alphabet, with or without a model
    # monotone in max_frames
    sizes = [f(m, 379, 3, 100, 1, 1) for m in (1, 2, 10, 11, 1000, 30000, 1 << 22)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[2] < sizes[4] < sizes[6]
    assert f(10, 379, 3, 100, 1, 0) - f(10, 379, 3, 100, 0, 0) == LM_MEMBERS
    # 0 for what the search does not take: widths, alphabets, orders, max_frames, a model without scored
    assert f(10, 379, 3, 129, 1, 0) == 0 and f(10, 379, 3, 0, 1, 0) == 0 and f(10, 8000, 3, 17, 0, 0) == 0
    assert f(10, 8000, 3, 16, 0, 0) > 0 and f(10, 0, 3, 4, 0, 0) == 0 and f(10, 379, 9, 4, 0, 0) == 0 and f(10, 379, 0, 4, 0, 0) == 0
    assert f(0, 379, 3, 4, 0, 0) == 0 and f((1 << 22) + 1, 379, 3, 4, 0, 0) == 0 and f(-1, 379, 3, 4, 1, 1) == 0
    assert f(10, 379, 3, 4, 0, 1) == 0


def test_workspace_bytes_do_not_depend_on_the_frames():
    """The whole call's workspace per utterance without its node pool, which is the row's."""
    from end2end_amd import _lib
    L = _lib.load()
    f = L.e2e_gram_beam_stream_workspace_bytes
    assert len(f.argtypes) == 6                                           # (B, V, max_order, beam_width, scored, with_lm): no frames
    for B, V, K, W in [(64, 379, 3, 100), (1, 21, 8, 7), (3, 8000, 2, 16)]:
        pool_of_one_frame = up(8 * (W * 2 + 1))
        for scored, with_lm in [(0, 0), (1, 0), (1, 1)]:
            whole = L.e2e_gram_beam_workspace_bytes_lm(B, 1, V, K, W, with_lm)
            assert f(B, V, K, W, scored, with_lm) == whole - B * pool_of_one_frame > 0
        assert f(B, V, K, W, 1, 1) - f(B, V, K, W, 1, 0) == B * up(2 * W * V * 16)          # the answer cache
        assert f(B, V, K, W, 1, 0) == f(B, V, K, W, 0, 0)
    assert f(64, 379, 3, 100, 1, 1) < L.e2e_gram_beam_workspace_bytes_lm(64, 1000, 379, 3, 100, 1)
    assert f(1, 379, 3, 129, 0, 0) == 0 and f(1, 8000, 3, 17, 0, 0) == 0 and f(-1, 379, 3, 4, 0, 0) == 0 and f(1, 379, 9, 4, 0, 0) == 0
    assert f(1, 379, 3, 4, 0, 1) == 0 and f(0, 379, 3, 4, 0, 0) == 256


def test_argument_errors_come_before_any_launch():
    """Made-up device addresses throughout: a launch would fault, an argument error returns first."""
    import ctypes
    from end2end_amd import _lib
    from end2end_amd.engines import LanguageModel
    L = _lib.load()
    P = 256                                                              # an aligned address that is never read

    def call(V=8, K=3, R=4, W=4, scored=1, space=3, nbest=1, dtype=_lib.F32, B=1, T=10, max_frames=100, row_bytes=None, lm=None,
             opts=None, ws_bytes=1 << 30, max_out=10, null=(), state=P, counts="P"):
        p = dict(lp=P, chunk_len=P, gram_ids=P, gram_len=P, out=P, out_len=P, n_hyp=P, scores=P, frames_done=P, ws=P)
        p["counts"] = (P if scored else None) if counts == "P" else counts
        p.update({k: None for k in null})
        if row_bytes is None:
            row_bytes = L.e2e_gram_beam_stream_row_bytes(max_frames, V, K, W, 1 if scored else 0, 1 if lm is not None else 0) or 1 << 20
        rc = L.e2e_gram_ctc_beam_stream(p["lp"], dtype, T * V, V, 1, p["chunk_len"], B, T, V, p["gram_ids"], p["gram_len"], K, R, W,
                                        scored, space, lm._first.handle if lm is not None else None, 1.0, 0.0, 0.0,
                                        state, row_bytes, max_frames, nbest, p["out"], max_out, p["out_len"], p["n_hyp"],
                                        p["scores"], p["counts"], p["frames_done"], p["ws"], ws_bytes, None,
                                        ctypes.byref(opts) if opts is not None else None)
        return rc, L.e2e_last_error().decode()

    other_alphabet = LanguageModel(ARPA, ["_", "a", "b"], True)          # 3 labels against num_base_labels = 4
    fits = LanguageModel(ARPA, ["_", "a", "b", " "], True)               # no lexicon, and (without a GPU) no device tables
    transcribed = LanguageModel(ARPA, ["_", "a", "b", " "], True, transcriptions=[("a", "a"), ("ab", "a b")], blank_idx=0)
    words = LanguageModel(None, ["_", "a", "b", " "], True, words=["ab"], lexicon=True)
    restrict, plain_opts = _lib.GramBeamOpts(1, None), _lib.GramBeamOpts(0, None)
    need = L.e2e_gram_beam_stream_row_bytes(100, 8, 3, 4, 1, 0)
    cases = [
        # the whole calls' errors, with their codes
        (dict(dtype=_lib.F16), E2E_ERR_ARG, "dtype"), (dict(dtype=99), E2E_ERR_ARG, "dtype"),
        (dict(B=-1), E2E_ERR_ARG, "bad sizes"), (dict(T=0), E2E_ERR_ARG, "bad sizes"), (dict(V=0), E2E_ERR_ARG, "bad sizes"),
        (dict(max_out=-1), E2E_ERR_ARG, "bad sizes"),
        (dict(K=0), E2E_ERR_ARG, "max_order"), (dict(K=9), E2E_ERR_ARG, "max_order"),
        (dict(W=0), E2E_ERR_ARG, "at least 1"), (dict(W=129), E2E_ERR_UNSUPPORTED, "exceeds e2e_gram_beam_max_width"),
        (dict(V=8000, R=4, W=17), E2E_ERR_UNSUPPORTED, "exceeds e2e_gram_beam_max_width"),
        (dict(R=0), E2E_ERR_ARG, "num_base_labels"), (dict(R=9), E2E_ERR_ARG, "num_base_labels"),
        (dict(space=4), E2E_ERR_ARG, "space_id"),
        (dict(lm=other_alphabet), E2E_ERR_ARG, "loaded with 3 labels"),
        (dict(lm=transcribed), E2E_ERR_ARG, "custom transcriptions"),
        (dict(lm=words), E2E_ERR_ARG, "word list"),
        (dict(opts=restrict), E2E_ERR_ARG, "restrict_to_lexicon needs a model"),
        (dict(lm=fits, opts=restrict), E2E_ERR_ARG, "has no lexicon"),
        # the stream's own
        (dict(nbest=-1), E2E_ERR_ARG, "nbest=-1 outside [0, beam_width=4]"), (dict(nbest=5), E2E_ERR_ARG, "nbest=5 outside"),
        (dict(max_frames=0), E2E_ERR_ARG, "max_frames"), (dict(max_frames=(1 << 22) + 1), E2E_ERR_ARG, "max_frames"),
        (dict(row_bytes=need - 8), E2E_ERR_ARG, "row_bytes"), (dict(row_bytes=need + 4), E2E_ERR_ARG, "multiple of 8"),
        (dict(scored=0, row_bytes=need - MEMBERS), E2E_ERR_ARG, "row_bytes"),
        (dict(scored=0, lm=fits), E2E_ERR_ARG, "scored = 0"), (dict(scored=0, counts=P), E2E_ERR_ARG, "scored = 0"),
        (dict(scored=0, opts=plain_opts), E2E_ERR_ARG, "scored = 0"),
        (dict(null=("lp",)), E2E_ERR_ARG, "null pointer"), (dict(null=("chunk_len",)), E2E_ERR_ARG, "null pointer"),
        (dict(null=("gram_ids",)), E2E_ERR_ARG, "null pointer"), (dict(null=("gram_len",)), E2E_ERR_ARG, "null pointer"),
        (dict(state=None), E2E_ERR_ARG, "null pointer"), (dict(null=("frames_done",)), E2E_ERR_ARG, "null pointer"),
        (dict(null=("n_hyp",)), E2E_ERR_ARG, "null pointer"), (dict(null=("scores",)), E2E_ERR_ARG, "null pointer"),
        (dict(null=("out",)), E2E_ERR_ARG, "null pointer"), (dict(null=("out_len",)), E2E_ERR_ARG, "null pointer"),
        (dict(counts=None), E2E_ERR_ARG, "null pointer"),
        (dict(state=P + 4), E2E_ERR_ARG, "8-byte aligned"),
        (dict(ws_bytes=1024), E2E_ERR_WORKSPACE, "workspace too small"), (dict(null=("ws",)), E2E_ERR_WORKSPACE, "workspace too small"),
        (dict(scored=0, ws_bytes=1024), E2E_ERR_WORKSPACE, "workspace too small"),
    ]
    for kw, code, text in cases:
        rc, err = call(**kw)
        assert rc == code and text in err, (kw, rc, err)
    if fits._first.device() < 0:                                         # (no GPU: the model has no device tables to search with)
        rc, err = call(lm=fits)
        assert rc == E2E_ERR_HIP and "no device tables" in err
    # feed only: the read-out's pointers may be NULL (the next error is the workspace's); an empty batch is no error and no launch
    rc, err = call(nbest=0, null=("out", "out_len", "n_hyp", "scores"), counts=None, ws_bytes=1024, max_out=-1)
    assert rc == E2E_ERR_WORKSPACE, err
    assert call(B=0, null=("lp", "chunk_len", "gram_ids", "gram_len", "frames_done", "ws"), state=None)[0] == 0
    assert call(B=0, scored=0, null=("lp", "chunk_len", "gram_ids", "gram_len", "frames_done", "ws"), state=None)[0] == 0


def decoder(width, labels=None):
    from end2end_amd import GramCTCDecoder
    return GramCTCDecoder(0, 4, 5, {4: [1, 2]}, beam_width=width, labels=labels, after_logsoftmax=True)


def test_open_stream_is_refused_without_a_beam():
    from end2end_amd.decoders.ctc_decoder import CTCDecoderError
    with pytest.raises(CTCDecoderError, match="beam_width > 1"):
        decoder(1).open_stream(2, 100)
    with pytest.raises(CTCDecoderError, match="at least 1"):
        decoder(4).open_stream(0, 100)
    with pytest.raises(CTCDecoderError, match="at least 1"):
        decoder(4).open_stream(2, 0)
    with pytest.raises(CTCDecoderError, match="configure"):              # an unconfigured decoder's results have no timesteps
        decoder(4).open_stream(2, 100, timesteps=True)
    st = decoder(4).open_stream(2, 100)
    assert st.frames == [0, 0] and st.state is None and st.row_bytes == 0 and not st._stream.scored
    with pytest.raises(ValueError, match="2"):
        st._stream.check_chunk((3, 5, 5))
    with pytest.raises(ValueError, match="max_frames"):
        st._stream.check_chunk((2, 101, 5))
    with pytest.raises(ValueError, match="configure"):
        st.feed_nbest(None, timesteps=True)
    scored = decoder(4, ["_", "a", "b", " "]).configure(wip=0.0).open_stream(2, 100, timesteps=True)
    assert scored._stream.scored and scored._stream.timesteps and scored._stream.lm is None


def test_symbols_and_surface():
    import inspect
    import re
    from end2end_amd import _C, _lib
    from end2end_amd.decoders import gram_ctc_decoder
    from end2end_amd.engines import ASGBeamStream, CTCBeamStream, GramBeamStream, GramCTCDecoderEngine
    L = _lib.load()
    for name in ("e2e_gram_beam_stream_row_bytes", "e2e_gram_beam_stream_workspace_bytes", "e2e_gram_ctc_beam_stream"):
        assert hasattr(L, name) and hasattr(_C, name[4:])
    assert L.e2e_ctc_abi_version() == 4
    assert list(inspect.signature(GramCTCDecoderEngine.open_stream).parameters) == ["self", "batch_size", "max_frames", "device",
                                                                                  "timesteps"]
    for name in ("feed_nbest", "feed", "reset", "frames", "check_chunk"):    # a user of one stream can use the other
        assert hasattr(GramBeamStream, name) and hasattr(CTCBeamStream, name) and hasattr(ASGBeamStream, name)
    assert GramBeamStream.HEADER_BYTES == CTCBeamStream.HEADER_BYTES == 256
    # the header declares the call with the arguments of the whole call around the stream's own
    with open(os.path.join(ROOT, "include", "e2e_ctc.h")) as f:
        code = f.read()
    m = re.search(r"int\s+e2e_gram_ctc_beam_stream\s*\(([^)]*)\)", code)
    args = [a.strip().split()[-1].lstrip("*") for a in m.group(1).split(",")]
    assert args == ["lp", "dtype", "sB", "sT", "sV", "chunk_len", "B", "T", "V", "gram_ids", "gram_len", "max_order",
                    "num_base_labels", "beam_width", "scored", "space_id", "lm", "lmwt", "wip", "oov_penalty", "state", "row_bytes",
                    "max_frames", "nbest", "out", "max_out", "out_len", "n_hyp", "scores", "counts", "frames_done", "workspace",
                    "workspace_bytes", "stream", "opts"]
    assert len(L.e2e_gram_ctc_beam_stream.argtypes) == len(args)
    # neither list of what is not provided names streaming any more
    for text in (gram_ctc_decoder.__doc__, code[code.index("int e2e_gram_ctc_greedy") - 1500:code.index("int e2e_gram_ctc_greedy")]):
        at = text.index("Not provided for Gram-CTC")
        assert "streaming" not in text[at:at + 300]
    with open(os.path.join(ROOT, "README.md")) as f:
        readme = f.read()
    for m in re.finditer(r"[Nn]ot provided for Gram-CTC", readme):
        assert "streaming" not in readme[m.start():m.start() + 300]
