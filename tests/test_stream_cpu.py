"""CPU: the streaming beam search (e2e_ctc_beam_stream) is declared, exported, bound, and checks its arguments before any
launch; the size of a state row; the plain calls' workspaces are what they were; the Python surface.  (The results themselves:
tests/test_gpu_stream.py.)"""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("e2e_ctc_beam_stream_row_bytes", "e2e_ctc_beam_stream_workspace_bytes", "e2e_ctc_beam_stream")


def test_header_declares_the_stream_entry_points_as_an_additive_part_of_abi_4():
    hdr = open(os.path.join(ROOT, "include", "e2e_ctc.h")).read()
    assert re.search(r"size_t\s+e2e_ctc_beam_stream_row_bytes\s*\(", hdr)
    assert re.search(r"size_t\s+e2e_ctc_beam_stream_workspace_bytes\s*\(", hdr)
    assert re.search(r"int\s+e2e_ctc_beam_stream\s*\(", hdr)
    section = hdr[hdr.index("Streaming beam search"):hdr.index("size_t e2e_ctc_beam_stream_row_bytes")]
    assert "additive, ABI 4" in section and "bit for bit" in section and "first 256 bytes are zero" in section
    assert re.search(r"#define\s+E2E_CTC_ABI_VERSION\s+4\b", hdr)


def test_library_exports_and_both_layers_bind_them():
    from end2end_amd import _C, _lib
    L = _lib.load()
    for n in NAMES:
        assert hasattr(L, n), n
        assert getattr(L, n).argtypes is not None, n                 # bound with a signature, not by default
        assert hasattr(_C, n[len("e2e_"):]), n
    assert L.e2e_ctc_abi_version() == 4 and _C.abi_version() == 4
    assert len(L.e2e_ctc_beam_stream.argtypes) == 33


def _call(_C, W=10, nbest=10, V=7, B=2, T=20, max_frames=100, ts=True, row_bytes=None, state=256, chunk_len=256, lp=256,
          out=256, out_len=256, n_hyp=256, scores=256, counts=256, timesteps=256, frames_done=256, ws=0, ws_bytes=0,
          restrict=False):
    # addresses are never dereferenced on the host: every error below is found before a launch (there is no GPU here)
    if row_bytes is None:
        row_bytes = _C.ctc_beam_stream_row_bytes(max_frames, V, W, False, ts)
    _C.ctc_beam_stream(lp, _C.F32, T * V, V, 1, chunk_len, B, T, V, 0, W, -1, 0, 1.0, 0.0, -10.0, state, row_bytes, max_frames,
                       ts, nbest, out, max_frames + 1, out_len, n_hyp, scores, counts, timesteps if ts else 0, frames_done,
                       ws, ws_bytes, 0, restrict)


def test_argument_errors_are_found_on_the_host():
    from end2end_amd import _C
    arg = r"\(code %d\)" % -1                                   # E2E_ERR_ARG
    for nbest in (-1, 11):
        with pytest.raises(_C.E2EError, match="nbest.*" + arg):
            _call(_C, W=10, nbest=nbest)
    for null in ("state", "chunk_len", "lp", "frames_done", "out", "out_len", "n_hyp", "scores", "counts"):
        with pytest.raises(_C.E2EError, match="null pointer.*" + arg):
            _call(_C, **{null: 0})
    for kw in (dict(T=0), dict(V=0), dict(W=0, nbest=0, row_bytes=4096), dict(max_frames=0, row_bytes=4096), dict(B=-1)):
        with pytest.raises(_C.E2EError, match="bad sizes.*" + arg):
            _call(_C, **kw)
    need = _C.ctc_beam_stream_row_bytes(100, 7, 10, False, True)
    with pytest.raises(_C.E2EError, match="row_bytes.*needs %d.*%s" % (need, arg)):
        _call(_C, row_bytes=need - 256)
    with pytest.raises(_C.E2EError, match="row_bytes.*" + arg):             # the row of a stream without timestamps is smaller
        _call(_C, ts=True, row_bytes=_C.ctc_beam_stream_row_bytes(100, 7, 10, False, False))
    with pytest.raises(_C.E2EError, match="timesteps.*with_timesteps = 0.*" + arg):
        _C.ctc_beam_stream(256, _C.F32, 140, 7, 1, 256, 2, 20, 7, 0, 10, -1, 0, 1.0, 0.0, -10.0, 256,
                           _C.ctc_beam_stream_row_bytes(100, 7, 10, False, False), 100, False, 10, 256, 101, 256, 256, 256, 256,
                           256, 256, 0, 0, 0)
    for V, lm in ((7, False), (29, False), (8000, False)):
        cap = _C.ctc_beam_max_width(V, lm)
        with pytest.raises(_C.E2EError, match="at most %d.*%s" % (cap, arg)):
            _call(_C, W=cap + 1, nbest=1, V=V, row_bytes=1 << 20)
    with pytest.raises(_C.E2EError, match="restrict_to_lexicon.*" + arg):
        _call(_C, restrict=True)
    # the general kernel needs a workspace, the one-workgroup kernel none: (V, W) = (300, 256) takes the general one
    assert _C.ctc_beam_stream_workspace_bytes(2, 7, 10, False) == 0
    assert _C.ctc_beam_stream_workspace_bytes(2, 300, 256, False) > 0
    with pytest.raises(_C.E2EError, match=r"workspace too small.*\(code -3\)"):
        _call(_C, V=300, W=256, nbest=1, ws=256, ws_bytes=16)


MEMBER_BYTES = 7 * 8 + 88 + 8 * 4       # Members::bytes per hypothesis: seven f64, the LM state (LmFields, 88 bytes), eight int32


@pytest.mark.parametrize("V,W", [(3, 2), (7, 100), (29, 100), (300, 256), (8000, 20)])
@pytest.mark.parametrize("lm", [False, True])
def test_row_bytes(V, W, lm):
    from end2end_amd import _C
    last = 0
    for mf in (1, 2, 40, 41, 1500, 30000):
        for ts in (False, True):
            n = _C.ctc_beam_stream_row_bytes(mf, V, W, lm, ts)
            nodes = W * (mf + 3) + 8
            exact = 256 + MEMBER_BYTES * W + nodes * (12 if ts else 8)
            assert n % 256 == 0 and exact <= n <= exact + 3 * 255, (mf, ts, n, exact)        # header, members, nodes, frames
        plain = _C.ctc_beam_stream_row_bytes(mf, V, W, lm, False)
        assert plain >= last and _C.ctc_beam_stream_row_bytes(mf, V, W, lm, True) > plain    # monotone in max_frames
        last = plain
    assert _C.ctc_beam_stream_row_bytes(0, V, W, lm, False) == 0                              # bad sizes: 0
    assert _C.ctc_beam_stream_row_bytes(40, V, 513, lm, False) == 0                           # beyond the width limit
    assert _C.ctc_beam_stream_row_bytes(40, V, W, lm, False) == _C.ctc_beam_stream_row_bytes(40, V + 1, W, lm, False)   # no alphabet in it


def test_plain_calls_workspaces_and_width_limits_are_unchanged():
    from end2end_amd import _C
    for V in (29, 80, 8000):
        for lm in (False, True):
            assert _C.ctc_beam_max_width(V, lm) == 512
    assert _C.ctc_beam_workspace_bytes_lm(64, 1500, 29, 100, False) == 64 * (100 * 1503 + 8) * 8 + 256 + (-(64 * (100 * 1503 + 8) * 8) % 256)
    for B, T, V, W in ((1, 1, 3, 10), (5, 40, 7, 100), (3, 25, 300, 256)):
        for lm in (False, True):
            plain = _C.ctc_beam_workspace_bytes_lm(B, T, V, W, lm)
            assert _C.ctc_beam_nbest_workspace_bytes(B, T, V, W, lm, False) == plain
            # the stream's workspace is the general kernel's share of the plain one: no nodes in it
            nodes = B * (W * (T + 3) + 8) * 8
            assert _C.ctc_beam_stream_workspace_bytes(B, V, W, lm) in (0, plain - nodes - (-nodes % 256))


def test_python_surface():
    import torch
    import cpp_ctc_decoder
    import end2end_amd
    import pytorch_end2end
    from end2end_amd import CTCDecoder, CTCDecoderError
    for cls in (end2end_amd.CTCDecoder, pytorch_end2end.CTCDecoder, cpp_ctc_decoder.CTCDecoder):
        assert hasattr(cls, "open_stream")
    with pytest.raises(CTCDecoderError, match="beam"):
        CTCDecoder(beam_width=1, labels=["_", "a", "b"]).open_stream(2, 100)
    with pytest.raises(ValueError, match="beam"):
        cpp_ctc_decoder.CTCDecoder(0, 1, ["_", "a", "b"]).open_stream(2, 100)
    # shapes are checked before any device is asked for (there is none here)
    s = CTCDecoder(beam_width=8, labels=["_", "a", "b"]).open_stream(2, 10)
    for name in ("feed", "feed_nbest", "reset", "frames", "state"):
        assert hasattr(s, name)
    assert s.frames == [0, 0] and s.state is None
    with pytest.raises(ValueError, match="max_frames"):
        s.feed(torch.zeros(2, 11, 3))
    with pytest.raises(ValueError, match="utterances"):
        s.feed_nbest(torch.zeros(3, 4, 3))
    tm = CTCDecoder(beam_width=8, labels=["_", "a", "b"], time_major=True).open_stream(2, 10)
    with pytest.raises(ValueError, match="max_frames"):
        tm.feed(torch.zeros(11, 2, 3))
    with pytest.raises(ValueError, match="utterances"):
        tm.feed(torch.zeros(4, 3, 3))
    e = cpp_ctc_decoder.CTCDecoder(0, 8, ["_", "a", "b"]).open_stream(2, 10, timesteps=True)
    with pytest.raises(ValueError, match="nbest"):
        e.feed_nbest(torch.zeros(2, 4, 3), nbest=9)
    with pytest.raises(ValueError, match="row"):
        e.reset([2])
    e.reset()
    with pytest.raises(ValueError):
        cpp_ctc_decoder.CTCDecoder(0, 8, ["_", "a", "b"]).open_stream(0, 10)


def _engine_streams():
    """One stream of each family, opened for 2 utterances of up to 10 frames at beam_width 4: no GPU is asked for."""
    from end2end_amd.engines import ASGBeamEngine, CTCDecoderEngine, GramCTCDecoderEngine
    labels = ["_", "a", "b"]
    return {"ctc": (CTCDecoderEngine(0, 4, labels).open_stream(2, 10), "logits"),
            "asg": (ASGBeamEngine(labels, 0, 4).open_stream(None, 2, 10), "emissions"),
            "gram": (GramCTCDecoderEngine(0, 3, 4, {3: [1, 2]}, 4, labels).open_stream(2, 10), "logits")}


def test_the_three_streams_share_one_base_and_its_errors():
    import inspect
    import torch
    from end2end_amd.engines import ASGBeamStream, CTCBeamStream, GramBeamStream, _BeamStream
    shared = ("feed_nbest", "feed", "reset", "check_chunk", "frames")
    for cls in (CTCBeamStream, ASGBeamStream, GramBeamStream):
        assert cls.__bases__ == (_BeamStream,)
        for name in shared:
            assert name in vars(_BeamStream)
            if (cls, name) != (GramBeamStream, "feed_nbest"):
                assert name not in vars(cls), (cls.__name__, name)
    # Gram's feed_nbest is the base's with `timesteps` per read-out, and hands the work to the base
    base, gram = inspect.signature(_BeamStream.feed_nbest), inspect.signature(GramBeamStream.feed_nbest)
    assert list(gram.parameters) == list(base.parameters) + ["timesteps"]
    names = GramBeamStream.feed_nbest.__code__.co_names
    assert "_feed_nbest" in names and not {"check_chunk", "_launch", "_prepare", "_state_for"} & set(names)
    for family, (s, what) in _engine_streams().items():
        assert isinstance(s, _BeamStream) and s.HEADER_BYTES == 256 and s.frames == [0, 0] and s.state is None and s.row_bytes == 0
        for nbest in (-1, 5):
            with pytest.raises(ValueError, match=re.escape("nbest=%d outside [0, beam_width=4]" % nbest)):
                s.feed_nbest(torch.zeros(2, 4, 4), nbest=nbest)
        for call in (s.feed, s.feed_nbest, lambda x: s.check_chunk(tuple(x.shape))):
            with pytest.raises(ValueError, match=re.escape("%s must be (batch, time, alphabet)" % what)):
                call(torch.zeros(2, 4))
            with pytest.raises(ValueError, match=re.escape("the chunk has 3 utterances, the stream was opened for 2")):
                call(torch.zeros(3, 4, 4))
            for frames in (0, 11):
                with pytest.raises(ValueError, match=re.escape("a chunk of %d frames: the stream takes 1 .. max_frames = 10" % frames)):
                    call(torch.zeros(2, frames, 4))
        for rows in ([2], [-1], torch.tensor([0, 2])):
            with pytest.raises(ValueError, match=re.escape("outside the stream's 2 utterances")):
                s.reset(rows)
        with pytest.raises(ValueError, match=re.escape("row 2 outside the stream's 2 utterances")):
            s.reset([1, 2])
        s.reset()
        s.reset([1])
        assert s.frames == [0, 0], family
