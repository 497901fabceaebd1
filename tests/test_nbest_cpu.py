"""CPU: the n-best read-out of the beam search is declared, exported, bound, and checks its arguments before any launch;
its workspace and the width limits; the Python surface.  (The results themselves: tests/test_gpu_nbest.py.)"""
import os
import re

import pytest

import nbest_util as NB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_nbest_entry_points_as_an_additive_part_of_abi_4():
    hdr = open(os.path.join(ROOT, "include", "e2e_ctc.h")).read()
    assert re.search(r"size_t\s+e2e_ctc_beam_nbest_workspace_bytes\s*\(", hdr)
    assert re.search(r"int\s+e2e_ctc_beam_nbest\s*\(", hdr)
    assert "additive, ABI 4" in hdr
    assert re.search(r"#define\s+E2E_CTC_ABI_VERSION\s+4\b", hdr)
    from end2end_amd import _lib
    L = _lib.load()
    assert hasattr(L, "e2e_ctc_beam_nbest") and hasattr(L, "e2e_ctc_beam_nbest_workspace_bytes")
    assert L.e2e_ctc_abi_version() == 4


def _call(_C, W=10, nbest=10, V=7, out=256, out_len=256, n_hyp=256, scores=256, counts=256, ws_bytes=1 << 30):
    # addresses are never dereferenced on the host: every error below is found before a launch (there is no GPU here)
    B, T = 2, 20
    _C.ctc_beam_nbest(256, _C.F32, T * V, V, 1, 256, B, T, V, 0, W, -1, 0, 1.0, 0.0, -10.0, nbest,
                      out, T + 1, out_len, n_hyp, scores, counts, 0, 256, ws_bytes, 0)


def test_argument_errors_are_found_on_the_host():
    from end2end_amd import _C
    assert hasattr(_C, "ctc_beam_nbest") and hasattr(_C, "ctc_beam_nbest_workspace_bytes")
    arg = r"\(code %d\)" % -1                                   # E2E_ERR_ARG
    for nbest in (0, 11, -3):
        with pytest.raises(_C.E2EError, match="nbest.*" + arg):
            _call(_C, W=10, nbest=nbest)
    for null in ("out", "out_len", "n_hyp", "scores", "counts"):
        with pytest.raises(_C.E2EError, match="null pointer.*" + arg):
            _call(_C, **{null: 0})
    for V, lm in ((7, False), (29, False), (8000, False)):
        cap = _C.ctc_beam_max_width(V, lm)
        with pytest.raises(_C.E2EError, match="at most %d.*%s" % (cap, arg)):
            _call(_C, W=cap + 1, nbest=1, V=V)
    with pytest.raises(_C.E2EError, match=r"workspace too small.*\(code -3\)"):      # ... and the width itself is fine
        _call(_C, ws_bytes=16)


@pytest.mark.parametrize("B,T,V,W", [(1, 1, 3, 10), (5, 40, 7, 100), (64, 1500, 29, 100), (3, 40, 100, 100), (3, 25, 300, 256),
                                     (2, 12, 8000, 20)])
@pytest.mark.parametrize("lm", [False, True])
def test_workspace(B, T, V, W, lm):
    from end2end_amd import _C
    plain = _C.ctc_beam_workspace_bytes_lm(B, T, V, W, lm)
    off = _C.ctc_beam_nbest_workspace_bytes(B, T, V, W, lm, False)
    on = _C.ctc_beam_nbest_workspace_bytes(B, T, V, W, lm, True)
    assert off == plain
    assert plain < on <= plain + B * (W * (T + 3) + 8) * 4 + 256       # one int32 per prefix-tree node, plus alignment
    assert _C.ctc_beam_nbest_workspace_bytes(B, 0, V, W, lm, True) == 0      # bad sizes: 0, as the plain query


def test_width_limits_are_unchanged():
    from end2end_amd import _C
    # (the widths the one-workgroup kernel takes are pinned by test_beam_width_limits_are_queryable_and_enforced_at_construction)
    for V in (29, 80, 8000):
        for lm in (False, True):
            assert _C.ctc_beam_max_width(V, lm) == 512
    # the plain call's workspace at the flagship decode shape is what it was: nothing of the n-best call is carried by it
    assert _C.ctc_beam_workspace_bytes_lm(64, 1500, 29, 100, False) == 64 * (100 * 1503 + 8) * 8 + 256 + (-(64 * (100 * 1503 + 8) * 8) % 256)


def test_python_surface():
    import end2end_amd
    import cpp_ctc_decoder
    import pytorch_end2end
    from end2end_amd import CTCDecoder, CTCDecoderError, NBestResults
    assert NBestResults._fields == ("decoded_targets", "decoded_targets_lengths", "decoded_sentences", "scores", "ctc_scores",
                                    "lm_scores", "num_words", "num_oov_words", "num_hypotheses", "timesteps")
    assert end2end_amd.DecoderResults._fields == ("decoded_targets", "decoded_targets_lengths", "decoded_sentences")
    assert hasattr(pytorch_end2end.CTCDecoder, "decode_nbest") and hasattr(cpp_ctc_decoder.CTCDecoder, "decode_nbest")
    import torch
    with pytest.raises(CTCDecoderError, match="beam"):
        CTCDecoder(beam_width=1, labels=["_", "a", "b"]).decode_nbest(torch.zeros(1, 4, 3))
    with pytest.raises(ValueError, match="nbest"):                 # checked before any device is asked for
        cpp_ctc_decoder.CTCDecoder(0, 8, ["_", "a", "b"]).decode_nbest(torch.zeros(1, 4, 3), torch.tensor([4]), nbest=9)


def test_exhaustive_cases_order_is_checkable():
    """The exact-order test of the GPU suite compares neighbours whose oracle likelihoods differ by more than 1e-6: at least
    90 % of the neighbouring pairs of every case must (oracle alone, no GPU); flat-emission goldens are replaced."""
    cases = NB.exhaustive_cases()
    assert [c["name"] for c in cases] == NB.EXHAUSTIVE_NAMES and len(cases) >= 6
    widths = sorted({c["beam_width"] for c in cases})
    assert widths[0] == 63 and widths[-1] == 255
    for c in cases:
        assert c["gap_fraction"] >= 0.9, (c["name"], c["gap_fraction"])
    assert sum(c["replaced"] for c in cases) <= len(cases) // 2
    assert NB.num_words((1, 2, 3, 3, 1, 3), 3) == 2 and NB.num_words((3, 1), 3) == 1 and NB.num_words((), 3) == 0
