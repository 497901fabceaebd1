"""The restricted ASG beam search without a GPU: the restatement (tests/asg_lexicon_ref.py) against enumeration over the
admissible labellings, the creation frames' properties, the margins and the coverage of the cases tests/test_gpu_asg_lexicon.py
compares, and what of ASGDecoder.restrict_to_vocabulary runs without a GPU.

Measured with the restatement on one CPU core: the four grids' full-length utterances have 11 to 40 admissible labellings out of 45 to 93 spellable
ones and agree with enumeration to 1e-15; the 48 fuzz cases take 7 s together, none is left out for its margin."""
import inspect

import pytest

import asg_lexicon_ref as LR
import asg_lexicon_util as LU


def check_frames(h, n):
    """The properties of the timesteps of one hypothesis of an utterance of n frames."""
    fr = h["frames"]
    assert len(fr) == len(h["ids"]) and fr[0] == 0
    assert all(a < b for a, b in zip(fr, fr[1:]))
    assert all(k <= f < n for k, f in enumerate(fr))


@pytest.mark.parametrize("i", range(len(LU.GRIDS)))
def test_unbounded_restatement_equals_filtered_enumeration(i):
    g = LU.GRIDS[i]
    x, A, lens, enum, total = LU.grid_case(i)
    got = LU.grid_unbounded(i)
    for b in range(3):
        assert 0 < len(enum[b]) <= total[b]
        assert {h["ids"] for h in got[b]} == set(enum[b])
        for h in got[b]:
            assert abs(h["ac"] - enum[b][h["ids"]]) <= 1e-12 * max(1.0, abs(h["ac"])), (b, h)
            assert LR.admissible(h["ids"], g["V"], g["R"], LU.space_of(g["chars"]), g["chars"], LR.Lexicon(g["words"]))
            check_frames(h, lens[b])
            assert h["lm"] == 0.0                                       # the model that scores nothing
    assert 7 <= len(enum[0]) <= 48 and 45 <= total[0] <= 93 and len(enum[2]) < total[2]   # the restriction bites


def test_admissible_is_the_definition():
    chars, lex = ["a", " ", "b", "d"], LR.Lexicon(["add", "bad", "a"])
    V, R, sp = 6, 2, 1                                                   # ids: a 0, space 1, b 2, d 3, <1> 4, <2> 5

    def adm(*s):
        return LR.admissible(s, V, R, sp, chars, lex)
    assert adm(0) and adm(0, 3) and adm(0, 3, 4) and adm(0, 3, 4, 1) and adm(0, 3, 4, 1, 2)
    assert not adm(0, 3, 1)                                              # "ad" is no word: no space after it
    assert not adm(0, 3, 5)                                              # "addd"
    assert not adm(0, 4)                                                 # "aa"
    assert not adm(3) and not adm(4) and not adm()                       # "d" begins nothing; a leading repeat label; empty
    assert adm(1) and adm(1, 0) and adm(0, 1, 0, 1) and not adm(1, 4)    # the space may come first; never a repeat after it
    assert adm(0, 3, 0) is False and adm(2, 0, 3, 1, 0)                  # "ada"; "bad a"
    assert not adm(0, 0) and not adm(0, 3, 3)                            # equal neighbours are one label
    folded = LR.Lexicon(["Add"], case_sensitive=False)
    assert LR.admissible((0, 3, 4), V, R, sp, ["A", " ", "b", "D"], folded)
    assert not LR.admissible((0, 3, 4), V, R, sp, ["A", " ", "b", "D"], LR.Lexicon(["add"], case_sensitive=True))


@pytest.mark.parametrize("name", sorted(LU.P_MODELS))
def test_pruned_cases_are_decided_by_wide_margins(name):
    for W in LU.P_WIDTHS:
        want, gap = LU.pruned_ref(name, W)
        assert gap >= LU.MIN_GAP, (name, W, gap)
        assert want[2] == [] and all(len(want[b]) > 0 for b in (0, 1, 3))
        for b in (0, 1, 3):
            for h in want[b]:
                check_frames(h, LU.P_LENS[b])
    want, gap = LU.wide_ref()
    assert gap >= LU.MIN_GAP and all(len(r) > 0 for r in want)


def test_fuzz_margins_and_coverage():
    left_out = tuple(s for s in range(LU.FUZZ_N) if not LU.compared(s))
    assert left_out == LU.LEFT_OUT and len(left_out) <= LU.LEFT_OUT_CAP * LU.FUZZ_N
    facts = [LU.facts(s) for s in range(LU.FUZZ_N) if s not in left_out]
    assert any(f.died for f in facts)
    assert any(f.never_fills for f in facts)
    assert any(f.full and f.case.W == 128 for f in facts)
    assert any(f.unfinished for f in facts)
    assert {f.case.V for f in facts} >= set(LU.FUZZ_V) and {f.case.W for f in facts} == set(LU.FUZZ_W)
    assert {f.case.R for f in facts} == {0, 1, 2} and {f.case.space >= 0 for f in facts} == {True, False}
    assert {f.case.model for f in facts} >= {None, "tiny_3gram.arpa", "lm_order4.arpa", "lm_order3_nounk.arpa"}
    assert any(f.case.no_A for f in facts) and max(len(f.case.x[0]) for f in facts) <= 48
    for f in facts:
        c = f.case
        for b, r in enumerate(f.ranking):
            for h in r:
                check_frames(h, c.lens[b])


# ---- the Python layer ----------------------------------------------------------------------------------------------------
def test_signatures():
    from end2end_amd import ASGDecoder
    assert list(inspect.signature(ASGDecoder.__init__).parameters) == ["self", "labels", "num_replabels", "time_major", "keep_on_device"]
    assert list(inspect.signature(ASGDecoder.configure).parameters) == ["self", "beam_width", "lm_path", "lmwt", "wip", "oov_penalty",
                                                                       "case_sensitive"]
    assert list(inspect.signature(ASGDecoder.restrict_to_vocabulary).parameters) == ["self", "lexicon"]
    assert inspect.signature(ASGDecoder.restrict_to_vocabulary).parameters["lexicon"].default is None
    p = inspect.signature(ASGDecoder.decode_nbest).parameters
    assert list(p) == ["self", "emissions", "transitions", "logits_lengths", "nbest", "timesteps"] and p["timesteps"].default is False
    from end2end_amd.engines import ASGBeamEngine
    assert inspect.signature(ASGBeamEngine.decode_nbest).parameters["timesteps"].default is False
    assert list(inspect.signature(ASGBeamEngine.restrict).parameters) == ["self", "lexicon"]


def test_restrict_to_vocabulary_checks(tmp_path):
    from end2end_amd import ASGDecoder
    from end2end_amd.decoders.ctc_decoder import CTCDecoderError
    labels = ["a", "b", " "]
    with pytest.raises(CTCDecoderError, match="beam_width > 1"):
        ASGDecoder(labels, 1).restrict_to_vocabulary(lexicon=["ab"])
    with pytest.raises(CTCDecoderError, match="beam_width > 1"):
        ASGDecoder(labels, 1).configure(beam_width=1).restrict_to_vocabulary(lexicon=["ab"])
    with pytest.raises(CTCDecoderError, match="labels"):
        ASGDecoder(None, 1).configure(beam_width=4).restrict_to_vocabulary(lexicon=["ab"])
    with pytest.raises(CTCDecoderError, match="needs a vocabulary"):
        ASGDecoder(labels, 1).configure(beam_width=4).restrict_to_vocabulary()
    with pytest.raises(CTCDecoderError, match="empty"):
        ASGDecoder(labels, 1).configure(beam_width=4).restrict_to_vocabulary(lexicon=[])
    with pytest.raises(CTCDecoderError, match="Can't find a lexicon"):
        ASGDecoder(labels, 1).configure(beam_width=4).restrict_to_vocabulary(lexicon=str(tmp_path / "none.txt"))


def test_c_symbol_and_opts_struct():
    import ctypes
    from end2end_amd import _lib
    L = _lib.load()
    assert hasattr(L, "e2e_asg_beam_nbest_opt")
    assert [f[0] for f in _lib.AsgBeamOpts._fields_] == ["restrict_to_lexicon", "timesteps"]
    assert ctypes.sizeof(_lib.AsgBeamOpts) == 16
    # restrict_to_lexicon without a model: E2E_ERR_ARG on the host, before anything is read or launched
    opts = _lib.AsgBeamOpts(1, None)
    args = [256, _lib.F32, 29 * 10, 29, 1, None, 256, 1, 10, 29, 2, 4, 0, None, 1.0, 0.0, 0.0, 4, 256, 10, 256, 256, 256, 256, 256, 1 << 30,
            None]
    rc = L.e2e_asg_beam_nbest_opt(*args, ctypes.byref(opts))
    assert rc == -1 and b"restrict_to_lexicon needs a model" in L.e2e_last_error()
