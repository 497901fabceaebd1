"""The ASG beam search's checker against brute force, the margins of the fixed-seed cases the GPU tests compare, and what
of the new API runs without a GPU (tests/test_gpu_asg_beam.py has the kernel)."""
import math
import os

import pytest
import torch

import asg_beam_ref as REF
import asg_beam_util as U


@pytest.mark.parametrize("i", range(len(U.TINY_GRID)))
def test_restatement_unbounded_equals_enumeration(i):
    V, T, R, space = U.TINY_GRID[i]
    _, _, lens, enum = U.tiny_case(i)
    got = U.tiny_unbounded(i)
    for b in range(3):
        want = enum[b]
        assert len(want) <= 128                      # (the GPU test's width holds every sequence)
        assert {h["ids"] for h in got[b]} == set(want)
        for h in got[b]:
            assert abs(h["ac"] - want[h["ids"]]) <= 1e-12 * max(1.0, abs(want[h["ids"]])), (b, h)
            assert h["total"] == h["ac"]             # no model, wip = 0
        order = sorted(got[b], key=lambda h: (-h["total"], REF.key_of(h["ids"])))
        assert [h["ids"] for h in order] == [h["ids"] for h in got[b]]


def test_enumeration_drops_unspellable():
    V, T, R, space = U.TINY_GRID[5]
    _, _, lens, enum = U.tiny_case(5)
    nch = V - R
    for seq in enum[0]:
        assert seq[0] < nch
        for a, c in zip(seq, seq[1:]):
            assert a != c and not (c >= nch and (a >= nch or a == space))
    assert any(c >= nch for seq in enum[0] for c in seq)
    assert (3,) not in enum[0] and (1, 3) not in enum[0] and (0, 3, 4) not in enum[0] and (0, 3) in enum[0]


@pytest.mark.parametrize("W", U.PRUNED_WIDTHS)
def test_pruned_cases_have_a_margin(W):
    ranking, gap = U.pruned_ref(W)
    assert gap >= U.MIN_GAP, gap
    assert all(len(r) == W for r in ranking)


def test_wide_case_has_a_margin():
    ranking, gap = U.wide_ref()
    assert gap >= U.MIN_GAP, gap
    assert all(len(r) == U.WIDE_W for r in ranking)


@pytest.mark.parametrize("model", sorted(U.LM_MODELS))
@pytest.mark.parametrize("W", U.LM_WIDTHS)
@pytest.mark.parametrize("case_sensitive", [True, False])
def test_lm_cases_have_a_margin(model, W, case_sensitive):
    ranking, gap = U.lm_ref(model, W, case_sensitive)
    assert gap >= U.MIN_GAP, gap
    # the folded look-up finds the same words as the exact one on the lower-case alphabet
    other = U.lm_ref(model, W, not case_sensitive)[0]
    assert [[(h["ids"], h["lm"], h["oov"]) for h in r] for r in ranking] == [[(h["ids"], h["lm"], h["oov"]) for h in r] for r in other]
    assert any(h["oov"] == 0 and h["words"] > 0 for r in ranking for h in r)
    assert any(h["oov"] > 0 for r in ranking for h in r)


def test_restatement_lm_fields_by_hand():
    """a b <1> in tiny_3gram's alphabet spells "abb": an unknown word in the context <s>."""
    lm = U.oracle_lm("tiny_3gram.arpa")
    s = REF.Search(4, 1, 2, None, ["a", "b", " "], lm, True, 1.0, 0.0, 0.0)
    bos = lm.word_index("<s>")
    f = s.child_fields(REF.LmFields((bos,)), None, 0)
    assert f.words == 1 and f.oov == 0 and f.word == "a"
    assert f.lm == lm.base_score([bos], lm.word_index("a"))[0] / REF.LN10
    f2 = s.child_fields(f, 0, 1)
    assert f2.word == "ab" and f2.oov == 0 and f2.lm == lm.base_score([bos], lm.word_index("ab"))[0] / REF.LN10
    f3 = s.child_fields(f2, 1, 3)
    assert f3.word == "abb" and f3.oov == 1 and f3.words == 1
    f4 = s.child_fields(f2, 1, 2)
    assert (f4.lm, f4.oov, f4.words, f4.st) == (f2.lm, f2.oov, f2.words, f2.st)
    f5 = s.child_fields(f4, 2, 0)
    assert f5.words == 2 and f5.word == "a" and f5.lm_before == f2.lm
    assert f5.lm == f2.lm + lm.base_score(list(f2.st), lm.word_index("a"))[0] / REF.LN10


def test_expanded_spelling_of_an_encoding():
    from end2end_amd import ASGEncoder
    enc = ASGEncoder(num_replabels=2)
    ids = enc.encode("hello all").tolist()
    chars = [enc.id2char[i] for i in range(enc.num_chars)]
    assert REF.expand(ids, chars) == "hello all"
    assert REF.spellable(tuple(ids), enc.num_symbols, 2, enc.char2id[" "])
    assert enc.replabel_id(1) in ids


def test_configure_checks():
    import inspect
    from end2end_amd import ASGDecoder, CTCDecoderError
    arpa = os.path.join(U.GOLDEN, "tiny_3gram.arpa")
    params = inspect.signature(ASGDecoder.configure).parameters         # CTCDecoder's names and defaults
    assert [(k, v.default) for k, v in params.items()][1:] == [
        ("beam_width", 1), ("lm_path", None), ("lmwt", 1.0), ("wip", 1.0), ("oov_penalty", -10), ("case_sensitive", True)]

    def make(labels=("a", "b", " "), R=1):
        return ASGDecoder(labels=None if labels is None else list(labels), num_replabels=R)

    d = make()                                                           # as constructed: the best-path decoder
    assert d._beam is None and d._beam_width == 1
    with pytest.raises(CTCDecoderError):
        d.decode_nbest(None, None)
    assert d.configure() is d and d._beam is None and d._beam_width == 1
    with pytest.raises(CTCDecoderError):
        make().configure(beam_width=1, lm_path=arpa)
    with pytest.raises(CTCDecoderError):
        make().configure(beam_width=4, lm_path=os.path.join(U.GOLDEN, "no_such_model.arpa"))
    with pytest.raises(CTCDecoderError):
        make(labels=None).configure(beam_width=4, lm_path=arpa)
    with pytest.raises(CTCDecoderError):
        make().configure(beam_width=0)
    with pytest.raises(ValueError):
        make().configure(beam_width=129)
    d = make().configure(beam_width=128, wip=0.5)
    assert d._beam.beam_width == 128 and d._beam.lmwt == 0.0 and d._beam.wip == 0.5


def test_width_and_alphabet_limits():
    from end2end_amd._runtime import _C
    assert _C.asg_max_labels() == 128
    assert [_C.asg_beam_max_width(V) for V in (1, 29, 128)] == [128, 128, 128]
    assert _C.asg_beam_max_width(129) == 0 and _C.asg_beam_max_width(0) == 0
    assert _C.asg_beam_workspace_bytes(2, 10, 129, 4, False) == 0
    assert _C.asg_beam_workspace_bytes(2, 10, 29, 129, False) == 0
    small, big = _C.asg_beam_workspace_bytes(1, 10, 29, 4, False), _C.asg_beam_workspace_bytes(64, 1000, 29, 100, True)
    assert 0 < small < big and big == 64 * (math.ceil(2900 * 8 / 256) * 256 * 2 + math.ceil(2900 * 4 / 256) * 256
                                            + math.ceil((100 * 1001 + 1) * 8 / 256) * 256) + math.ceil(29 * 29 * 8 / 256) * 256 + 256


def test_argument_errors_come_before_any_launch():
    """Null device pointers throughout: a launch would fault, an argument error returns first."""
    from end2end_amd import _runtime as R
    from end2end_amd._runtime import _C

    def call(V=29, W=4, R_=2, space=0, nbest=1, dtype=None, B=1):
        _C.asg_beam_nbest(0, R.dtype_code(torch.float32) if dtype is None else dtype, 0, 0, 0, 0, 0, B, 10, V,
                          R_, W, space, 0, 1.0, 0.0, 0.0, nbest, 0, 10, 0, 0, 0, 0, 0, 0, 0)

    cases = [(dict(V=129), "e2e_asg_max_labels"), (dict(W=129), "exceeds e2e_asg_beam_max_width"), (dict(W=0), "at least 1"),
             (dict(nbest=5), "nbest"), (dict(R_=29), "num_replabels"), (dict(space=27), "space_id"), (dict(dtype=99), "dtype"),
             (dict(), "null pointer")]
    for kw, text in cases:
        with pytest.raises(Exception) as e:
            call(**kw)
        assert text in str(e.value), (kw, str(e.value))
    call(B=0)                                                       # an empty batch is no error and no launch
