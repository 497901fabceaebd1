"""CPU: the vocabulary restriction of the beam search without a GPU -- the checker (tests/lexicon_ref.py) against the C oracle
with the rule off, the lexicon tables against Python sets, the refusals of the wrapper and of the C ABI, lexicon parsing.
(The restricted search itself: tests/test_gpu_lexicon.py.)"""
import os

import numpy as np
import pytest
import torch

import lexicon_ref as LR
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
ARPA = os.path.join(GOLD, "tiny_3gram.arpa")
LABELS4 = ["_", "a", "b", " "]


def rand_lp(seed, B, T, V, sharp=1.5):
    g = torch.Generator().manual_seed(seed)
    return torch.log_softmax(torch.randn(B, T, V, generator=g, dtype=torch.float64) * sharp, -1).numpy()


def test_checker_with_the_rule_off_is_the_c_oracle():
    """V=4, T=25, lengths 25 / 22 / 12, W in {2, 3, 10, 30}, with and without tiny_3gram.arpa, 10 seeds: 240 utterances, none
    left out.  The checker's best hypothesis is the oracle's sentence, id for id."""
    olm = O.OracleLM(ARPA)
    xl = [25, 22, 12]
    n = 0
    for seed in range(10):
        lp = rand_lp(900 + seed, 3, 25, 4)
        for W in (2, 3, 10, 30):
            for lm, kw in ((None, dict(wip=1.0)), (olm, dict(lmwt=0.7, wip=0.5, oov_penalty=-3.0))):
                o_ids, o_lens, _ = O.ctc_beam(lp, xl, 0, W, LABELS4, lm, case_sensitive=True, **kw)
                got, _ = LR.beam(lp, xl, 0, W, LABELS4, lm, True, kw.get("lmwt", 1.0), kw["wip"], kw.get("oov_penalty", -1000.0))
                for b in range(3):
                    assert list(got[b][0]["ids"]) == o_ids[b, : o_lens[b]].tolist(), (seed, W, lm is not None, b)
                    assert len(got[b]) <= W and len({h["ids"] for h in got[b]}) == len(got[b])
                    n += 1
    assert n >= 200


def test_checker_rule_on_toy_case():
    """One frame over `_ a b space` with the lexicon {ab}: `a` may be created (a prefix of ab), `b` may not, the space after
    the root may; a second frame: `ab` yes, `a space` no (a is no word), `aa` no."""
    lp = np.log(np.full((1, 2, 4), 0.25))
    lx = LR.Lexicon(["ab"])
    got, _ = LR.beam(lp, [2], 0, 50, LABELS4, LR.WordListLM(["ab"]), True, 0.0, 0.0, 0.0, lexicon=lx)
    seqs = {h["ids"] for h in got[0]}
    assert seqs == {(-1,), (1,), (3,), (1, 2), (3, 1), (3, 3)}
    by = {h["ids"]: h for h in got[0]}
    assert by[(1, 2)]["oov"] == 0 and by[(1,)]["oov"] == 1 and by[(3, 1)]["words"] == 1


MODELS = [("tiny_3gram.arpa", ["_", "a", "b", " "]), ("lm_order4.arpa", ["_", "a", "b", "c", "d", "e", "'", " "]),
          ("lm_order3_nounk.arpa", ["_", "a", "b", "c", "d", "e", "'", " "])]


def probes(words):
    """Spellings around a word list: the words, their prefixes, one byte more or less, other case, the specials."""
    out = {"<unk>", "<s>", "</s>", "<", "zz", "x"}
    for w in words:
        for n in range(1, len(w) + 1):
            out |= {w[:n], w[:n] + "a", w[:n] + "'", w[:n].upper(), w[:n].capitalize()}
    return sorted(out)


@pytest.mark.parametrize("case_sensitive", [True, False])
@pytest.mark.parametrize("name,labels", MODELS)
def test_lexicon_tables_of_the_golden_models(name, labels, case_sensitive):
    from end2end_amd.engines import LanguageModel
    path = os.path.join(GOLD, name)
    words = LR.arpa_words(path)
    assert len(words) >= 4 and not {"<unk>", "<s>", "</s>"} & set(words)
    lx = LR.Lexicon(words, case_sensitive)
    plain = LanguageModel(path, labels, case_sensitive)
    lm = LanguageModel(path, labels, case_sensitive)
    assert not plain.has_lexicon() and not lm.has_lexicon()
    assert all(plain.spelling_class(s) == 0 for s in probes(words)[:50])          # never asked for: none
    lm.enable_lexicon()
    lm.enable_lexicon()                                                            # idempotent
    assert lm.has_lexicon() and not plain.has_lexicon()
    seen = set()
    for s in probes(words):
        got = lm.spelling_class(s)
        assert got == lx.spelling_class(s), (s, got)
        seen.add(got)
        # what an unrestricted lookup answers is what it answered before: a prefix that is no word is still a miss
        assert lm.word_index(s if case_sensitive else s.lower()) == plain.word_index(s if case_sensitive else s.lower()), s
    # (a, ab, b, ba: every prefix of a word of the tiny model is a word itself)
    assert seen == ({0, 1, 3} if name == "tiny_3gram.arpa" else {0, 1, 2, 3})
    for sp in ("<unk>", "<s>", "</s>"):
        assert lm.spelling_class(sp) == 0                                          # specials are no words
    a, b = lm.word_index("a"), lm.word_index("b")
    assert lm.score([a], b) == plain.score([a], b) and lm.score([], 0) == plain.score([], 0)


@pytest.mark.parametrize("case_sensitive", [True, False])
def test_lexicon_tables_of_a_word_list(case_sensitive):
    """The model that scores nothing: upper case in words and labels, a multi-byte label."""
    from end2end_amd.engines import LanguageModel
    labels = ["_", "A", "b", "é", "ch", " "]
    words = ["Ab", "bé", "chA", "A", "bbéch", "ab"]
    lm = LanguageModel(None, labels, case_sensitive, words=words)
    assert lm.order() == 1 and not lm.has_lexicon() and lm.spelling_class("A") == 0
    assert lm.word_index("<unk>") == 0 and lm.word_index("<s>") != 0 and lm.word_index("</s>") != 0
    for w in words:
        i = lm.word_index(w if case_sensitive else w.lower())
        assert i > 2 and lm.score([], i) == 0.0 and lm.score([lm.word_index("<s>")], i) == 0.0
    assert lm.score([], 0) == 0.0                                                  # <unk> at log10 p = 0
    lm.enable_lexicon()
    lx = LR.Lexicon(words, case_sensitive)
    extra = ["bÉ", "CH", "cH", "bb", "bbé", "bbéc", "B"]
    seen = set()
    for s in probes(words) + extra:
        assert lm.spelling_class(s) == lx.spelling_class(s), s
        seen.add(lm.spelling_class(s))
    assert seen == {0, 1, 2, 3}
    # a byte prefix that ends inside the two-byte character is a prefix all the same (byte prefixes, by the definition)
    assert lm._first.spelling_class(b"b\xc3") == 2 and lm._first.spelling_class(b"\xc3") == 0
    with pytest.raises(Exception, match="white space|empty"):
        LanguageModel(None, labels, True, words=["two words"])


def test_labels_that_spell_a_special_word_inside_the_lexicon_are_refused(tmp_path):
    from end2end_amd.engines import LanguageModel
    from end2end_amd._runtime import E2EError
    lm = LanguageModel(None, ["_", "<s>", "a", " "], True, words=["a"])
    with pytest.raises(E2EError, match="<s>"):
        lm.enable_lexicon()
    assert not lm.has_lexicon()
    # spelled label by label, "<s>" would have to pass "<", which is no allowed spelling: unreachable, accepted
    ok = LanguageModel(None, ["_", "<", "s", ">", "a", " "], True, words=["a"])
    ok.enable_lexicon()
    assert ok.has_lexicon() and ok.spelling_class("<s>") == 0


def test_wrapper_refusals_and_lexicon_parsing(tmp_path):
    from end2end_amd import CTCDecoder, CTCDecoderError
    from end2end_amd.decoders.ctc_decoder import read_lexicon
    from end2end_amd.engines import CTCDecoderEngine
    with pytest.raises(CTCDecoderError, match="needs a vocabulary"):
        CTCDecoder(labels=LABELS4, restrict_to_vocabulary=True)
    with pytest.raises(CTCDecoderError, match="lexicon together with lm_path"):
        CTCDecoder(labels=LABELS4, lm_path=ARPA, lexicon=["a"])
    with pytest.raises(CTCDecoderError, match="beam_width > 1"):
        CTCDecoder(labels=LABELS4, beam_width=1, lexicon=["a"])
    with pytest.raises(CTCDecoderError, match="beam_width > 1"):
        CTCDecoder(labels=LABELS4, beam_width=1, lm_path=ARPA, restrict_to_vocabulary=True)
    with pytest.raises(CTCDecoderError, match="empty"):
        CTCDecoder(labels=LABELS4, lexicon=[])
    with pytest.raises(CTCDecoderError, match="Can't find a lexicon"):
        CTCDecoder(labels=LABELS4, lexicon=str(tmp_path / "none.txt"))
    from end2end_amd.engines import LanguageModel
    shared = LanguageModel(ARPA, LABELS4, False)
    for ctor, kw in ((dict(), dict(restrict_to_vocabulary=True)), (dict(), dict(lexicon=["a"], lm=shared)),
                     (dict(beam_width_=1), dict(lexicon=["a"])), (dict(case_sensitive=True), dict(lm=shared))):
        with pytest.raises(ValueError):
            CTCDecoderEngine(0, **{"beam_width_": 8, "labels": LABELS4, **ctor}).configure(**kw)
    assert CTCDecoderEngine(0, 8, LABELS4).configure().restrict is False
    CTCDecoder(labels=LABELS4)                                                      # the default stays off
    p = tmp_path / "dict.txt"
    p.write_text("ab  AE B\n\nba\tB AE\n  a\nab again\nb\n", encoding="utf-8")
    assert read_lexicon(str(p)) == ["ab", "ba", "a", "b"] == read_lexicon(p)
    assert read_lexicon(iter(["ab  x", "ba", "", "ab"])) == ["ab", "ba"]
    assert read_lexicon(("b",)) == ["b"]


def test_restriction_without_a_lexicon_is_an_argument_error_found_on_the_host():
    """e2e_ctc_beam_nbest_opt: the flag with no model, or with a model whose lexicon was never built, is E2E_ERR_ARG before
    anything is launched or dereferenced (there is no GPU here; the addresses are made up)."""
    from end2end_amd import _C, _lib
    from end2end_amd.engines import LanguageModel
    L = _lib.load()
    assert hasattr(L, "e2e_ctc_beam_nbest_opt") and hasattr(_C.LanguageModel, "from_words")
    B, T, V, W = 2, 20, 4, 10
    args = (256, _C.F32, T * V, V, 1, 256, B, T, V, 0, W, 3)
    tail = (1.0, 0.0, -10.0, W, 256, T + 1, 256, 256, 256, 256, 0, 256, 1 << 30, 0)
    lm = LanguageModel(ARPA, LABELS4, True)
    with pytest.raises(_C.E2EError, match=r"needs a model.*\(code -1\)"):
        _C.ctc_beam_nbest(*args, 0, *tail, restrict_to_lexicon=True)
    with pytest.raises(_C.E2EError, match=r"no lexicon.*\(code -1\)"):
        _C.ctc_beam_nbest(*args, lm._first.handle, *tail, restrict_to_lexicon=True)
    opts = _lib.BeamOpts(1)
    import ctypes as C
    rc = L.e2e_ctc_beam_nbest_opt(256, _lib.F32, T * V, V, 1, 256, B, T, V, 0, W, 3, None, 1.0, 0.0, -10.0, W, 256, T + 1, 256,
                                  256, 256, 256, None, 256, 1 << 30, None, C.byref(opts))
    assert rc == -1 and b"needs a model" in L.e2e_last_error()
