"""CPU: custom transcriptions without a GPU -- the loader's host tables (kept and dropped entries, label-id keys, homophone
sets), every refusal with its message, the host helper e2e_lm_transcribe against the checker's choice, the tie rule of the
model that scores nothing, the lexicon on label boundaries, and the checker (tests/transcription_ref.py) against totals worked
out by hand.  (The search itself: tests/test_gpu_transcriptions.py.)"""
import math
import os
import warnings

import numpy as np
import pytest

import lexicon_ref as LR
import oracle_lib as O
import transcription_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARPA = os.path.join(ROOT, "tests", "golden", "tiny_3gram.arpa")
LABELS5 = ["_", "p", "q", "r", " "]
# tiny_3gram lists a, ab, b, ba.  `ab` and `b` collide on "p q"; `ba` has two variants; `zz` is outside the model.
ENTRIES = [("a", "p"), ("ab", "p q"), ("b", "p q"), ("ba", "q p"), ("ba", "r"), ("zz", "q q")]


def model(entries=ENTRIES, labels=LABELS5, path=ARPA, case_sensitive=True, **kw):
    from end2end_amd.engines import LanguageModel
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return LanguageModel(path, labels, case_sensitive, transcriptions=entries, blank_idx=0, **kw)


def test_loader_keeps_variants_and_homophones_and_drops_words_outside_the_model():
    from end2end_amd.engines import LanguageModel
    with pytest.warns(UserWarning, match="1 of 6 entries dropped"):
        lm = LanguageModel(ARPA, LABELS5, True, transcriptions=ENTRIES, blank_idx=0)
    plain = LanguageModel(ARPA, ["_", "a", "b", " "], True)
    assert lm.is_transcribed() and not plain.is_transcribed()
    assert lm.transcriptions_dropped() == 1 and plain.transcriptions_dropped() == 0
    assert lm.order() == 3 and lm._first.device() == -1            # host tables only: there is no GPU here
    # the words, their ids and their scores are the model's
    for w in ("<unk>", "<s>", "</s>", "a", "ab", "b", "ba", "zz"):
        assert lm.word_index(w) == plain.word_index(w), w
        assert lm._first.word_string(lm.word_index(w)) == (w if w != "zz" else "<unk>")
    assert lm._first.word_string(99) is None
    a, b = lm.word_index("a"), lm.word_index("b")
    assert lm.score([a], b) == plain.score([a], b)
    # every kept key: one word, a variant pair, <unk> for what is no key or a proper prefix only
    sp = 4
    assert lm.transcribe([1], sp) == ["a"] and lm.transcribe([2, 1], sp) == ["ba"] and lm.transcribe([3], sp) == ["ba"]
    assert lm.transcribe([2], sp) == ["<unk>"] and lm.transcribe([2, 2], sp) == ["<unk>"]      # a prefix only; dropped
    assert lm.transcribe([1, 2, 1], sp) == ["<unk>"] and lm.transcribe([], sp) == [] and lm.transcribe([4, 4], sp) == []
    # an entry listed twice is one word of its key; the text file and the mapping read the same entries
    twice = model(ENTRIES + [("b", "p q"), ("a", "p")])
    assert twice.transcriptions_dropped() == 1 and twice.transcribe([1, 2], sp) == lm.transcribe([1, 2], sp)


def test_text_file_mapping_and_iterable_are_the_same_lexicon(tmp_path):
    from end2end_amd.engines import read_transcriptions
    p = tmp_path / "lexicon.txt"
    p.write_text("a p\n\nab\tp  q\nb p q\nba q p\nba r\nzz q q\n", encoding="utf-8")
    want = [("a", [1]), ("ab", [1, 2]), ("b", [1, 2]), ("ba", [2, 1]), ("ba", [3]), ("zz", [2, 2])]
    assert read_transcriptions(str(p), LABELS5, 0) == want == read_transcriptions(ENTRIES, LABELS5, 0)
    mapping = {"a": "p", "ab": ["p", "q"], "b": "p q", "ba": [["q", "p"], ["r"]], "zz": ["q", "q"]}
    assert read_transcriptions(mapping, LABELS5, 0) == want


def test_keys_are_label_ids_not_concatenated_strings():
    """Labels A, AH, HK, K: `A HK` and `AH K` both spell AHK and are different words."""
    labels = ["_", "A", "AH", "HK", "K", " "]
    lm = model([("a", "A HK"), ("b", "AH K")], labels)
    assert lm.transcribe([1, 3], 5) == ["a"] and lm.transcribe([2, 4], 5) == ["b"]
    assert lm.transcribe([1, 3, 5, 2, 4], 5) == ["a", "b"]
    assert lm.transcribe([1, 4], 5) == ["<unk>"] and lm.transcribe([2, 3], 5) == ["<unk>"]
    lm.enable_lexicon()
    assert lm.transcribe([1, 3, 5, 2, 4], 5) == ["a", "b"] and lm.transcribe([1], 5) == ["<unk>"]


def test_every_refusal_names_its_cause():
    from end2end_amd import _C
    from end2end_amd.engines import LanguageModel
    with pytest.raises(ValueError, match=r"entry 1 \(b\).*'x' is none of the labels"):
        model([("a", "p"), ("b", "p x")])
    with pytest.raises(ValueError, match=r"entry 0 \(a\).*blank"):
        model([("a", "p _")])
    with pytest.raises(ValueError, match=r"entry 2 \(ab\).*space"):
        model([("a", "p"), ("b", "q"), ("ab", ["p", " ", "q"])])
    with pytest.raises(ValueError, match="empty"):
        model([])
    with pytest.raises(ValueError, match=r"entry 0 \(a\) has no tokens"):
        model([("a", [])])
    with pytest.raises(ValueError, match="exclude"):
        LanguageModel(None, LABELS5, True, words=["a"], transcriptions=ENTRIES)
    # the C ABI's own checks, past the Python parser
    load = _C.LanguageModel.from_transcriptions
    with pytest.raises(_C.E2EError, match=r"lexicon is empty.*\(code -1\)"):
        load(ARPA, [], [], [0], LABELS5, True)
    with pytest.raises(_C.E2EError, match=r"entry 1 \(b\): 5 is no label id.*\(code -1\)"):
        load(ARPA, ["a", "b"], [1, 5], [0, 1, 2], LABELS5, True)
    with pytest.raises(_C.E2EError, match=r"entry 0 \(a\): the space.*\(code -1\)"):
        load(ARPA, ["a"], [1, 4], [0, 2], LABELS5, True)
    with pytest.raises(_C.E2EError, match=r"entry 1 \(b\) has no labels.*\(code -1\)"):
        load(ARPA, ["a", "b"], [1], [0, 1, 1], LABELS5, True)
    with pytest.raises(_C.E2EError, match=r"entry 0: <s> has no transcription.*\(code -1\)"):
        load(ARPA, ["<s>"], [1], [0, 1], LABELS5, True)
    with pytest.raises(_C.E2EError, match=r"entry 0 \(a\) has 256 labels: at most 255.*\(code -2\)"):
        load(ARPA, ["a"], [1] * 256, [0, 256], LABELS5, True)
    assert load(ARPA, ["a"], [1] * 255, [0, 255], LABELS5, True).is_transcribed()
    with pytest.raises(_C.E2EError, match=r"65536 labels.*at most 65535.*\(code -2\)"):
        load("", ["a"], [1], [0, 1], ["_"] + ["t%d" % i for i in range(65534)] + [" "], True)
    words = ["w%d" % i for i in range(17)]
    with pytest.raises(_C.E2EError, match=r"entry 16 \(w16\): more than 16 words share.*\(code -2\)"):
        load("", words, [1] * 17, list(range(18)), LABELS5, True)
    assert load("", words[:16], [1] * 16, list(range(17)), LABELS5, True).transcriptions_dropped() == 0


def test_the_homophone_choice_flips_with_the_context():
    """`ab` and `b` share "p q".  At the start log10 p(ab | <s>) = -1.4 beats p(b | <s>) = -1.6; behind `a`, p(b | <s> a) = -0.2
    beats p(ab | a) + backoff(<s> a) = -1.0 (the gaps of this fixture are >= 0.1, far above f32 round-off)."""
    lm, olm = model(), O.OracleLM(ARPA)
    t = TR.Table(ENTRIES, LABELS5, olm)
    assert t.dropped == 1 and t.keys[(1, 2)] == [olm.word_index("ab"), olm.word_index("b")]
    s0 = [olm.word_index("<s>")]
    assert olm.base_score(s0, olm.word_index("ab"))[0] - olm.base_score(s0, olm.word_index("b"))[0] > 0.1
    s1 = [olm.word_index("a")] + s0
    assert olm.base_score(s1, olm.word_index("b"))[0] - olm.base_score(s1, olm.word_index("ab"))[0] > 0.1
    sp = 4
    assert lm.transcribe([1, 2], sp) == ["ab"]
    assert lm.transcribe([1, sp, 1, 2], sp) == ["a", "b"]
    assert lm.transcribe([1, 2, sp, 1, sp, 1, 2, sp, 1, 2], sp) == ["ab", "a", "b", "ab"]
    # ... and every sequence of up to four pieces is the checker's choice, id for id
    pieces = [(1,), (1, 2), (2, 1), (3,), (2,), (2, 2)]
    rng = np.random.RandomState(7)
    for _ in range(200):
        ids = []
        for k in rng.randint(0, len(pieces), size=rng.randint(1, 5)):
            ids += list(pieces[k]) + [sp] * rng.randint(1, 3)
        want = TR.words_of(ids, LABELS5, olm, t)
        assert [lm.word_index(w) for w in lm.transcribe(ids, sp)] == want, ids
    # the lower-cased match of case_sensitive=False
    folded = model([("A", "p"), ("AB", "p q"), ("B", "p q")], case_sensitive=False)
    assert folded.transcriptions_dropped() == 0 and folded.transcribe([1, sp, 1, 2], sp) == ["a", "b"]
    assert model([("A", "p")]).transcriptions_dropped() == 1


def test_the_model_that_scores_nothing_gives_the_first_listed_homophone():
    entries = [("there", "p q"), ("their", "p q"), ("they're", "p q"), ("the", "p"), ("Their", "r")]
    lm = model(entries, path=None)
    assert lm.order() == 1 and lm.transcriptions_dropped() == 0
    i = lm.word_index("their")
    assert i > 2 and lm.score([], i) == 0.0 and lm.score([lm.word_index("<s>")], i) == 0.0
    assert lm.transcribe([1, 2, 4, 1, 4, 1, 2, 4, 3], 4) == ["there", "the", "there", "Their"]
    rev = model(list(reversed(entries)), path=None)
    assert rev.transcribe([1, 2, 4, 1, 2], 4) == ["they're", "they're"]
    # folded: Their is their, so "r" is a variant of it and "p q" lists it once
    f = model(entries, path=None, case_sensitive=False)
    assert f.transcribe([3, 4, 1, 2], 4) == ["their", "there"]


def test_the_lexicon_is_the_kept_transcriptions_on_label_boundaries():
    """Restricted or not, what a lookup answers stays; a key's label-boundary prefixes enter the tables as <unk>; a
    transcription model cannot spell <unk>, <s> or </s>, so labels that could are not refused."""
    from end2end_amd import _C
    labels = ["_", "<s>", "q", "r", " "]
    lm = model([("a", "<s>"), ("ab", "<s> q r"), ("b", "<s> q r"), ("ba", "r q")], labels)
    before = [lm.transcribe(list(k), 4) for k in ((1,), (1, 2), (1, 2, 3), (3,), (3, 2), (2,))]
    assert not lm.has_lexicon()
    lm.enable_lexicon()
    lm.enable_lexicon()
    assert lm.has_lexicon() and lm.spelling_class("a") == 0
    assert before == [lm.transcribe(list(k), 4) for k in ((1,), (1, 2), (1, 2, 3), (3,), (3, 2), (2,))]
    assert before == [["a"], ["<unk>"], ["ab"], ["<unk>"], ["ba"], ["<unk>"]]
    # a restricted call on a model whose lexicon was never built is an argument error found on the host
    plain = model()
    args = (256, _C.F32, 20 * 5, 5, 1, 256, 2, 20, 5, 0, 10, 4)
    tail = (1.0, 0.0, -10.0, 10, 256, 21, 256, 256, 256, 256, 0, 256, 1 << 30, 0)
    with pytest.raises(_C.E2EError, match=r"no lexicon.*\(code -1\)"):
        _C.ctc_beam_nbest(*args, plain._first.handle, *tail, restrict_to_lexicon=True)


def test_wrappers_refuse_what_is_not_supported():
    from end2end_amd import CTCDecoder, CTCDecoderError, GramCTCDecoder
    with pytest.raises(CTCDecoderError, match="lexicon together with transcriptions"):
        CTCDecoder(labels=LABELS5, transcriptions=ENTRIES, lexicon=["a"])
    with pytest.raises(CTCDecoderError, match="beam_width > 1"):
        CTCDecoder(labels=LABELS5, beam_width=1, transcriptions=ENTRIES)
    with pytest.raises(CTCDecoderError, match="custom transcriptions"):
        GramCTCDecoder(num_base_labels=3, total_labels=3, transcriptions=ENTRIES)
    # ASGDecoder loads its own model from lm_path and has no way to be given one; e2e_asg_beam_nbest refuses a transcription
    # model on the host (the addresses are made up)
    from end2end_amd import _C
    B, T, V, W = 1, 6, 5, 4
    with pytest.raises(_C.E2EError, match=r"custom transcriptions.*\(code -2\)"):
        _C.asg_beam_nbest(256, _C.F32, T * V, V, 1, 256, 256, B, T, V, 0, W, 4, model()._first.handle, 1.0, 0.0, -10.0, W, 256, T,
                          256, 256, 256, 256, 256, 1 << 24, 0)


def test_checker_against_totals_worked_out_by_hand():
    """Three uniform frames over `_ p q space`; a: q, ab: p, b: p; lmwt 0.7, wip 0.5, nothing pruned.
    (p): six of the 27 paths; the word is ab (-0.9 + backoff(<s>) -0.5 beats b's -1.1 - 0.5).
    (q, space, p): one path; a scores p(a | <s>) = -0.4, then b (p(b | <s> a) = -0.2) beats ab (-0.9 - 0.1).
    (p, space, p): one path; ab, then ab again (-0.9 - 0.2 beats -1.1 - 0.2)."""
    labels = ["_", "p", "q", " "]
    olm = O.OracleLM(ARPA)
    t = TR.Table([("a", "q"), ("ab", "p"), ("b", "p")], labels, olm)
    lp = np.log(np.full((1, 3, 4), 0.25))
    got, _ = TR.beam(lp, [3], 0, 200, labels, olm, t, lmwt=0.7, wip=0.5, oov_penalty=-3.0)
    by = {h["ids"]: h for h in got[0]}
    f, ln10 = np.float32, math.log(10.0)

    def total(paths, scores, words, oov=0):
        lm = 0.0
        for s in scores:
            lm = lm + float(s) / ln10
        return math.log(paths / 64.0) + 0.7 * lm - 0.5 * words - 3.0 * oov, lm

    for ids, paths, scores, words in (((1,), 6, [f(-0.9) + f(-0.5)], 1),
                                      ((2, 3, 1), 1, [f(-0.4), f(-0.2)], 2),
                                      ((1, 3, 1), 1, [f(-0.9) + f(-0.5), f(-0.9) + f(-0.2)], 2)):
        want, lm = total(paths, scores, words)
        h = by[ids]
        assert abs(h["total"] - want) < 1e-12 and abs(h["lm"] - lm) < 1e-12, (ids, h, want)
        assert (h["words"], h["oov"]) == (words, 0)
    # (q, q) is no key: one out-of-vocabulary word at <unk>'s unigram -1.0 + backoff(<s>)
    want, lm = total(1, [f(-1.0) + f(-0.5)], 1, oov=1)
    assert abs(by[(2, 2)]["total"] - want) < 1e-12 and by[(2, 2)]["oov"] == 1
    # restricted: `q q` is no prefix of a key and is never created; a space needs a whole word before it
    res, _ = TR.beam(lp, [3], 0, 200, labels, olm, t, restrict=True, lmwt=0.7, wip=0.5, oov_penalty=-3.0)
    seqs = {h["ids"] for h in res[0]}
    assert (2, 2) not in seqs and (2, 3, 1) in seqs and (1, 3, 1) in seqs and (1, 1) not in seqs
    assert {h["ids"]: h["total"] for h in res[0] if h["ids"] in by} == {k: by[k]["total"] for k in seqs if k in by}
