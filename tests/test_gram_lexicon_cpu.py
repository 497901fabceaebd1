"""CPU: the test-side restatement of the Gram-CTC beam search restricted to a vocabulary (tests/gram_lexicon_ref.py) against
the enumeration of all paths filtered by admissible(), the rule against itself over every cut of a sequence into columns, the
timestamps' properties, and the properties of the fixed-seed cases that the GPU tests (tests/test_gpu_gram_lexicon.py) rely
on."""
import itertools
import os
import re

import pytest

import gram_decode_lm_ref as LR
import gram_lexicon_ref as XR
import gram_ref as GR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case_sensitive", [True, False])
@pytest.mark.parametrize("source", XR.TINY_SOURCES, ids=["tiny_3gram", "word_list"])
def test_unbounded_restatement_equals_filtered_enumeration_on_the_tiny_cases(source, case_sensitive):
    """Ranking identical; total, ac and lm to 1e-12 (both sides are f64 sums of at most 625 products of at most 4 factors)."""
    import torch
    F, rule = XR.vocabulary(source, XR.tiny_labels(case_sensitive), case_sensitive)
    dropped = 0
    for i in range(len(LR.TINY_GRID)):
        R, V, l2i, x = LR.tiny_case(i)
        lp = torch.log_softmax(torch.from_numpy(x).double(), -1).numpy()
        want = XR.tiny_enumeration(i, source, case_sensitive)
        got, _ = XR.beam_search(lp, GR.grams_of(R, V, l2i), F, rule, None)
        assert [r["ids"] for r in got] == [r["ids"] for r in want], i
        for g, w in zip(got, want):
            for k in ("total", "ac", "lm"):
                assert abs(g[k] - w[k]) <= 1e-12 * max(1.0, abs(w[k])), (i, g["ids"], k, g[k], w[k])
            assert (g["words"], g["oov"]) == (w["words"], w["oov"])
            assert not XR.timestep_properties(g, x.shape[0]), (i, g)
        everything = LR.tiny_enumeration(i, True, case_sensitive)
        dropped += len(everything) - len(want)
        assert want and len(want) <= len(everything), i           # (T = 2 without grams: all of a, ab, b, ba, ` ` combinations fit)
        assert all(r["oov"] <= 1 for r in want)                   # (only the last word can be unfinished)
    assert dropped > 100


def test_the_two_vocabularies_are_what_the_cases_assume():
    _, rule = XR.vocabulary(LR.TINY_MODEL, XR.tiny_labels(True))
    assert rule.lexicon.words == {b"a", b"ab", b"b", b"ba"} and rule.space_id == 3
    _, lst = XR.vocabulary(tuple(XR.TINY_WORDS), XR.tiny_labels(True))
    assert lst.lexicon.words == {b"ab", b"b"} and lst.lexicon.prefixes == {b"a", b"ab", b"b"}
    # known answers of the rule: a b ` ` b is admissible, a ` ` is not (a is no word of {ab, b}); spaces may follow spaces
    assert XR.admissible((1, 2, 3, 2), lst) and not XR.admissible((1, 3), lst) and not XR.admissible((1, 3, 2), lst)
    assert XR.admissible((3, 3, 2, 3, 3), lst) and XR.admissible((), lst) and XR.admissible((1,), lst)
    _, ab = XR.vocabulary(("a", "b"), XR.tiny_labels(True))
    assert not XR.admissible((1, 2), ab) and XR.admissible((1, 3, 2), ab)
    _, up = XR.vocabulary(tuple(XR.TINY_WORDS), XR.tiny_labels(False), False)
    assert XR.admissible((1, 2, 3, 2), up) and not XR.admissible((1, 3), up)


@pytest.mark.parametrize("source", XR.TINY_SOURCES + (("a", "b"),), ids=["tiny_3gram", "word_list", "letters"])
def test_admissible_agrees_however_a_sequence_is_cut_into_columns(source):
    """Every sequence of up to 5 ids over a, b and the space, every cut of it into grams of 1 to 3 ids: the rule applied
    gram by gram stops somewhere exactly if the sequence is inadmissible, whichever cut is taken."""
    _, rule = XR.vocabulary(source, XR.tiny_labels(True))

    def cuts(n):
        if n == 0:
            yield ()
        for k in range(1, min(3, n) + 1):
            for rest in cuts(n - k):
                yield (k,) + rest

    seen = {True: 0, False: 0}
    for n in range(1, 6):
        for seq in itertools.product((1, 2, 3), repeat=n):
            want = XR.admissible(seq, rule)
            seen[want] += 1
            for cut in cuts(n):
                y, ok = (), True
                for k in cut:
                    ok = ok and rule.gram_allowed(y, seq[len(y):len(y) + k])
                    y = seq[:len(y) + k]
                assert ok == want, (seq, cut)
    assert seen[True] > 20 and seen[False] > 20


def test_pruned_cases_are_decided_by_more_than_rounding_and_their_timestamps_have_the_stated_properties():
    """The smallest gap at any cut and in the final ranking of every pruned case the GPU test runs: >= 1e-6, the project's
    margin for this search.  A case below it is listed in LEFT_OUT and not run on the GPU: at most one in ten."""
    gaps = {}
    for name, W in XR.PRUNED_CASES:
        rows, gaps[(name, W)] = XR.pruned_ref(name, W)
        R, V, l2i, _ = XR.pruned_case(name)
        assert V == 21 and max(len(g) for g in l2i.values()) == 8
        _, rule = XR.vocabulary(XR.PRUNED[name]["source"], tuple(XR.PRUNED[name]["labels"]))
        assert rows[3] == [dict(ids=(), total=0.0, ac=0.0, lm=0.0, words=0, oov=0, frames=())]
        for b, n in enumerate(XR.PRUNED_LENS):
            assert 1 <= len(rows[b]) <= W
            for r in rows[b]:
                assert XR.admissible(r["ids"], rule) and not XR.timestep_properties(r, n), (name, W, b, r)
        # the restriction matters: the unrestricted search of the same input ends with sequences that are not admissible
        free, _ = XR.pruned_ref(name, W, restricted=False)
        assert any(not XR.admissible(r["ids"], rule) for r in free[0])
        # a first value that is not 0 (the empty prefix stayed) and a gram's shared frame both occur
        if W == 2:                                                # (a wide beam takes every first label in at frame 0)
            assert all(r["frames"] and r["frames"][0] > 0 for r in rows[1])
        if W == 32:
            assert any(a == b for r in rows[0] for a, b in zip(r["frames"], r["frames"][1:]))
    below = sorted(k for k, g in gaps.items() if g < XR.MIN_GAP)
    assert below == sorted(XR.LEFT_OUT), gaps
    assert len(below) <= len(XR.PRUNED_CASES) // 10
    assert XR.PRUNED_LENS == [14, 9, 1, 0] and XR.PRUNED_T <= 14


def test_most_tiny_cases_fit_the_widest_beam():
    """The GPU test runs the unpruned restricted search at width 128 and may skip a case with more admissible labellings than
    that: at least 4/5 of the cases fit."""
    for source in XR.TINY_SOURCES:
        fits = [len(XR.tiny_enumeration(i, source, True)) <= LR.PATH_CAP for i in range(len(LR.TINY_GRID))]
        assert sum(fits) >= 0.8 * len(fits), (source, fits)


def test_header_declares_the_opt_entry_as_an_additive_part_of_abi_4():
    hdr = open(os.path.join(ROOT, "include", "e2e_ctc.h")).read()
    assert "#define E2E_CTC_ABI_VERSION 4" in hdr
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"typedef struct e2e_gram_beam_opts \{\s*int restrict_to_lexicon;\s*int64_t\* timesteps;\s*\} e2e_gram_beam_opts;", code)
    m = re.search(r"int\s+e2e_gram_ctc_beam_nbest_opt\s*\(([^)]*)\)", code)
    lm = re.search(r"int\s+e2e_gram_ctc_beam_nbest_lm\s*\(([^)]*)\)", code)
    norm = lambda s: re.sub(r"\s+", " ", s).strip()
    assert m and lm and norm(m.group(1)) == norm(lm.group(1)) + ", const e2e_gram_beam_opts* opts"


def test_library_exports_and_both_layers_bind_the_opt_entry():
    from end2end_amd import _C, _lib
    L = _lib.load()
    assert hasattr(L, "e2e_gram_ctc_beam_nbest_opt") and hasattr(_C, "gram_ctc_beam_nbest_opt")
    assert L.e2e_gram_ctc_beam_nbest_opt.argtypes[:-1] == L.e2e_gram_ctc_beam_nbest_lm.argtypes
    assert [f[0] for f in _lib.GramBeamOpts._fields_] == ["restrict_to_lexicon", "timesteps"]


def test_the_python_surface_checks_its_arguments_without_a_gpu(tmp_path):
    from end2end_amd.decoders import GramCTCDecoder
    from end2end_amd.decoders.gram_ctc_decoder import GramNBestResults
    import torch
    l2i = {4: [1, 2]}

    def dec():
        return GramCTCDecoder(0, 4, 5, l2i, beam_width=4, labels=LR.TINY_LABELS, after_logsoftmax=True)

    with pytest.raises(ValueError, match="configure"):
        dec().restrict_to_vocabulary(["ab"])
    with pytest.raises(ValueError, match=r"configure\(wip=0\)"):
        dec().decode_nbest(torch.zeros(1, 2, 5), timesteps=True)
    assert "timesteps" not in GramNBestResults._fields
    with pytest.raises(ValueError, match="vocabulary"):
        dec().configure(wip=0.4).restrict_to_vocabulary()
    with pytest.raises(ValueError, match="empty"):
        dec().configure(wip=0.4).restrict_to_vocabulary([])
    with pytest.raises(ValueError, match="Can't find a lexicon"):
        dec().configure(wip=0.4).restrict_to_vocabulary(str(tmp_path / "missing.txt"))
    d = dec().configure(wip=0.4)
    assert d._decoder.restricted is False
