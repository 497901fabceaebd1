"""The Gram-CTC decoding fuzz without a GPU: the margins of the seeded utterances tests/test_gpu_gram_beam_fuzz.py compares (at
most a tenth of a family's utterances may be left out, and the list is the utility's constant), that the draw is a function
of the seed, and what the compared utterances cover -- asserted, so that a change of the draw cannot lose a shape quietly.
Every reference is computed once per process (gram_beam_fuzz_util.reference)."""
import numpy as np
import pytest

import gram_beam_fuzz_util as F
import gram_lexicon_ref as XR


def compared_facts(family):
    return [F.facts(family, s) for s in range(F.FAMILIES[family])]


def pairs(fs):
    """(case, compared utterance) of every utterance that has a frame."""
    return [(f.case, u) for f in fs for u in f.utts if u.frames > 0]


@pytest.mark.parametrize("family", F.SEARCHES)
def test_margins(family):
    utts = F.utterances(family)
    left = tuple((s, b) for s, b in utts if not F.compared(family, s, b))
    gaps = [F.reference(family, s)[b][1] for s, b in utts if (s, b) not in left]
    print(family, "cases", F.FAMILIES[family], "utterances", len(utts), "left out", left, "smallest margin %.3g" % min(gaps))
    assert len(left) <= F.LEFT_OUT_CAP * len(utts), left
    assert left == F.LEFT_OUT[family]                                   # (the GPU test skips exactly these)
    assert all(g >= F.MIN_GAP for g in gaps) and F.MIN_GAP == 1e-6


@pytest.mark.parametrize("fam,seed", [("plain", 17), ("long", 2), ("lm", 5), ("lex", 7), ("greedy", 11)])
def test_the_draw_is_a_function_of_the_seed(fam, seed):
    F.draw.cache_clear()
    a = F.draw(fam, seed)
    F.draw.cache_clear()
    b = F.draw(fam, seed)
    assert a is not b and a.x.dtype == np.float32 and np.array_equal(a.x, b.x, equal_nan=True)
    va, vb = dict(vars(a)), dict(vars(b))
    for k in ("x", "tied"):
        va.pop(k, None), vb.pop(k, None)
    assert va == vb


def test_plain_covers_the_cases_it_is_there_for():
    fs = compared_facts("plain")
    cs = [f.case for f in fs if f.utts]
    ps = pairs(fs)
    assert {c.V for c in cs} == set(F.PLAIN_V)
    assert {c.W for c in cs} >= {w for w in F.PLAIN_W if w != "cap"} | {F.max_width(1025), F.max_width(1100)}
    big = [V for V in F.PLAIN_V if V >= 1023]
    assert {(c.V, c.W) for c in cs} >= {(V, min(W, F.max_width(V))) for V in big for W in (31, 32, 33, 64, 100, 127, 128)}
    assert {c.kind for c in cs} == set(F.PLAIN_KINDS)
    orders = lambda c: max([len(g) for g in c.l2i.values()] + [1])   # noqa: E731
    assert {orders(c) for c in cs} >= {1, 2, 3, 8} and any(c.R == c.V and c.V > 3 for c in cs)
    assert {c.dtype for c in cs} == {"f32", "f64"} and {c.scale for c in cs} == set(F.PLAIN_SCALES)
    for flag in ("time_major", "strided", "cpu", "keep_on_device"):
        for dt in ("f32", "f64"):
            assert {c.shape[flag] for c in cs if c.dtype == dt and not c.raw} == {True, False}, (flag, dt)
    assert sum(c.raw for c in cs) >= 30 and any(c.raw and c.V > 1024 for c in cs)
    assert {len(c.lens) for c in cs} == {1, 2, 3, 4}
    T = lambda c: c.x.shape[1]   # noqa: E731
    assert any(n == 0 for c in cs for n in c.lens) and any(n == 1 and T(c) > 1 for c in cs for n in c.lens)
    assert any(n == T(c) + 1 for c in cs for n in c.lens)                # (the header: clamped to T)
    assert any(c.nbest is None for c in cs) and any(c.nbest is not None and c.nbest < c.W for c in cs)
    # full beams at the limits: 128 and 127 members for three frames and more, the pair bound, the cap beyond 1024 columns
    assert any(c.W == 128 and u.full_frames >= 3 for c, u in ps)
    assert any(c.W == 128 and c.V == 1024 and u.full_frames >= 3 for c, u in ps)
    assert any(c.W == 127 and u.full_frames >= 3 for c, u in ps)
    assert any(c.W * c.V >= 120000 and u.full_frames >= 2 for c, u in ps)
    assert any(c.V > 1024 and c.at_cap and c.W == F.max_width(c.V) and u.full_frames >= 2 for c, u in ps)
    assert {c.V for c, u in ps if c.V >= 1023 and u.full_frames >= 2} == set(big)      # a second trip of the column loops
    assert any(c.nbest is not None and c.nbest < c.W and c.W >= 64 and u.n == c.W for c, u in ps)
    # the non-candidate rule: beams that die beside living ones, beams that never fill
    masked = [f for f in fs if f.case.masked]
    assert len(masked) >= 20 and sum(f.dead_beside_living for f in masked) >= 3
    assert any(f.full and f.case.W >= 64 for f in masked)               # zero shares inside a full, wide beam
    assert sum(f.partial for f in fs) >= 10
    assert sum(not c.masked and u.frames > 0 and u.n > 0 for c, u in ps) >= 100       # ... also held against the loss


def test_long_covers_the_cases_it_is_there_for():
    fs = compared_facts("long")
    cs = [f.case for f in fs]
    assert all(len(f.utts) == 2 for f in fs)
    assert {c.V for c in cs} == {21, 33} and {c.dtype for c in cs} == {"f32", "f64"} and {c.scale for c in cs} == set(F.LONG_SCALES)
    assert all(300 <= c.x.shape[1] <= 700 and c.W <= 8 and sorted(c.lens) == [1, c.x.shape[1]] for c in cs)
    assert all(f.full for f in fs)
    # esum grows large where the frames are flat: scale 1 (sharp frames, scale 30, leave the best score near 0).  -994 is an
    # esum of some -1430; the tolerance on such a score is relative
    assert any(h["total"] < -900.0 for f in fs for u in f.utts for h in u.ranking)
    assert any(f.case.scale == 30.0 and -100.0 < u.ranking[0]["total"] < -10.0 for f in fs for u in f.utts)
    assert any(len(h["ids"]) > 200 for f in fs for u in f.utts for h in u.ranking)           # a read-out walk of hundreds of nodes


def scored_coverage(family):
    fs = compared_facts(family)
    cs = [f.case for f in fs if f.utts]
    ps = pairs(fs)
    hyps = [h for f in fs for u in f.utts for h in u.ranking]
    assert {c.W for c in cs} == set(F.LM_W) and {c.dtype for c in cs} == {"f32", "f64"}
    assert {c.wip for c in cs} == set(F.WIP) and {c.case_sensitive for c in cs} == {True, False}
    assert {c.upper for c in cs} == {True, False} and any(c.upper and not c.case_sensitive for c in cs)
    assert any(c.space < 0 for c in cs) and any(1 <= c.space < c.R - 1 for c in cs)
    # grams with an inner, a leading and a trailing space -- and results that took them
    inner = lambda c, g: c.space in g[1:-1]   # noqa: E731
    assert sum(any(inner(c, g) for g in c.l2i.values()) for c in cs) >= 10
    assert any(g[0] == c.space and len(g) > 1 for c in cs for g in c.l2i.values())
    assert any(g[-1] == c.space and len(g) > 1 for c in cs for g in c.l2i.values())
    assert any(h["words"] > 1 for h in hyps)
    assert any(c.V >= 150 and c.W >= 100 and u.full_frames >= 3 for c, u in ps)          # a wide table under a wide beam
    assert any(c.raw for c in cs) and any(c.nbest is not None and c.nbest < c.W and c.W >= 64 for c in cs)
    # the row hand-over at 128 and 127 members; frames in which the new members outnumber those that stay, and frames in which
    # all stay (the floor filter's n_stay == W)
    assert any(c.W == 128 and u.full_frames >= 3 for c, u in ps) and any(c.W == 127 and u.full_frames >= 3 for c, u in ps)
    assert any(c.W >= 100 and any(new > stay for _, stay, new in u.moves) for c, u in ps)
    assert any(c.W >= 100 and any(was == c.W and new > stay for was, stay, new in u.moves) for c, u in ps)
    assert any(c.W >= 100 and any(was == c.W == stay for was, stay, _ in u.moves) for c, u in ps)
    assert any(c.W >= 100 and any(was == c.W and 0 < new < stay for was, stay, new in u.moves) for c, u in ps)
    assert sum(c.masked for c in cs) >= 3 and any(f.partial for f in fs)
    assert sum(f.dead_beside_living for f in fs if f.case.masked) >= 1  # a dead scored beam beside a living one
    # members that stay with a total of zero inside a full beam of 100 and more (a frame of one letter's column): they are no
    # candidates and do not count towards n_stay == W, and the W-th survivor lies below the least member that lives on
    trapped = [(c, u) for c, u in ps if u.dead_stays_in_a_full_beam]
    assert len(trapped) >= 4 and all(c.W >= 100 and c.sparse_frame is not None for c, u in trapped)
    assert {c.W for c, u in trapped} == {100, 127, 128}
    return fs, cs, ps, hyps


def test_lm_covers_the_cases_it_is_there_for():
    fs, cs, ps, hyps = scored_coverage("lm")
    assert {c.model for c in cs} == set(F.LM_FILES) | {None} and 4 <= sum(c.model is None for c in cs) <= 8
    assert {c.lmwt for c in cs if c.model} == set(F.LMWT) and {c.oov for c in cs if c.model} == set(F.OOV)
    assert {c.timesteps for c in cs} == {True, False}
    assert sum(any(h["oov"] == 0 and h["words"] > 0 and h["lm"] != 0.0 for u in f.utts for h in u.ranking) for f in fs) >= 8
    assert sum(any(h["oov"] > 0 for u in f.utts for h in u.ranking) for f in fs) >= 8
    assert any(h["oov"] == 0 and h["words"] > 1 for h in hyps)          # a context beyond <s>


def test_lex_covers_the_cases_it_is_there_for():
    fs, cs, ps, hyps = scored_coverage("lex")
    assert {c.model for c in cs} == set(F.LM_FILES) and all(c.timesteps and c.restricted for c in cs)
    assert sum(c.words is not None for c in cs) >= 10 and sum(c.words is None for c in cs) >= 10
    assert {c.lmwt for c in cs if c.words is None} == set(F.LMWT) and {c.oov for c in cs if c.words is None} == set(F.OOV)
    assert any(len(set(h["frames"])) < len(h["frames"]) for h in hyps)  # the ids of one gram share a frame
    assert any(h["frames"] and h["frames"][0] > 0 for h in hyps)
    # what the draw found (seeds 10 and 27): no space label, so space_id is -1.  Seed 10 (a model's words) ends with results
    # whose one word is unfinished -- a proper prefix of a word that is no word itself, counted as out of vocabulary; seed 27
    # (the word list ab, b, ba) with words of two ids, which single ids spell only through the unfinished `a`
    for seed in (10, 27):
        assert fs[seed].case.seed == seed and fs[seed].case.space < 0 and fs[seed].utts
    assert fs[10].case.words is None and fs[27].case.words == ["ab", "b", "ba"]
    assert any(h["oov"] == 1 and h["words"] == 1 and h["ids"] for u in fs[10].utts for h in u.ranking)
    assert any(h["oov"] == 0 and len(h["ids"]) == 2 for u in fs[27].utts for h in u.ranking)
    # the restriction bites: left to itself, the search keeps a sequence that is not admissible.  (Up to the first frame at
    # which it does, both searches hold the same beam: that sequence was a candidate there and made the cut)
    bites = 0
    for f in fs:
        c = f.case
        rule = F.fields_and_rule(c)[1]
        for u in f.utts:
            if u.frames:
                free, _, _ = F.search(c, u.b, n_frames=min(u.frames, 3), restricted=False)
                bites += any(not XR.admissible(h["ids"], rule) for h in free)
    assert bites >= 20


def test_greedy_covers_the_cases_it_is_there_for():
    cs = [F.draw("greedy", s) for s in range(F.FAMILIES["greedy"])]
    assert {(c.V, c.x.shape[1]) for c in cs} == {(V, T) for V in F.GREEDY_V for T in F.GREEDY_T}
    assert {c.dtype for c in cs} == set(F.GREEDY_DTYPES) and {c.kind for c in cs} == set(F.PLAIN_KINDS)
    for dt in F.GREEDY_DTYPES:
        assert any(c.dtype == dt and c.V == 1025 for c in cs) and any(c.dtype == dt and c.x.shape[1] >= 63 for c in cs), dt
    assert {c.shape["time_major"] for c in cs} == {True, False} and {c.shape["strided"] for c in cs} == {True, False}
    assert any(len(set(c.lens)) > 1 for c in cs) and all(1 <= n <= c.x.shape[1] for c in cs for n in c.lens)
    tied = 0
    for c in cs:
        for b, n in enumerate(c.lens):
            top = c.x[b, :n].max(axis=1, keepdims=True)
            tied += int(((c.x[b, :n] == top).sum(axis=1) > 1).sum())
            assert ((c.x[b, :n] == top).sum(axis=1) > 1).sum() >= c.tied[b, :n].sum()
    assert tied >= 100
    assert any(c.x[b, t, 0] == c.x[b, t].max() and c.tied[b, t] for c in cs for b in range(len(c.lens)) for t in range(c.lens[b]))
