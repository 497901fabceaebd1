"""The ASG beam search fuzz without a GPU: the margins of the seeded cases tests/test_gpu_asg_beam_fuzz.py compares (at most
3 % of a family may be left out), what the compared cases cover -- asserted, so that a change of the draw cannot lose a
shape quietly --, and the restatement's rule "a candidate whose total is -inf or NaN is no candidate" against brute force.
Every reference is computed once per process (asg_beam_fuzz_util.reference)."""
import math

import numpy as np
import pytest

import asg_beam_fuzz_util as F
import asg_beam_ref as REF
import asg_beam_util as U


def compared_facts(family):
    return [F.facts(family, s) for s in range(F.FAMILIES[family]) if F.compared(family, s)]


@pytest.mark.parametrize("family", sorted(F.FAMILIES))
def test_margins(family):
    n = F.FAMILIES[family]
    left = tuple(s for s in range(n) if not F.compared(family, s))
    gaps = [F.reference(family, s)[1] for s in range(n) if s not in left]
    print(family, "cases", n, "left out", left, "smallest margin %.3g" % min(gaps))
    assert len(left) <= F.LEFT_OUT_CAP * n, left
    assert left == F.LEFT_OUT[family]                                   # (the GPU test is parametrised without them)
    assert all(g >= U.MIN_GAP for g in gaps)


def test_the_draw_is_a_function_of_the_seed():
    F.draw.cache_clear()
    a = F.draw("plain", 17)
    F.draw.cache_clear()
    b = F.draw("plain", 17)
    assert a is not b and np.array_equal(a.x, b.x) and np.array_equal(a.A, b.A) and a.lens == b.lens and a.shape == b.shape
    assert a.x.dtype == np.float32 and a.A.dtype == np.float32


def test_plain_covers_the_cases_it_is_there_for():
    fs = compared_facts("plain")
    cs = [f.case for f in fs]
    assert {c.V for c in cs} == set(F.PLAIN_V) and {c.W for c in cs} == set(F.PLAIN_W)
    assert {(c.V, c.W) for c in cs} >= {(V, W) for V in F.PLAIN_V for W in (31, 32, 33, 64, 127, 128)}
    assert {c.R for c in cs} == {0, 1, 2}
    assert any(c.space >= 0 for c in cs) and any(c.space < 0 for c in cs)
    assert any(0 < c.space < c.V - c.R - 1 for c in cs)
    assert {c.dtype for c in cs} == {"f32", "f64"}
    for flag in ("time_major", "strided", "cpu", "transposed_A"):
        for dt in ("f32", "f64"):
            assert {c.shape[flag] for c in cs if c.dtype == dt} == {True, False}, (flag, dt)
    assert any(c.dtype == "f64" and c.shape["time_major"] and not c.shape["strided"] for c in cs)
    assert {c.x_scale for c in cs} == {1.0, 8.0, 30.0} and {c.a_scale for c in cs} == {0.0, 1.0, 5.0}
    assert {c.wip for c in cs} == {0.0, 0.25} and any(c.no_A for c in cs)
    assert {len(c.lens) for c in cs} == {1, 2, 3, 4}
    assert any(n == 0 for c in cs for n in c.lens) and any(n == c.x.shape[1] + 1 for c in cs for n in c.lens)
    assert any(c.nbest is None for c in cs) and any(c.nbest is not None and c.nbest < c.W for c in cs)
    # full beams at the limits: 128 members that all stay, 128 keys in the table, sel_* filled to the end, 16384 pairs
    assert any(f.full and c.W == 128 and c.V == 128 and c.x.shape[1] >= 3 for f, c in zip(fs, cs))
    assert any(f.full and c.W * c.V >= 16000 and c.x.shape[1] >= 3 for f, c in zip(fs, cs))
    assert any(f.full and c.W == 127 and c.V == 127 for f, c in zip(fs, cs))
    assert any(f.full and c.nbest is not None and c.nbest < c.W and c.W >= 64 for f, c in zip(fs, cs))
    # the non-candidate rule: beams that die beside living ones, beams that never fill
    masked = [f for f in fs if f.case.masked]
    assert len(masked) >= 20
    assert sum(f.dead_beside_living for f in masked) >= 5
    assert any(f.full and f.case.W >= 64 for f in masked)               # -inf shares inside a full, wide beam
    assert sum(f.partial for f in fs) >= 10
    assert any(f.partial and not f.case.masked and f.case.W >= 64 for f in fs)
    # R = 0 and nothing masked: the cases also held against the ASG loss
    assert sum(c.R == 0 and not c.masked for c in cs) >= 20


def test_long_covers_the_cases_it_is_there_for():
    fs = compared_facts("long")
    cs = [f.case for f in fs]
    assert len(fs) >= 5
    assert {c.V for c in cs} == {5, 29} and {c.R for c in cs} == {0, 2} and {c.dtype for c in cs} == {"f32", "f64"}
    assert all(300 <= c.x.shape[1] <= 700 and c.W <= 8 and sorted(c.lens) == [1, c.x.shape[1]] for c in cs)
    assert all(f.full for f in fs)
    assert any(abs(h["total"]) > 1000.0 for f in fs for r in f.ranking for h in r)      # the tolerance is relative
    assert any(len(h["ids"]) > 200 for f in fs for r in f.ranking for h in r)           # a read-out walk of hundreds of nodes


def test_lm_covers_the_cases_it_is_there_for():
    fs = compared_facts("lm")
    cs = [f.case for f in fs]
    hyps = lambda f: [h for r in f.ranking for h in r]
    assert {c.model for c in cs} == set(F.LM_FILES) and {c.W for c in cs} == set(F.LM_W) and {c.R for c in cs} == {0, 1, 2}
    assert {c.lmwt for c in cs} == {0.0, 0.7, 2.0} and {c.wip for c in cs} == {0.0, 0.4} and {c.oov for c in cs} == {-1.3, -1000.0}
    assert {c.case_sensitive for c in cs} == {True, False} and {c.dtype for c in cs} == {"f32", "f64"}
    upper = lambda c: any("A" <= ch <= "Z" for ch in c.chars)
    assert any(upper(c) and not c.case_sensitive for c in cs) and any(not upper(c) for c in cs)
    assert sum(any(h["oov"] == 0 and h["words"] > 0 and h["lm"] != 0.0 for h in hyps(f)) for f in fs) >= 8
    assert sum(any(h["oov"] > 0 for h in hyps(f)) for f in fs) >= 8
    assert any(h["oov"] == 0 and h["words"] > 1 for f in fs for h in hyps(f))                 # a context beyond <s>
    assert any(c.R == 2 and any(i >= c.V - 2 for h in hyps(f) for i in h["ids"]) for f, c in zip(fs, cs))
    assert any(c.space < 0 for c in cs)
    assert any(0 <= c.space < len(c.chars) - 1 for c in cs)             # a space that is not the last character
    assert any(c.W == 128 and f.full for f, c in zip(fs, cs)) and any(c.W > 32 and c.R == 2 for c in cs)
    assert sum(c.masked for c in cs) >= 3 and any(f.partial for f in fs)


# ---- the rule against brute force ------------------------------------------------------------------------------------
@pytest.mark.parametrize("i,seed", [(1, 1), (5, 2)])
def test_masked_restatement_equals_enumeration(i, seed):
    """-inf emissions on a tiny grid: a -inf path contributes nothing, and a labelling whose paths are all masked is absent
    from the enumeration and from the unbounded search alike."""
    V, T, R, space = U.TINY_GRID[i]
    x, A, lens, plain = U.tiny_case(i)
    x = x.copy()
    x[np.random.default_rng(seed).random(x.shape) < 0.35] = -np.inf
    got = REF.beam(x.tolist(), A.tolist(), lens, V, R, space, W=None)[0]
    lost = 0
    for b in range(3):
        want = REF.enumerate_paths(x[b].tolist(), A.tolist(), lens[b], V, R, space)
        assert set(want) <= set(plain[b]) and all(math.isfinite(v) for v in want.values())
        lost += len(plain[b]) - len(want)
        assert {h["ids"] for h in got[b]} == set(want), b
        for h in got[b]:
            assert abs(h["ac"] - want[h["ids"]]) <= 1e-12 * max(1.0, abs(want[h["ids"]])), (b, h)
        assert [h["total"] for h in got[b]] == sorted((h["total"] for h in got[b]), reverse=True)
    assert lost > 0 and any(got)
    # a width too: the masked candidates are dropped before the cut, so a narrow beam is still full of numbers
    narrow = REF.beam(x.tolist(), A.tolist(), lens, V, R, space, W=3)[0]
    assert all(math.isfinite(h["total"]) for r in narrow for h in r)
    assert all(len(narrow[b]) <= min(3, len(got[b])) for b in range(3)) and any(len(r) == 3 for r in narrow)


def test_a_dead_beam_has_no_hypotheses():
    """One frame without a number ends the utterance; NaN counts as -inf does."""
    x = [[0.5, -1.0], [REF.NEG_INF, REF.NEG_INF], [0.25, 0.0]]
    assert REF.beam([x], None, [3], 2, W=4)[0] == [[]]
    assert len(REF.beam([x], None, [1], 2, W=4)[0][0]) == 2
    y = [[0.5, float("nan")], [0.0, float("nan")]]
    out = REF.beam([y], None, [2], 2, W=4)[0][0]
    assert [h["ids"] for h in out] == [(0,)] and out[0]["ac"] == 0.5
    # a member whose label is masked leaves the beam (its stay and its parent's share both carry the -inf); its children stay
    z = [[0.0, 0.0], [REF.NEG_INF, 0.0]]
    out = REF.beam([z], None, [2], 2, W=4)[0][0]
    assert {h["ids"]: h["ac"] for h in out} == {(1,): 0.0, (0, 1): 0.0}


def test_an_exact_tie_at_a_cut_is_a_zero_margin():
    out, gap = REF.beam([[[0.5, 0.5, 0.5]]], None, [1], 3, W=2)
    assert gap == 0.0 and [h["ids"] for h in out[0]] == sorted(((0,), (1,), (2,)), key=REF.key_of)[:2]
    out, gap = REF.beam([[[0.5, 0.25, 0.0]]], None, [1], 3, W=3)        # no cut: the final neighbours' gap
    assert gap == 0.25
