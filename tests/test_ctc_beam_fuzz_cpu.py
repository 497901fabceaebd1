"""The CTC decoder's fuzz without a GPU: the margins of the seeded utterances tests/test_gpu_ctc_beam_fuzz.py compares (at most
LEFT_OUT_CAP of a family's utterances may be left out, and the list is the utility's constant), that the draw is a function of
the seed, that the restatement's first hypothesis is the C oracle's, and what the compared utterances cover -- asserted, so
that a change of the draw cannot lose a shape quietly.  Every reference is computed once per process
(ctc_beam_fuzz_util.reference).  The host queries need the built extension, no GPU."""
import numpy as np
import pytest

import ctc_beam_fuzz_util as F
import lexicon_ref as LR
import oracle_lib as O


def compared_facts(family):
    return [F.facts(family, s) for s in range(F.FAMILIES[family])]


def pairs(fs):
    """(case, facts, compared utterance) of every utterance that has a frame."""
    return [(f.case, f, u) for f in fs for u in f.utts if u.frames > 0]


@pytest.mark.parametrize("family", F.SEARCHES)
def test_margins(family):
    utts = F.utterances(family)
    left = tuple((s, b) for s, b in utts if not F.compared(family, s, b))
    gaps = [F.reference(family, s)[b][1] for s, b in utts if (s, b) not in left]
    secs = [(F.reference(family, s)[b][2].seconds, s, b) for s, b in utts]
    print(family, "cases", F.FAMILIES[family], "utterances", len(utts), "left out", left, "smallest margin %.3g" % min(gaps),
          "reference %.1f s, slowest %.2f s (seed %d, utterance %d)" % ((sum(t for t, _, _ in secs),) + max(secs)))
    assert len(left) <= F.LEFT_OUT_CAP * len(utts), left
    assert left == F.LEFT_OUT[family]                                   # (the GPU test skips exactly these)
    assert all(g >= F.MIN_GAP for g in gaps) and F.MIN_GAP == 1e-7 and F.LEFT_OUT_CAP == 0.03


@pytest.mark.parametrize("fam,seed", [("plain", 17), ("plain", 28), ("long", 2), ("lm", 5), ("lex", 7), ("trans", 11), ("greedy", 11)])
def test_the_draw_is_a_function_of_the_seed(fam, seed):
    F.draw.cache_clear()
    a = F.draw(fam, seed)
    F.draw.cache_clear()
    b = F.draw(fam, seed)
    assert a is not b and a.x.dtype == np.float32 and np.array_equal(a.x, b.x)
    assert not np.isnan(a.x).any()
    va, vb = dict(vars(a)), dict(vars(b))
    for k in ("x", "tied"):
        va.pop(k, None), vb.pop(k, None)
    assert va == vb


@pytest.mark.parametrize("family", ["plain", "lm"])
def test_the_restatement_is_the_oracles_first_hypothesis(family):
    """An independent implementation: with the rule off and no table, hypothesis 0 is oracle_lib.ctc_beam's result."""
    n = 0
    for s in range(F.FAMILIES[family]):
        c = F.draw(family, s)
        ref = F.reference(family, s)
        lens = [F.frames_of(c, b) for b in range(len(c.lens))]
        ids, out_len, _ = O.ctc_beam(c.x.astype(np.float64), lens, c.blank, c.W, c.labels, F.ref_lm(c), c.case_sensitive,
                                     c.lmwt, c.wip, c.oov)
        for b, (ranking, gap, _) in enumerate(ref):
            if gap >= F.MIN_GAP:
                assert tuple(ids[b, :out_len[b]].tolist()) == ranking[0]["ids"], (family, s, b)
                n += 1
    assert n >= 60


def check_call_shapes(cs):
    for flag in ("time_major", "strided", "cpu", "keep_on_device"):
        assert {c.shape[flag] for c in cs if not c.raw} == {True, False}, flag
    assert any(c.raw for c in cs) and any(c.nbest is None for c in cs) and any(c.nbest == 1 for c in cs)
    assert any(c.nbest is not None and 1 < c.nbest < c.W for c in cs)


def test_plain_covers_the_cases_it_is_there_for():
    fs = compared_facts("plain")
    cs = [f.case for f in fs if f.utts]
    ps = pairs(fs)
    assert {c.V for c in cs} == set(F.PLAIN_V)
    want_w = {F.width(w, V, False) for w in F.PLAIN_W for V in F.PLAIN_V}
    assert {c.W for c in cs} == want_w
    assert {(c.V, c.W) for c in cs} == {(V, F.width(w, V, False)) for w in F.PLAIN_W for V in F.PLAIN_V}      # every pair
    assert F.fastcap(29, False) == 150 and F.fastcap(29, True) == 103 and F.fastcap(80, False) == 81 and F.fastcap(1000, False) == 7
    # both kernels; the widths at fastcap and one beyond; both sides of 256
    assert {f.general for f in fs if f.utts} == {True, False}
    for V in (29, 53, 81, 300, 1000):
        cap = F.fastcap(V, False)
        assert any(c.V == V and c.W == cap and not f.general and u.full_run >= 2 for c, f, u in ps), V
        assert any(c.V == V and c.W == cap + 1 and f.general and u.full_run >= 2 for c, f, u in ps), V
    assert {c.W for c, f, u in ps if u.full_run >= 3} >= {7, 33, 64, 100, 256, 257}
    assert any(c.W == 512 and u.full_run >= 1 for c, f, u in ps)
    assert any(f.general and c.W >= 256 and u.full_run >= 3 for c, f, u in ps)
    assert any(not f.general and c.W >= 256 and u.full_run >= 3 for c, f, u in ps)
    assert {c.dtype for c in cs} == {"f32", "f64", "f16", "bf16"} and {c.scale for c in cs} == set(F.PLAIN_SCALES)
    assert {c.wip for c in cs} == set(F.PLAIN_WIP)
    assert any(c.blank == 0 for c in cs) and any(c.blank == c.V - 1 for c in cs) and any(0 < c.blank < c.V - 1 for c in cs)
    assert any(" " in c.labels for c in cs) and any(" " not in c.labels for c in cs)
    assert any(" " in c.labels and c.wip > 0 and any(h["words"] > 1 for h in u.ranking) for c, f, u in ps)
    check_call_shapes(cs)
    assert sum(c.raw for c in cs) >= 25 and any(c.short_out for c in cs)
    assert {len(c.lens) for c in cs} == {1, 2, 3, 4}
    T = lambda c: c.x.shape[1]   # noqa: E731
    assert any(n == 0 for c in cs for n in c.lens) and any(n == 1 and T(c) > 1 for c in cs for n in c.lens)
    assert all(T(c) in c.lens for c in cs) and all(T(c) <= max(1, min(30, F.PLAIN_BUDGET // (c.W * c.V) + 1)) for c in cs)
    # beams that never fill; -inf members inside a full beam; the empty winner; a pruned but living child found again
    assert sum(u.never_full for c, f, u in ps) >= 10
    masked = [(c, f, u) for c, f, u in ps if c.masked]
    assert len({c.seed for c, f, u in masked}) >= 20 and sum(u.search.ninf_in_full > 0 for c, f, u in masked) >= 3
    assert sum(u.empty_winner for c, f, u in ps) >= 3
    assert sum(u.search.q7 > 0 for c, f, u in ps) >= 20
    assert any(u.search.q7 > 0 and f.general for c, f, u in ps) and any(u.search.q7 > 0 and not f.general for c, f, u in ps)
    # tied frames: bit-equal columns, and more of them at the maximum than the general kernel's pre-selection list holds
    tied = [(c, f, u) for c, f, u in ps if c.tie is not None and u.frames > c.tie[0]]
    assert len(tied) >= 20
    for c, f, u in tied:
        t, cols, _ = c.tie
        assert len({c.x[u.b, t, k].tobytes() for k in cols}) == 1
    over = [(c, f, u) for c, f, u in tied if c.overflow]
    assert over and all(f.general and len(c.tie[1]) > 4 * c.W + 64 for c, f, u in over)
    for c, f, u in over:
        assert (c.x[u.b, c.tie[0], c.tie[1]] == c.x[u.b, c.tie[0]].max()).all()
    assert sum(not c.masked and u.n > 0 for c, f, u in ps) >= 100       # ... also held against the CTC loss


def test_long_covers_the_cases_it_is_there_for():
    fs = compared_facts("long")
    cs = [f.case for f in fs]
    assert all(len(f.utts) == 2 for f in fs)
    assert {c.V for c in cs} == {5, 29} and {c.dtype for c in cs} == {"f32", "f64"}
    assert all(300 <= c.x.shape[1] <= 700 and c.W <= 8 and c.timesteps and sorted(c.lens) == [1, c.x.shape[1]] for c in cs)
    hyps = [h for f in fs for u in f.utts for h in u.ranking]
    assert any(len(h["ids"]) > 100 for h in hyps) and any(h["frames"] and h["frames"][-1] > 290 for h in hyps)
    assert all(max(u.full_run for u in f.utts) >= 290 for f in fs)


def scored_coverage(family):
    fs = compared_facts(family)
    cs = [f.case for f in fs if f.utts]
    ps = pairs(fs)
    hyps = [h for f in fs for u in f.utts for h in u.ranking]
    assert {c.dtype for c in cs} == {"f32", "f64"} and {c.wip for c in cs} == set(F.WIP)
    assert {f.general for f in fs if f.utts} == {True, False}                           # both kernels
    assert any(f.general and u.full_run >= 2 for c, f, u in ps)
    check_call_shapes(cs)
    assert any(h["words"] > 1 for h in hyps) and any(h["oov"] > 0 for h in hyps)        # hypotheses with OOV words
    assert sum(c.masked for c in cs) >= 3
    assert any(n == 0 for c in cs for n in c.lens) and any(n == 1 for c in cs for n in c.lens)
    assert any(u.never_full for c, f, u in ps) and any(u.full_run >= 3 for c, f, u in ps)
    assert any(u.search.q7 > 0 for c, f, u in ps)
    return fs, cs, ps, hyps


def spelled_coverage(family):
    fs, cs, ps, hyps = scored_coverage(family)
    assert {c.pad for c in cs} == set(F.LM_PADS) and {c.case_sensitive for c in cs} == {True, False}
    assert {c.upper for c in cs} == {True, False} and any(c.upper and not c.case_sensitive for c in cs)
    want_w = {F.width(w, c.V, True) for c in cs for w in F.LM_W if F.LM_W[c.seed % len(F.LM_W)] == w}
    assert {c.W for c in cs} == want_w and {F.LM_W[c.seed % len(F.LM_W)] for c in cs} == set(F.LM_W)
    # fastcap and fastcap + 1 with a model, on either side of the kernels' boundary
    assert any(c.W == F.fastcap(c.V, True) and not f.general for c, f, u in ps if F.lm_kind(c) != "none")
    assert any(c.W == F.fastcap(c.V, True) + 1 and f.general for c, f, u in ps if F.lm_kind(c) != "none")
    assert any(c.W < 256 for c in cs) and any(c.W >= 256 for c in cs)
    assert any(c.pad and f.general and c.W <= 33 for c, f, u in ps)     # the general kernel at a small width, under a model
    return fs, cs, ps, hyps


def test_lm_covers_the_cases_it_is_there_for():
    fs, cs, ps, hyps = spelled_coverage("lm")
    assert {c.model for c in cs} == set(F.LM_FILES) | {None} and 5 <= sum(c.model is None for c in cs) <= 9
    assert {c.lmwt for c in cs if c.model} == set(F.LMWT) and {c.oov for c in cs if c.model} == set(F.OOV)
    assert {c.timesteps for c in cs} == {True, False}
    assert {(c.model, c.pruned) for c in cs if c.model} == {(m, p) for m in F.LM_FILES for p in (False, True)}
    assert sum(any(h["oov"] == 0 and h["words"] > 0 and h["lm"] != 0.0 for u in f.utts for h in u.ranking) for f in fs) >= 8
    assert any(h["oov"] == 0 and h["words"] > 1 for h in hyps)          # a context beyond <s>


def test_lex_covers_the_cases_it_is_there_for():
    fs, cs, ps, hyps = spelled_coverage("lex")
    assert {c.model for c in cs} == set(F.LM_FILES) and all(c.timesteps and c.restricted for c in cs)
    assert sum(c.words is not None for c in cs) >= 10 and sum(c.words is None for c in cs) >= 10
    assert {c.lmwt for c in cs if c.words is None} == set(F.LMWT) and {c.oov for c in cs if c.words is None} == set(F.OOV)
    assert 7 <= sum(" " not in c.labels for c in cs) <= 11              # a quarter without a space label
    assert any(" " not in c.labels and any(h["oov"] == 1 and h["words"] == 1 for h in u.ranking) for c, f, u in ps)
    assert any(h["frames"] and h["frames"][0] > 0 for h in hyps)
    # a last word that is an unfinished prefix (it counts as out of vocabulary); none before the last
    assert any(h["oov"] == 1 and h["words"] > 1 for h in hyps) and all(h["oov"] <= 1 for h in hyps)
    # the restriction changes the ranking: left to itself, the search ranks otherwise
    bites = 0
    for c, f, u in ps:
        free, _, _ = F.search(c, u.b, n_frames=min(u.frames, 4), restricted=False)
        held, _, _ = F.search(c, u.b, n_frames=min(u.frames, 4), restricted=True)
        bites += [h["ids"] for h in free] != [h["ids"] for h in held]
    assert bites >= 20


def test_trans_covers_the_cases_it_is_there_for():
    fs, cs, ps, hyps = scored_coverage("trans")
    assert {c.model for c in cs} == set(F.LM_FILES) | {None} and {c.restricted for c in cs} == {True, False}
    assert {(c.pruned, c.restricted) for c in cs if c.model} == {(p, r) for p in (False, True) for r in (False, True)}
    assert {c.restricted for c in cs if c.model is None} == {True, False}
    assert {c.timesteps for c in cs} == {True, False}
    for c in cs:
        table = F.table_of(c)
        sizes = sorted(len(v) for v in table.keys.values())
        assert sizes[-1] == min(16, len(F.model_words(c.model or F.LM_FILES[c.seed % 3]))) or c.model is None and sizes[-1] >= 4
        assert any(2 <= n <= 4 for n in sizes[:-1]) and sizes[0] == 1
        assert table.dropped == sum(w.startswith("zz") for w, _ in c.entries) and (table.dropped > 0) == (c.model is not None)
        words = [w for w, _ in c.entries]
        assert len(set(words)) < len(words)                             # variants
        assert any(len(t) > 1 for t in c.labels)                        # multi-character labels
    # a homophone choice that differs between two contexts of one search
    assert sum(any(len(v) > 1 for v in u.search.lm.choices.values()) for c, f, u in ps if c.model) >= 5
    assert any(c.model is None and u.search.lm.choices for c, f, u in ps)
    assert any(c.restricted and h["oov"] == 1 for c, f, u in ps for h in u.ranking)


def test_the_nine_lm_kinds_are_drawn():
    kinds = set()
    for family in ("plain", "lm", "lex", "trans"):
        kinds |= {F.lm_kind(f.case) for f in compared_facts(family) if f.utts}
    assert kinds == {"none"} | {(t, h, r) for t in ("signatures", "id tables") for h in ("spelled", "homophones") for r in (False, True)}


def test_pruned_models_lose_one_listed_context():
    for m in F.LM_FILES:
        full, cut = open(F.model_path(m)).read(), open(F.model_path(m, True)).read()
        assert len(full.split("\n")) == len(cut.split("\n")) + 1
        assert O.OracleLM(F.model_path(m, True)).order() == O.OracleLM(F.model_path(m)).order()
        assert sorted(LR.arpa_words(F.model_path(m, True))) == sorted(F.model_words(m))


def test_greedy_covers_the_cases_it_is_there_for():
    cs = [F.draw("greedy", s) for s in range(F.FAMILIES["greedy"])]
    assert {c.V for c in cs} == set(F.GREEDY_V) and {c.x.shape[1] for c in cs} == set(F.GREEDY_T)
    assert all(c.x.shape[1] <= 65 for c in cs if c.V == 8000) and {c.dtype for c in cs} == set(F.GREEDY_DTYPES)
    for dt in F.GREEDY_DTYPES:
        assert {c.shape["strided"] for c in cs if c.dtype == dt} == {True, False}, dt
        assert any(c.dtype == dt and c.x.shape[1] >= 1023 for c in cs), dt
    assert {c.shape["time_major"] for c in cs} == {True, False}
    assert any(len(set(c.lens)) > 1 for c in cs) and all(1 <= n <= c.x.shape[1] for c in cs for n in c.lens)
    tied = 0
    for c in cs:
        for b, n in enumerate(c.lens):
            top = c.x[b, :n].max(axis=1, keepdims=True)
            k = ((c.x[b, :n] == top).sum(axis=1) > 1).sum()
            assert k >= c.tied[b, :n].sum()
            tied += int(k)
        if c.dtype == "f64":                                            # the C oracle reads the first of equal maxima too
            out, out_len = O.ctc_greedy(c.x.astype(np.float64), c.lens, c.blank)
            for b in range(len(c.lens)):
                assert out[b, :out_len[b]].tolist() == F.greedy_definition(c, b)
    assert tied >= 1000
