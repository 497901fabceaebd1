"""CPU: pins tests/align_ref.py -- the plain f64 statement of a forced alignment that tests/test_gpu_align_edges.py holds
the kernel to -- before anything runs on a GPU: against exhaustive enumeration, against the labellings upstream's own
functions produced (tests/golden/align.npz), and against the oracle on a few hundred small cases."""
import itertools

import numpy as np
import pytest

import align_ref as AR
import golden_util as G
import oracle_lib as O


def small_case(rng, quantised):
    is_ctc = bool(rng.integers(0, 2))
    V = int(rng.integers(2, 7))
    blank = int(rng.integers(0, V)) if is_ctc else 0
    S = int(rng.integers(1, 9))
    labels = [v for v in range(V) if not (is_ctc and v == blank)]
    tg = rng.choice(labels, size=S)
    if rng.integers(0, 2):                     # doubled labels
        tg[rng.integers(0, S):] = tg[-1]
    need = S + (int((tg[1:] == tg[:-1]).sum()) if is_ctc else 0)
    T = max(2, need + int(rng.integers(0, 3)) * int(rng.integers(0, 8)))
    if quantised:
        lp = AR.quantised(rng, (T, V))
    else:
        x = rng.standard_normal((T, V)) * 2
        lp = x - np.log(np.exp(x).sum(-1, keepdims=True))
        if rng.integers(0, 4) == 0:
            lp = lp.astype(np.float32).astype(np.float64)
    return lp, tg, T, is_ctc, blank


def test_best_score_is_the_maximum_over_all_legal_labellings():
    """Exhaustive: every labelling of V^T that path_cells accepts, scored by path_score; the largest is best_score, exactly
    (both add in frame order), and every labelling path_cells refuses collapses to something else."""
    rng = np.random.default_rng(3)
    for n in range(24):
        is_ctc = n % 2 == 0
        V, T = 3, int(rng.integers(2, 7))
        blank = int(rng.integers(0, V)) if is_ctc else 0
        labels = [v for v in range(V) if not (is_ctc and v == blank)]
        S = int(rng.integers(1, 3 if is_ctc else 4))
        tg = rng.choice(labels, size=S)
        if not AR.feasible(tg, T, is_ctc):
            continue
        lp = AR.quantised(rng, (T, V)) if n % 4 < 2 else np.log(rng.dirichlet(np.ones(V), size=T))
        ext = AR.extended(tg, is_ctc, blank)
        best, legal = -np.inf, 0
        for lab in itertools.product(range(V), repeat=T):
            keep = [lab[0]] + [b for a, b in zip(lab, lab[1:]) if b != a]
            collapsed = [v for v in keep if v != blank] if is_ctc else None
            try:
                cells = AR.path_cells(lab, ext, is_ctc, blank)
            except ValueError:
                if is_ctc:
                    assert collapsed != tg.tolist(), (lab, tg)
                continue
            legal += 1
            assert np.array_equal(ext[cells], lab) and (np.diff(cells) >= 0).all() and (np.diff(cells) <= 2).all()
            if is_ctc:
                assert collapsed == tg.tolist(), (lab, tg)
            best = max(best, AR.path_score(lp, lab))
        assert legal > 0 and best == AR.best_score(lp, ext, T, is_ctc, blank)


def test_path_cells_refuses_illegal_walks():
    ext = AR.extended([1, 1, 2], True, 0)                       # 0 1 0 1 0 2 0
    assert AR.path_cells([1, 0, 1, 2], ext, True, 0).tolist() == [1, 2, 3, 5]
    assert AR.path_cells([0, 1, 0, 1, 2, 0], ext, True, 0).tolist() == [0, 1, 2, 3, 5, 6]
    for bad in ([1, 1, 2, 0],            # the doubled label needs its blank: no +2 onto an equal label
                [0, 1, 0, 1, 0],         # ends before the last label
                [0, 1, 2, 2],            # skips a label
                [2, 1, 0, 1]):           # starts in the wrong cell
        with pytest.raises(ValueError):
            AR.path_cells(bad, ext, True, 0)
    asg = AR.extended([3, 3, 1], False, 0)
    assert AR.path_cells([3, 3, 3, 1], asg, False, 0).tolist() in ([0, 0, 1, 2], [0, 1, 1, 2])
    for bad in ([3, 1, 1], [3, 3, 3], [1, 3, 3, 1]):
        with pytest.raises(ValueError):
            AR.path_cells(bad, asg, False, 0)


def test_quantised_emissions_are_exact_in_every_dtype():
    import torch
    q = AR.quantised(np.random.default_rng(0), (64, 50))
    assert q.min() == -8 and q.max() == 0 and np.array_equal(q * 8, np.round(q * 8))
    for dt in (torch.float16, torch.bfloat16, torch.float32):
        assert np.array_equal(torch.from_numpy(q).to(dt).double().numpy(), q)


@pytest.mark.parametrize("case", G.align_cases(), ids=lambda c: c["name"])
def test_upstreams_labellings_are_legal_and_best(case):
    """tests/golden/align.npz (blank 0): every feasible row of at least two frames is a legal walk of the best score; a
    one-frame row is targets[0] (upstream's quirk) or blank for an empty target; frames past x_len are -100."""
    is_ctc = bool(case["is_ctc"])
    lp = case["lp"].astype(np.float64)
    checked = 0
    for b in range(lp.shape[0]):
        T, S = int(case["x_len"][b]), int(case["t_len"][b])
        tg, out = case["targets"][b, :S], case["out"][b]
        assert (out[T:] == -100).all()
        if T == 1:
            assert out[0] == (tg[0] if S else 0)
        elif AR.feasible(tg, T, is_ctc) and (S or is_ctc):
            AR.check_utterance(lp[b], out, tg, T, is_ctc, 0)
            checked += 1
    assert checked or case["name"] in ("ctc_t1", "ctc_too_few_frames")


@pytest.mark.parametrize("quantised", [False, True], ids=["random", "quantised"])
def test_the_oracles_labellings_are_legal_and_best(quantised):
    """200 small cases each way, any blank, doubled labels, tight and loose: what the oracle returns is a legal walk whose
    score is best_score, exactly."""
    rng = np.random.default_rng(11 + quantised)
    for _ in range(200):
        lp, tg, T, is_ctc, blank = small_case(rng, quantised)
        out = O.ctc_align(lp[None], tg[None], [T], [len(tg)], blank, is_ctc, n_threads=1)[0]
        AR.check_utterance(lp, out, tg, T, is_ctc, blank)
        members = set(tg.tolist()) | ({blank} if is_ctc else set())
        assert set(out.tolist()) <= members
