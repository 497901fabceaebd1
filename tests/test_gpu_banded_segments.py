"""-m gpu: the banded segment kernel (targets tensors of 128..255 columns: two label pairs per lane over the 128 pairs of the
lattice that carry the segment's posterior mass; end2end_amd/csrc/ctc_loss_fast.hip, segment_wave_band) against the oracle.

Every case is held to the default tolerances -- losses 6e-7 relative, gradients 2e-6 + 1e-4 |g| -- and reads the call's flag
words (e2e_debug_fast_state) to state which path produced the result: 0 = the fast path's own kernels, bit 8 = a segment was
redone in f64 by the flagged launch.  The window the kernel derives is restated on the CPU by tools/diag/band_width.py
(rule_windows: the same rule on f64 cells), which the tests use to show that a case exercises what it is meant to."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import oracle_lib as O
import gpu_util as U
from end2end_amd import _lib

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "diag"))
import band_width as BW  # noqa: E402

pytestmark = pytest.mark.gpu

LOSS_RTOL = 6e-7
GRAD_RTOL, GRAD_ATOL = 1e-4, 2e-6
V = 29


def fast_flags(keep, B, T):
    L = _lib.load()
    flags, logz = (ctypes.c_int * B)(), (ctypes.c_double * (2 * B))()
    assert L.e2e_debug_fast_state(keep["workspace"].data_ptr(), B, T, V, keep["Smax"], flags, logz) == 0
    return np.array(list(flags))


def band_misses(keep, B, T):
    L = _lib.load()
    n = ctypes.c_int(-1)
    assert L.e2e_debug_band_misses(keep["workspace"].data_ptr(), B, T, V, keep["Smax"], ctypes.byref(n)) == 0
    return n.value


def reference(x, tg, xl, tl, logprobs=False):
    """the oracle's losses and the gradient the call returns: d loss / d logits (zero past an utterance's frames) for logits"""
    lp = np.asarray(x, dtype=np.float64) if logprobs else BW.log_softmax(x)
    l_o, g_o = O.ctc_loss(lp, tg, xl, tl, 0)
    if not logprobs:
        for b in range(len(xl)):
            g_o[b, xl[b]:] = 0.0
    return lp, l_o, g_o


def run_and_compare(x, tg, xl, tl, want_flags=None, logprobs=False, ref=None):
    B, T, _ = x.shape
    lp, l_o, g_o = ref if ref is not None else reference(x, tg, xl, tl, logprobs)
    keep = {}
    la, ga = U.c_abi_loss(torch.from_numpy(np.asarray(x, dtype=np.float32)), tg, xl, tl, 0, logprobs, _lib.ALGO_AUTO, keep=keep)
    assert keep["route"] % 100 // 10 == 4 and keep["route"] // 1000 == 2, "not the fast path's four-pair lattice: %d" % keep["route"]
    flags = fast_flags(keep, B, T)
    print("flags", flags.tolist(), "band misses", band_misses(keep, B, T),
          "max |dloss|/loss %.3g" % np.max(np.abs(la - l_o) / np.abs(l_o)), "max |dgrad| %.3g" % np.max(np.abs(ga - g_o)))
    U.assert_same(la, l_o, LOSS_RTOL, 0.0, "losses")
    U.assert_same(ga, g_o, GRAD_RTOL, GRAD_ATOL, "grads")
    if want_flags is not None:
        assert flags.tolist() == list(want_flags), "flag words %s" % flags.tolist()
    return keep, flags, lp


def random_case(seed, T, S, lengths, xl=None, scale=1.0):
    rng = np.random.default_rng(seed)
    B = len(lengths)
    x = (rng.standard_normal((B, T, V)) * scale).astype(np.float32)
    tg = rng.integers(1, V, size=(B, S))
    return x, tg, np.full(B, T) if xl is None else np.asarray(xl), np.asarray(lengths)


# S: the width of the targets tensor (what selects the kernels).  At T = 200 a target of 223 labels has no alignment, so the
# longest target of that case is the longest that 200 frames hold with its repeats.
@pytest.mark.parametrize("T,S,lengths", [(200, 128, (128, 97)), (200, 160, (160, 131)), (200, 223, (188, 150)), (203, 160, (160, 131))],
                         ids=["T200_S128", "T200_S160", "T200_S223", "T203_S160"])
def test_lattice_ends_and_interior_windows(T, S, lengths):
    """Unit-variance logits.  The first and the last segment hold cell 0 and cell L-1; interior segments have a window that
    starts above pair 0 (shown with the CPU restatement); T = 203: a last segment of 11 steps.  No utterance flagged."""
    x, tg, xl, tl = random_case(100 + T + S, T, S, lengths)
    keep, flags, lp = run_and_compare(x, tg, xl, tl, want_flags=[0] * len(lengths))
    la, lq, lz, _ = BW.lattice(lp[0], tg[0, :tl[0]])
    win = BW.rule_windows(la, lq, lz, int(tl[0]))
    assert win[0][0] == 0 and win[-1][1] == tl[0] // 4 and all(w[2] for w in win)
    assert any(lo > 0 for lo, _, _ in win[1:-1]), "no interior window starts above pair 0"
    assert band_misses(keep, len(lengths), T) == 0


def test_barely_feasible_targets_with_long_runs():
    """T = S + (adjacent repeats) -- one alignment, a band one cell wide along the diagonal -- and three frames more; the targets
    are runs of up to 12 equal labels, so that the window's label slots hold many equal labels."""
    rng = np.random.default_rng(7)
    S = 150
    runs = []
    while len(runs) < S:
        runs += [int(rng.integers(1, V))] * int(rng.integers(1, 13))
    t1 = np.array(runs[:S])
    rep = int((t1[1:] == t1[:-1]).sum())
    T = S + rep + 3
    tg = np.stack([t1, t1])
    x = rng.standard_normal((2, T, V)).astype(np.float32)
    # Flag 16 on both: a lattice one alignment wide takes the f32 rows out of range in the four-pair form as well (the same
    # words with e2e_debug_segment_band(0)), and the flagged launch redoes those segments; no window failed to fit.  The
    # re-ranking of equal labels on the banded form's own rows is what test_long_runs_of_equal_labels_on_the_fast_path holds.
    keep, flags, _ = run_and_compare(x, tg, np.array([S + rep, T]), np.array([S, S]))
    assert all(f in (0, 16) for f in flags.tolist()), flags
    assert band_misses(keep, 2, T) == 0


def test_long_runs_of_equal_labels_on_the_fast_path():
    """The same targets (runs of up to 12 equal labels, 150 of them) with frames to spare: the banded form's own rows, no flag --
    the window's label slots hold many equal labels and the gradient still equals the oracle's."""
    rng = np.random.default_rng(7)
    S = 150
    runs = []
    while len(runs) < S:
        runs += [int(rng.integers(1, V))] * int(rng.integers(1, 13))
    t1 = np.array(runs[:S])
    T = 2 * S + 37
    x = rng.standard_normal((2, T, V)).astype(np.float32)
    run_and_compare(x, np.stack([t1, t1[::-1].copy()]), np.array([T, T - 30]), np.array([S, S]), want_flags=[0, 0])


def test_a_blank_that_dominates_needs_the_second_stage_of_the_window_rule():
    """An untrained model: the blank carries most of every frame (logits x 0.1 with + 4 on the blank; 200 and 223 labels).  The
    rows are steep, the bound from the group exponents alone gives windows of more than 128 pairs in a quarter of the segments
    (asserted on the CPU), and the kernel's second stage -- the groups' weights cell by cell -- brings every window inside: no
    window that did not fit, hence no flag 8 from the window.  What this regime does set, with the four-pair form over the
    whole lattice just the same (profiles/band/band_misses.txt: 256 of 256 utterances either way), is flag 16: f32 rows of
    some segments leave their range and the flagged launch redoes those segments."""
    T, S = 1000, 223
    rng = np.random.default_rng(1)
    x = (rng.standard_normal((2, T, V)) * 0.1).astype(np.float32)
    x[:, :, 0] += 4.0
    tg = rng.integers(1, V, size=(2, S))
    xl, tl = np.array([T, T]), np.array([200, 223])
    keep, flags, lp = run_and_compare(x, tg, xl, tl)
    for b in range(2):
        la, lq, lz, _ = BW.lattice(lp[b], tg[b, :tl[b]])
        first = BW.rule_windows(la, lq, lz, int(tl[b]), second_stage=False)
        assert sum(1 for w in first if not w[2]) >= 10, "the first stage fits by itself: the case does not reach the second"
        assert all(w[2] for w in BW.rule_windows(la, lq, lz, int(tl[b])))
    assert band_misses(keep, 2, T) == 0
    assert all(f in (0, 16) for f in flags.tolist()), flags


def test_mixed_target_lengths_in_one_call():
    """Targets of 5, 60, 127, 128 and 223 labels and ragged frame counts behind one targets tensor of 223 columns: the banded
    form takes all of them, also the utterances whose whole lattice is narrower than the window."""
    x, tg, xl, tl = random_case(11, 300, 223, (5, 60, 127, 128, 223), xl=(300, 280, 300, 250, 300))
    run_and_compare(x, tg, xl, tl, want_flags=[0] * 5)


def test_flat_emissions_are_the_widest_ordinary_band():
    """logits x 0.1, T = 600, 223 labels: the widest band of the ordinary regimes -- at most 94 pairs down to 2^-60 of Z
    (tools/diag/band_width.py, asserted here for this batch), which the window of 128 holds: no utterance flagged."""
    x, tg, xl, tl = random_case(13, 600, 223, (223, 223, 223, 223), scale=0.1)
    keep, flags, lp = run_and_compare(x, tg, xl, tl, want_flags=[0] * 4)
    for b in range(4):
        r = BW.utterance_numbers(lp[b], tg[b])
        assert r["measured"][-60] <= 94 and r["misses"] == 0, r
    assert band_misses(keep, 4, 600) == 0


def test_a_window_that_cannot_fit_is_redone_in_f64():
    """Emissions that are an even mixture of two alignments of the same 223 labels, one packed into the first frames and one into
    the last: at mid-utterance the posterior spans the whole lattice (checked on the CPU first), no 128 pairs hold it, the
    segment waves set flag 8 and the flagged launch redoes their segments in f64.  AUTO equals the oracle, FAST poisons the
    utterance, and no bounded wait of the flagged launch runs out."""
    T, S = 480, 223
    rng = np.random.default_rng(5)
    tg = np.stack([BW.no_repeat_targets(rng, S, V), rng.integers(1, V, size=S)])
    lp = np.stack([BW.two_alignment_logits(tg[0], T, V), BW.log_softmax(rng.standard_normal((T, V)))]).astype(np.float32)
    r = BW.utterance_numbers(lp[0], tg[0])
    assert r["measured"][-40] > 128 and r["misses"] > 0, r
    xl, tl = np.array([T, T]), np.array([S, S])
    keep, flags, _ = run_and_compare(lp, tg, xl, tl, logprobs=True)
    assert flags[0] & 8 and flags[1] == 0, flags
    assert band_misses(keep, 2, T) >= r["misses"]
    L = _lib.load()
    to, fr = ctypes.c_int(-1), ctypes.c_int(-1)
    assert L.e2e_debug_flagged_counters(keep["workspace"].data_ptr(), 2, T, V, S, ctypes.byref(to), ctypes.byref(fr)) == 0
    assert to.value == 0, "%d bounded waits of the flagged launch ran out" % to.value
    lf, gf = U.c_abi_loss(torch.from_numpy(lp), tg, xl, tl, 0, True, _lib.ALGO_FAST)
    assert np.isnan(lf[0]) and np.isnan(gf[0]).all() and np.isfinite(lf[1]) and np.isfinite(gf[1]).all()


def test_bf16_logits_through_the_banded_form():
    """The 16-bit instance: the T = 200, S = 160 case with bf16 logits, against the oracle on the rounded logits, at the
    tolerance tests/test_gpu_module.py holds 16-bit gradients to (the source dtype's rounding, twice: 4 * 2^-7)."""
    x, tg, xl, tl = random_case(100 + 200 + 160, 200, 160, (160, 131))
    xb = torch.from_numpy(x).to(torch.bfloat16)
    _, l_o, g_o = reference(xb.double().numpy(), tg, xl, tl)
    keep = {}
    la, ga = U.c_abi_loss(xb, tg, xl, tl, 0, False, _lib.ALGO_AUTO, keep=keep)
    assert keep["route"] % 100 // 10 == 4 and keep["route"] // 1000 == 2, "not the fast path's four-pair lattice: %d" % keep["route"]
    flags = fast_flags(keep, 2, 200)
    print("flags", flags.tolist(), "max |dgrad| %.3g" % np.max(np.abs(ga - g_o)))
    assert flags.tolist() == [0, 0]
    eps = 2.0 ** -7
    U.assert_same(la, l_o, LOSS_RTOL, 0.0, "losses")           # (losses stay f32)
    U.assert_same(ga, g_o, 4 * eps, 4 * eps, "grads")
