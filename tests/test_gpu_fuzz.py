"""-m gpu: fixed-seed slices of the randomised sweeps (tools/diag/fuzz_*_vs_oracle.py, fuzz_align.py) in the driver-run suite.

Every case is compared with the ORACLE (oracle/ctc_oracle.c through tests/oracle_lib.py), never with another HIP kernel.
Round 5's three latent bugs (an f64 segment redo that wrote NaN rows and reported success, a call that failed for 73..96
columns with more than 255 labels, a wave vote inside `if (lane == 0)`) were all found by these generators while the suite,
which only had hand-picked shapes, stayed green for two rounds -- hence this file.

Families (cases; what they drive):
  ext      300 f32 + 70 bf16 + 70 f16   E2E_ALGO_AUTO on emissions that leave the f32 lattice: the f64 segment redo, the
                                        extended-range redo (ctc_ext.h), the hand-over to the exact kernel
  scaled   144 (+ 48 wide alphabets)    the exact kernel's scaled form: blank-valued targets, targets beyond 447 labels,
                                        -inf log-probs, infeasible alignments
  exact    120                          E2E_ALGO_EXACT, f32 and f64, log domain
  fastauto 120                          unit-noise / trained-model emissions: the fast path proper (AUTO), ragged, any blank
  align    60                           e2e_ctc_align, bit-exact
  noblank  98 (f32 + f64, x 2 widths)   CTC without blank against tests/noblank_ref.py: every LDS block size K = 16..1
  gram     98 (f32 + f64, x 2 widths)   Gram-CTC against tests/gram_ref.py: every (max_order, K) of orders 1..8
  callshape 393 random + 156 sweep     cases of the ext (120 f32 + 40 bf16 + 40 f16 drawn), fastauto (120), scaled (60) and exact (40)
            + 7 flag-route batches     generators under a randomised CALL SHAPE: targets padded into another dispatch band with garbage
                                        beyond t_len, tgt_stride beyond the width, strided logits, grad_scale, fused reduction; asserts
                                        the routes (e2e_debug_loss_route) and flag routes it reached.  16-bit cases that the engine
                                        would up-cast are counted as callshape_upcast.  The align family runs each case a second
                                        time with padded targets.
(noblank and gram compare with the f64 test-side references, not the oracle: each case runs with targets exactly max(t_len)
wide and padded wider with garbage, and both runs must match; the tests assert the block sizes and redo reasons they reach.)
The beam search's slice of the same kind lives in tests/test_gpu_beam.py::test_fuzz_slice_equals_the_oracle_or_is_a_proven_tie
(220 cases, run through both kernels).  The counts are printed in pytest's summary (tests/conftest.py).
"""
import ctypes
import threading

import numpy as np
import pytest
import torch

import gram_ref as GR
import noblank_ref as NR
import oracle_lib as O
import gpu_util as U
from end2end_amd import _lib
from test_gpu_align import c_abi_align
from test_gpu_gram import gc_block
from test_gpu_noblank import nb_block

pytestmark = pytest.mark.gpu

COUNTS = {}          # family -> [cases, utterances]; reported by conftest.pytest_terminal_summary


def _count(family, utterances):
    c = COUNTS.setdefault(family, [0, 0])
    c[0] += 1
    c[1] += utterances


def _feasible(tg, tl, xl):
    """shorten targets until every utterance has an alignment (the infeasible ones belong to the scaled / exact families)"""
    for b in range(len(tl)):
        need = lambda n: n + int((tg[b, 1:n] == tg[b, :n - 1]).sum())
        while need(int(tl[b])) > xl[b]:
            tl[b] = max(1, tl[b] // 2)


# ---------------------------------------------------------------------------------------------------------------------
# ext: tools/diag/fuzz_ext_vs_oracle.py
# ---------------------------------------------------------------------------------------------------------------------
def _ext_case(rng):
    B = int(rng.integers(1, 7))
    V = int(rng.choice([3, 5, 29, 29, 48, 80, 96, 97, 150, 224, 300, 448]))
    T = int(rng.choice([2, 9, 17, 64, 200, 500, 1000, 1000, 2100]))
    Smax = int(rng.integers(1, min(447, max(1, T // 2)) + 1))
    blank = int(rng.integers(0, V)) if rng.random() < 0.3 else 0
    mode = str(rng.choice(["sharp", "sharp", "peaky_noise", "neginf"]))
    labels = [v for v in range(V) if v != blank]
    tg = rng.choice(labels, size=(B, Smax))
    tl = rng.integers(1, Smax + 1, size=B)
    tl[0] = Smax
    xl = rng.integers(max(2, T // 2), T + 1, size=B)
    xl[0] = T
    _feasible(tg, tl, xl)
    logprobs = False
    if mode == "sharp":
        x = rng.standard_normal((B, T, V)) * float(rng.choice([3.0, 8.0, 12.0]))
    elif mode == "peaky_noise":
        x = rng.standard_normal((B, T, V))
        for b in range(B):
            src = (b + 1) % B if rng.random() < 0.5 else b        # half of the utterances emit ANOTHER one's transcript
            n2 = min(int(tl[src]), int(xl[b]))
            slots = np.sort(rng.choice(int(xl[b]), size=n2, replace=False))
            path = np.full(int(xl[b]), blank)
            path[slots] = tg[src, :n2]
            x[b, np.arange(int(xl[b])), path] += float(rng.choice([6.0, 10.0, 14.0]))
    else:
        x = rng.standard_normal((B, T, V)) * 8.0
        x[rng.random((B, T, V)) < 0.05] = -np.inf
        x[:, :, blank] = np.where(np.isinf(x[:, :, blank]), 0.0, x[:, :, blank])     # (the blank stays possible: a finite loss)
        logprobs = True
    return dict(x=x, tg=tg, xl=xl, tl=tl, blank=blank, logprobs=logprobs, mode=mode)


def _run_ext(c, io16):
    """-> None (equal), "marginal" (single elements within 1e-5: the f32 subtraction in the softmax at |x - max| up to 80,
    DESIGN 4.2a) or the assertion's text"""
    g_rtol, g_atol = (1e-4, 2e-6) if io16 is None else ((2.0 ** -7, 2.0 ** -8) if io16 == torch.bfloat16 else (2.0 ** -10, 2.0 ** -11))
    xt = torch.from_numpy(c["x"])
    tg, xl, tl, blank = c["tg"], c["xl"], c["tl"], c["blank"]
    if c["logprobs"]:
        arg = torch.log_softmax(xt, -1).float()
        l_o, g_o = O.ctc_loss(arg.double().numpy(), tg, xl, tl, blank)       # (the oracle on what the call is given: ROUNDED log-probs)
    else:
        arg = xt.float() if io16 is None else xt.to(io16)
        l_o, g_o = O.ctc_loss(torch.log_softmax(arg.double(), -1).numpy(), tg, xl, tl, blank)
        for b in range(len(xl)):
            g_o[b, xl[b]:] = 0.0
    la, ga = U.c_abi_loss(arg, tg, xl, tl, blank, c["logprobs"], _lib.ALGO_AUTO)
    try:
        U.assert_same(la, l_o, 1e-4, 2e-5, "losses")
        U.assert_same(ga, g_o, g_rtol, g_atol, "grads")
        return None
    except AssertionError as e:
        try:
            U.assert_same(la, l_o, 1e-4, 2e-5, "losses")
            U.assert_same(ga, g_o, g_rtol, max(1e-5, 2 * g_atol), "grads")
            return "marginal"
        except AssertionError:
            return str(e).strip().splitlines()[:6]


@pytest.mark.parametrize("seed,n,dtype", [(0, 150, None), (1, 150, None), (2, 70, torch.bfloat16), (3, 70, torch.float16)],
                         ids=["f32_seed0", "f32_seed1", "bf16_seed2", "f16_seed3"])
def test_ext_family_against_the_oracle(seed, n, dtype):
    rng = np.random.default_rng(seed)
    bad, marginal, done = [], [], 0
    for case in range(n):
        c = _ext_case(rng)
        if c["logprobs"] and dtype is not None:
            continue                                             # (16-bit log-probabilities cannot hold these: logits only)
        r = _run_ext(c, dtype)
        done += 1
        _count("ext", len(c["xl"]))
        if r == "marginal":
            marginal.append(case)
        elif r is not None:
            bad.append((case, c["mode"], c["x"].shape, int(c["tg"].shape[1]), c["blank"], r))
    assert not bad, "mismatching cases of seed %d: %s" % (seed, bad)
    assert len(marginal) <= max(1, done // 50), "marginal cases (one element within 1e-5) of seed %d: %s" % (seed, marginal)


# ---------------------------------------------------------------------------------------------------------------------
# scaled / exact: tools/diag/fuzz_scaled_vs_oracle.py, fuzz_exact_vs_oracle.py
# ---------------------------------------------------------------------------------------------------------------------
def _small_case(rng, case, family, wide):
    long_targets = family == "scaled" and case % 12 == 11
    if family == "scaled":
        B = int(rng.integers(1, 5))
        if long_targets:
            T = int(rng.integers(450, 700)); V = int(rng.choice([3, 29, 64])); Smax = int(rng.integers(448, min(T + 2, 600) + 1))
        else:
            T = int(rng.integers(1, 200)); V = int(rng.choice([2, 3, 5, 29, 64, 96, 200, 1500] if wide else [2, 3, 5, 29, 64, 96]))
            Smax = int(rng.integers(1, min(120, T + 3) + 1))
        f64 = False
        scale = float(rng.choice([0.3, 1.0, 4.0, 8.0, 12.0]))
    else:
        B = int(rng.integers(1, 6)); T = int(rng.integers(1, 90)); V = int(rng.choice([2, 3, 5, 29, 64, 97, 300]))
        Smax = int(rng.integers(0, min(60, T + 3) + 1))
        f64 = bool(rng.integers(0, 2))
        scale = float(rng.choice([0.3, 1.0, 4.0]))
    fused = bool(rng.integers(0, 2))
    blank = int(rng.choice([0, V - 1, rng.integers(0, V)]))
    g = torch.Generator().manual_seed(int(rng.integers(1 << 30)))
    x = torch.randn(B, T, V, generator=g, dtype=torch.float64) * scale
    lp = torch.log_softmax(x, -1)
    if not fused and rng.integers(0, 3) == 0:
        lp[:, ::4, int(rng.integers(0, V))] = float("-inf")
    labs = [v for v in range(V) if v != blank]
    tg = torch.tensor(rng.choice(labs, size=(B, max(Smax, 1))), dtype=torch.long)
    xl = torch.tensor(rng.integers(1, T + 1, size=B)); xl[0] = T
    tl = torch.tensor(rng.integers(0, Smax + 1, size=B)); tl[0] = Smax
    if family == "scaled" and not long_targets:
        for b in range(B):
            if tl[b] > 0:
                tg[b, int(rng.integers(0, int(tl[b])))] = blank          # a target equal to the blank id: handed over by the fast path
    inp = (x if fused else lp).to(torch.float64 if f64 else torch.float32)
    return dict(inp=inp, fused=fused, tg=tg, xl=xl, tl=tl, blank=blank, f64=f64, shape=(B, T, V, Smax))


def _run_small(c, algo):
    ref_lp = torch.log_softmax(c["inp"].double(), -1) if c["fused"] else c["inp"].double()
    l_o, g_o = O.ctc_loss(ref_lp.numpy(), c["tg"].numpy(), c["xl"].numpy(), c["tl"].numpy(), c["blank"])
    if c["fused"]:
        for b in range(len(l_o)):
            if np.isfinite(l_o[b]):
                g_o[b, int(c["xl"][b]):] = 0.0          # (an infeasible utterance stays NaN everywhere, quirk Q2)
    lg, gg = U.c_abi_loss(c["inp"], c["tg"], c["xl"], c["tl"], c["blank"], not c["fused"], algo)
    rt, at = (1e-9, 1e-12) if c["f64"] else (1e-4, 2e-6)
    try:
        U.assert_same(lg, l_o, rt, at, "losses")
        U.assert_same(gg, g_o, rt, at, "grads")
        return None
    except AssertionError as e:
        return str(e).strip().splitlines()[:4]


@pytest.mark.parametrize("family,seed,n,wide", [("scaled", 0, 144, False), ("scaled", 5, 48, True), ("exact", 0, 120, False)],
                         ids=["scaled_seed0", "scaled_wide_seed5", "exact_seed0"])
def test_scaled_and_exact_families_against_the_oracle(family, seed, n, wide):
    rng = np.random.default_rng(seed)
    bad = []
    for case in range(n):
        c = _small_case(rng, case, family, wide)
        r = _run_small(c, _lib.ALGO_AUTO if family == "scaled" else _lib.ALGO_EXACT)
        _count(family, c["shape"][0])
        if r is not None:
            bad.append((case, c["shape"], c["fused"], c["blank"], c["f64"], r))
    assert not bad, "mismatching cases: %s" % bad


# ---------------------------------------------------------------------------------------------------------------------
# fastauto: what the fast path keeps (unit noise, a trained model's emissions), every lattice width, 32-bit and 16-bit I/O
# ---------------------------------------------------------------------------------------------------------------------
def _fast_case(rng):
    B = int(rng.integers(1, 9))
    V = int(rng.choice([2, 5, 29, 29, 32, 33, 64, 96, 120, 224, 448, 1000, 1001, 8000]))     # (1001: the wide path's two-pass rows, 16-bit too)
    T = int(rng.choice([1, 3, 15, 16, 17, 33, 100, 256, 511, 1000]))
    Smax = int(rng.integers(1, min(447, max(1, (T + 1) // 2)) + 1))
    if V >= 1000:
        Smax = min(Smax, 120)
    blank = int(rng.integers(0, V)) if rng.random() < 0.3 else 0
    labels = [v for v in range(V) if v != blank]
    tg = rng.choice(labels, size=(B, Smax))
    if rng.random() < 0.3 and Smax > 1:
        tg[:, 1::2] = tg[:, 0::2][:, :tg[:, 1::2].shape[1]]                     # adjacent repeats
    tl = rng.integers(1, Smax + 1, size=B); tl[0] = Smax
    xl = rng.integers(max(1, T // 2), T + 1, size=B); xl[0] = T
    _feasible(tg, tl, xl)
    x = rng.standard_normal((B, T, V)) * float(rng.choice([0.1, 1.0, 1.0, 2.0]))
    if rng.random() < 0.4:
        for b in range(B):                                                       # a trained model: the own transcript boosted
            n = min(int(tl[b]), int(xl[b]))
            slots = np.sort(rng.choice(int(xl[b]), size=n, replace=False))
            x[b, slots, tg[b, :n]] += float(rng.choice([4.0, 8.0]))
    logprobs = bool(rng.random() < 0.3)
    time_major = bool(rng.random() < 0.3)
    return dict(x=x, tg=tg, xl=xl, tl=tl, blank=blank, logprobs=logprobs, time_major=time_major)


@pytest.mark.parametrize("seed,n", [(10, 60), (11, 60)], ids=["seed10", "seed11"])
def test_fast_path_family_against_the_oracle(seed, n):
    rng = np.random.default_rng(seed)
    bad = []
    for case in range(n):
        c = _fast_case(rng)
        xt = torch.from_numpy(c["x"])
        io16 = [None, None, torch.bfloat16, torch.float16][case % 4]
        if c["logprobs"]:
            io16 = None
        arg = xt.float() if io16 is None else xt.to(io16)
        lp = torch.log_softmax(arg.double(), -1)
        if c["logprobs"]:
            arg = lp.float(); lp = arg.double()
        l_o, g_o = O.ctc_loss(lp.numpy(), c["tg"], c["xl"], c["tl"], c["blank"])
        if not c["logprobs"]:
            for b in range(len(c["xl"])):
                g_o[b, c["xl"][b]:] = 0.0
        if c["time_major"]:
            arg = arg.permute(1, 0, 2).contiguous().permute(1, 0, 2)            # a time-major view, no copy
        la, ga = U.c_abi_loss(arg, c["tg"], c["xl"], c["tl"], c["blank"], c["logprobs"], _lib.ALGO_AUTO)
        g_rtol, g_atol = (1e-4, 2e-6) if io16 is None else ((2.0 ** -7, 2.0 ** -8) if io16 == torch.bfloat16 else (2.0 ** -10, 2.0 ** -11))
        _count("fastauto", len(c["xl"]))
        try:
            U.assert_same(la, l_o, 1e-4, 2e-5, "losses")
            U.assert_same(ga, g_o, g_rtol, g_atol, "grads")
        except AssertionError as e:
            bad.append((case, c["x"].shape, int(c["tg"].shape[1]), c["blank"], str(io16), c["logprobs"], str(e).strip().splitlines()[:4]))
    assert not bad, "mismatching cases: %s" % bad


# ---------------------------------------------------------------------------------------------------------------------
# align: tools/diag/fuzz_align.py (bit-exact)
# ---------------------------------------------------------------------------------------------------------------------
def test_align_family_is_bit_exact_against_the_oracle():
    rng = np.random.default_rng(0)
    rp = np.random.default_rng(100)                      # the padded second run's draws
    bad = []
    for case in range(60):
        B = int(rng.integers(1, 6)); T = int(rng.integers(1, 300)); V = int(rng.integers(2, 40))
        S = int(rng.integers(0, min(T, 120) + 1))
        is_ctc = bool(rng.integers(0, 2))
        blank = int(rng.choice([0, V - 1, rng.integers(0, V)])) if is_ctc else 0
        g = torch.Generator().manual_seed(int(rng.integers(1 << 30)))
        x = torch.randn(B, T, V, generator=g, dtype=torch.float64) * float(rng.choice([0.0, 0.3, 1.0, 4.0]))
        style = int(rng.integers(0, 3))
        if style == 1:
            x = x.round()
        lp = torch.log_softmax(x, -1)
        if style == 2 and V > 2:
            lp[:, ::3, int(rng.integers(0, V))] = float("-inf")
        pool = [v for v in range(V) if v != blank] if is_ctc else list(range(V))
        tg = torch.tensor(rng.choice(pool, size=(B, max(S, 1))))
        if rng.integers(0, 2) and S > 1:
            tg[:, 1::2] = tg[:, 0::2][:, : tg[:, 1::2].shape[1]]
        tl = rng.integers(0 if is_ctc else 1, S + 1, size=B) if S > 0 else np.zeros(B, dtype=np.int64)
        if not is_ctc:
            tl = np.maximum(tl, 1)
        xl = rng.integers(1, T + 1, size=B); xl[0] = T
        if not is_ctc:
            xl = np.maximum(xl, np.minimum(tl, T))
        if rng.integers(0, 2):
            lp = lp.float()
        got = c_abi_align(lp, tg, xl, tl, blank, is_ctc)
        want = O.ctc_align(lp.double().numpy(), tg.numpy(), xl, tl, blank, is_ctc)
        _count("align", B)
        if not np.array_equal(got, want):
            bad.append((case, dict(B=B, T=T, V=V, S=S, is_ctc=is_ctc, blank=blank, style=style)))
        # the same call with the targets padded wider with garbage beyond t_len and handed over as a column slice of a wider
        # buffer (tgt_stride > width): the same labelling (the draws come from a generator of their own)
        fill = [[-1, V, blank, int(pool[0]), 1 << 40, -(1 << 63)][int(rp.integers(0, 6))] for _ in range(B)]
        width = tg.shape[1] + int(rp.integers(1, 200))
        wide = U.padded_targets(tg.numpy(), tl, width, fill, width + int(rp.integers(1, 41)))
        got = c_abi_align(lp, wide, xl, tl, blank, is_ctc)
        if not np.array_equal(got, want):
            bad.append((case, "padded to %d with %s" % (width, sorted(set(fill))), dict(B=B, T=T, V=V, S=S, is_ctc=is_ctc, blank=blank, style=style)))
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------
# Round 5's regressions as named cases (the other two: test_gpu_regimes.py::test_probabilities_at_the_end_of_f32_...,
# test_gpu_loss.py::test_long_transcripts_take_the_fast_path[B2_T1000_V96_S425 / B2_T900_V80_S300])
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,S,T", [(29, 200, 1000), (29, 100, 2100), (48, 223, 1000)], ids=lambda v: str(v))
def test_no_redo_reports_success_over_nan_rows(V, S, T):
    """Sharp unrelated emissions at scale 12: row sums of the f64 segment redo sit near the end of f64, where the reciprocal of
    its Newton step overflowed -- NaN rows were written and the redo reported success (rounds 3..5).  Whatever route an
    utterance takes, a finite oracle loss means a finite gradient slab, equal to the oracle's."""
    rng = np.random.default_rng(V + S)
    B = 4
    x = (rng.standard_normal((B, T, V)) * 12.0).astype(np.float32)
    tg = rng.integers(1, V, size=(B, S)); tl = rng.integers(S // 2, S + 1, size=B); tl[0] = S
    xl = np.array([T, T - 7, T // 2 + 3, T])
    lp = torch.log_softmax(torch.from_numpy(x).double(), -1).numpy()
    l_o, g_o = O.ctc_loss(lp, tg, xl, tl, 0)
    for b in range(B):
        g_o[b, xl[b]:] = 0.0
    la, ga = U.c_abi_loss(torch.from_numpy(x), tg, xl, tl, 0, False, _lib.ALGO_AUTO)
    assert np.isfinite(l_o).all() and np.isfinite(la).all() and np.isfinite(ga).all()
    U.assert_same(la, l_o, 1e-4, 2e-5, "losses")
    U.assert_same(ga, g_o, 1e-4, 1e-5, "grads")          # (scale 12: single elements up to 7e-6)


# ---------------------------------------------------------------------------------------------------------------------
# The flagged launch's bounded waits under contention
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lds", [0, 120 * 1024], ids=["issue_slots_only", "lds_taken"])
def test_flagged_batch_is_right_while_another_stream_holds_the_cus(lds):
    """The flagged launch is a multi-round protocol between the workgroups of ONE launch with bounded waits; the regime tests
    assert that no wait runs out on an idle GPU.  Here a second stream keeps the chip busy with long-running workgroups
    (`e2e_debug_occupy` from the same library: 224 workgroups of 1024 threads resident for 3 ms each, launched back to back;
    with 120 KB of LDS each no workgroup of the flagged launch fits beside one, so part of its grid is NOT resident while the
    rest waits) while a batch with mislabelled utterances, range-flagged utterances and a blank-valued target runs.  The
    results must equal the oracle's WHATEVER the counters say -- a wait that runs out has to end in the slow route, not in a
    wrong or unsettled row."""
    L = _lib.load()
    if not hasattr(L, "e2e_debug_occupy"):
        pytest.skip("library without e2e_debug_occupy")
    d = U.dev()
    from test_gpu_regimes import aligned
    rng = np.random.default_rng(77)
    x, tg, xl, tl = aligned(rng, 12, 1000, 29, 200, 10.0, short=[(5, 933)])
    tg[1], tl[1] = tg[2].copy(), tl[2]                          # mislabelled: extended-range chains
    tg[5], tl[5] = tg[6].copy(), tl[6]
    x[7] = rng.standard_normal(x[7].shape) * 3.0                # sharp unrelated at scale 3: range flags, f64 segment redo
    x[8] = rng.standard_normal(x[8].shape) * 3.0
    tg[9, 3] = 0                                                # a target equal to the blank: full recomputation (step 2)
    lp = torch.log_softmax(torch.from_numpy(x).double(), -1).numpy()
    l_o, g_o = O.ctc_loss(lp, tg, xl, tl, 0)
    for b in range(len(xl)):
        g_o[b, xl[b]:] = 0.0
    side = torch.cuda.Stream(device=d)
    stop = threading.Event()

    def hog():
        torch.cuda.set_device(d)
        while not stop.is_set():
            for _ in range(4):
                _lib.check(L.e2e_debug_occupy(224, 1024, lds, 3_000_000, ctypes.c_void_p(side.cuda_stream)))
            side.synchronize()

    th = threading.Thread(target=hog)
    th.start()
    try:
        outcomes = []
        for rep in range(6):
            keep = {}
            la, ga = U.c_abi_loss(torch.from_numpy(x), tg, xl, tl, 0, False, _lib.ALGO_AUTO, keep=keep)
            U.assert_same(la, l_o, 1e-4, 2e-5, "losses (rep %d)" % rep)
            U.assert_same(ga, g_o, 1e-4, 2e-6, "grads (rep %d)" % rep)
            to, fr = ctypes.c_int(-1), ctypes.c_int(-1)
            L.e2e_debug_flagged_counters(keep["workspace"].data_ptr(), 12, 1000, 29, 200, ctypes.byref(to), ctypes.byref(fr))
            outcomes.append((to.value, fr.value))
    finally:
        stop.set()
        th.join()
    torch.cuda.synchronize()
    print("flagged launch under contention: (waits that ran out, failed redos) per repetition:", outcomes)


@pytest.mark.parametrize("shape", [(300, 70, 66, 24), (520, 40, 90, 12)], ids=lambda s: "B%d_T%d_V%d_S%d" % s)
def test_batches_beyond_the_cu_count_take_the_shallow_probability_ring(shape):
    """More utterances than the chip has CUs on an alphabet whose f64 probability ring of eight blocks keeps a second workgroup off
    the CU (61..96 columns): the single-wave chain kernel then runs with a ring of four (round 6; BASELINE configs[4]'s compact
    lattice is the case that matters).  Ragged lengths, repeats, against the oracle."""
    B, T, V, S = shape
    rng = np.random.default_rng(B)
    x = rng.standard_normal((B, T, V)).astype(np.float32)
    tg = rng.integers(1, V, size=(B, S))
    tg[:, 1::3] = tg[:, 0::3][:, :tg[:, 1::3].shape[1]]
    tl = rng.integers(1, S + 1, size=B); tl[0] = S
    xl = rng.integers(2 * S + 2, T + 1, size=B); xl[0] = T
    lp = torch.log_softmax(torch.from_numpy(x).double(), -1).numpy()
    l_o, g_o = O.ctc_loss(lp, tg, xl, tl, 0)
    for b in range(B):
        g_o[b, xl[b]:] = 0.0
    la, ga = U.c_abi_loss(torch.from_numpy(x), tg, xl, tl, 0, False, _lib.ALGO_AUTO)
    U.assert_same(la, l_o, 1e-4, 2e-5, "losses")
    U.assert_same(ga, g_o, 1e-4, 2e-6, "grads")
    lf, _ = U.c_abi_loss(torch.from_numpy(x), tg, xl, tl, 0, False, _lib.ALGO_FAST)
    assert not np.isnan(lf).any(), "the fast path gave up on %s" % np.nonzero(np.isnan(lf))[0].tolist()


# ---------------------------------------------------------------------------------------------------------------------
# noblank / gram: CTC without blank (ctc_loss_noblank.hip) and Gram-CTC (ctc_loss_gram.hip) against the f64 test-side
# references on exactly the log-probabilities the kernel sees.  The padded target width picks the LDS block K and the row
# layout, so every case runs twice: targets exactly max(t_len) wide, then wider (within capacity) with garbage beyond t_len.
# ---------------------------------------------------------------------------------------------------------------------
DEV = torch.device("cuda", 0)


def _bands(block, last):
    """{K: (first, last width)} of a block-size function over the widths 0..last"""
    out = {}
    for s in range(last + 1):
        k = block(s)
        out[k] = (out.get(k, (s, s))[0], s)
    return out


NB_LAST = 1855                                       # the longest target the no-blank kernel serves
NB_BANDS = _bands(nb_block, NB_LAST)
GC_LAST = {M: max(s for s in range(1400) if gc_block(s, M)) for M in range(1, 9)}
GC_BANDS = {M: _bands(lambda s: gc_block(s, M), GC_LAST[M]) for M in range(1, 9)}
GC_PAIRS = sorted((M, K) for M in GC_BANDS for K in GC_BANDS[M])


def _wider(bands, W, rng):
    """a padded width beyond W, in a random block-size band that has one"""
    ks = sorted(k for k, (lo, hi) in bands.items() if hi > W)
    lo, hi = bands[int(rng.choice(ks))]
    return int(rng.integers(max(lo, W + 1), hi + 1))


def _lengths(rng, need, K, T):
    """x_len >= need: exactly need, ending on the first or the last frame of a block, anywhere; one frame short (infeasible)
    now and then"""
    kind = int(rng.integers(0, 6))
    if kind == 5 and need >= 2:
        return min(need - 1, T)
    x = [need, -(-(need - 1) // K) * K + 1, -(-need // K) * K, int(rng.integers(need, max(need, T) + 1))][min(kind, 3)]
    return min(max(x, need), T)


def _on_gpu(x, view):
    """x (B, T, V) on the GPU as it is, as a time-major view (a permuted copy) or column-strided (sV = 2)"""
    if view == "time_major":
        return x.permute(1, 0, 2).contiguous().to(DEV).permute(1, 0, 2)
    if view == "strided":
        w = torch.zeros(x.shape[0], x.shape[1], 2 * x.shape[2], dtype=x.dtype, device=DEV)
        w[:, :, ::2] = x.to(DEV)
        return w[:, :, ::2]
    return x.to(DEV)


def _padded(tg, tl, width, V, rng):
    """targets `width` wide: row b holds tg[b, :tl[b]], then garbage (-1, V or 2**40)"""
    out = np.empty((len(tl), width), dtype=np.int64)
    for b in range(len(tl)):
        out[b] = [-1, V, 1 << 40][int(rng.integers(0, 3))]
        out[b, :tl[b]] = tg[b, :tl[b]]
    return torch.from_numpy(out)


def _differs(got_l, got_g, want_l, want_g, tol):
    """None, or what differs: the inf/NaN pattern exactly, losses within tol * max(1, |want|), gradients within tol"""
    inf = np.isinf(want_l)
    if not (np.array_equal(np.isinf(got_l), inf) and np.array_equal(np.isnan(got_l), np.isnan(want_l))
            and np.array_equal(got_l[inf], want_l[inf])):
        return "losses %s, want %s" % (got_l.tolist(), want_l.tolist())
    fin = np.isfinite(want_l)
    dl = np.abs(got_l[fin] - want_l[fin]) / np.maximum(1.0, np.abs(want_l[fin]))
    if (dl > tol).any():
        return "losses off by %.3g (relative) at %s" % (dl.max(), np.flatnonzero(fin)[dl > tol].tolist())
    if not np.array_equal(np.isnan(got_g), np.isnan(want_g)):
        return "NaN pattern of the gradient, utterances %s" % sorted(set(np.nonzero(np.isnan(got_g) != np.isnan(want_g))[0].tolist()))
    ok = ~np.isnan(want_g)
    dg = np.max(np.abs(got_g[ok] - want_g[ok]), initial=0.0)
    return None if dg <= tol else "gradient off by %.3g" % dg


def _run_twice(family, c, eng, want_l, want_g, rng, block, reached, reasons):
    """c's call at its exact and its padded width -> [(run, width, what differs)]; adds the block sizes reached and, for f32,
    the redo reasons reported.  The backward must not redo an f32 'plain' utterance (unit-scale noise): its mass check fails
    only when the forward's rows lost cells that carry paths.  (The forward may redo one: with a long target and few spare
    frames the end cells fall 2**-1074 below their row's largest, and the probability-domain total is 0.)"""
    bad = []
    tol = 1e-9 if c["x"].dtype == torch.float64 else 1e-5
    xl, tl = torch.from_numpy(c["xl"]).to(DEV), torch.from_numpy(c["tl"]).to(DEV)
    for run, width in (("exact", int(c["tl"].max())), ("padded", c["pad"])):
        out = eng.compute(_on_gpu(c["x"], c["view"]), _padded(c["tg"], c["tl"], width, c["V"], rng).to(DEV), xl, tl,
                          input_is_logprobs=c["logprobs"], grad_scale=c["scale"], reduction=c["reduction"])
        flags = eng.redo_flags() if c["x"].dtype == torch.float32 else None
        reached.add(block(width))
        r = _differs(out[0].cpu().double().numpy(), out[1].cpu().double().numpy(), want_l, want_g * c["scale"], tol)
        if r is None and c["reduction"]:
            want = want_l.sum() if c["reduction"] == "sum" else want_l.mean()
            got = float(out[2].item())
            if not (got == want or (np.isnan(got) and np.isnan(want)) or
                    (np.isfinite(want) and abs(got - want) <= tol * max(1.0, abs(want)))):
                r = "reduced (%s) %r, want %r" % (c["reduction"], got, want)
        if r is None and flags is not None:
            reasons.update(flags.tolist())
            if not set(flags.tolist()) <= {0, 1, 2}:
                r = "redo flags %s" % flags.tolist()
            elif c["mode"] == "plain" and (flags == 2).any():
                r = "the backward redid unit-noise utterances: flags %s" % flags.tolist()
        if r is not None:
            bad.append((run, width, r))
    _count(family, len(c["tl"]))
    return bad


def _common(rng, c, B):
    c["view"] = str(rng.choice(["contiguous", "contiguous", "time_major", "strided"]))
    c["scale"] = float(rng.choice([1.0, 0.37, 1.0 / B]))
    c["reduction"] = [None, "sum", "mean"][int(rng.integers(0, 3))]
    return c


def _inputs(rng, B, T, V, mode, dtype):
    """(x as the call gets it, logprobs): 'plain' unit-scale noise, 'sharp' logits at scale 8-20, 'low' log-probabilities
    below -700 (logits at scale 150-250, or log-probabilities given so)"""
    logprobs = False
    if mode == "sharp":
        x = torch.from_numpy(rng.standard_normal((B, T, V)) * float(rng.choice([8.0, 12.0, 16.0, 20.0])))
    elif mode == "low" and rng.random() < 0.5:
        x = torch.from_numpy(rng.standard_normal((B, T, V)) * float(rng.integers(150, 251)))
    else:
        x = torch.from_numpy(rng.standard_normal((B, T, V)) * float(rng.choice([0.5, 1.0, 2.0, 3.0])))
        logprobs = mode == "low" or rng.random() < 0.4
        if logprobs:
            x = torch.log_softmax(x, -1)
            if mode == "low":
                x[rng.random((B, T, V)) < 0.05] = -750.0 - 100.0 * float(rng.random())
    return x.to(dtype), logprobs


# ---- noblank ----
NB_V = [1, 2, 3, 5, 29, 29, 64, 300, 2000, 32000]


def _nb_case(rng, case, dtype, big=False):
    """The exact width in the band of K = 16 - case % 16 (case % 16 == 0: sharp logits, == 8: log-probabilities below -700)"""
    K = 16 - case % 16
    mode = "plain" if big else {0: "sharp", 8: "low"}.get(case % 16, "plain")
    lo, hi = NB_BANDS[K]
    if big:                                          # more utterances than the 256 CUs
        B, W, T = 300, int(rng.integers(0, 21)), int(rng.integers(20, 61))
    elif mode == "sharp":
        B, W, T = int(rng.integers(4, 7)), int(rng.integers(20, 41)), int(rng.integers(300, 601))
    else:
        W = int(rng.integers(lo, min(hi, NB_LAST - 1) + 1)) if K < 16 or rng.random() < 0.5 else int(rng.integers(0, 49))
        B = int(rng.integers(1, 7 if W < 300 else 3))
        T = max(W, 1) + int(rng.choice([0, 0, 1, K - 1, K, K + 1, int(rng.integers(0, 3 * K + 1))]))
    V = 29 if mode == "sharp" or big else int(rng.choice([v for v in NB_V if B * T * v <= 4_000_000]))
    sp = int(rng.choice(sorted({-1, 0, V - 1, V // 2})))
    style = str(rng.choice(["random", "runs", "distinct", "space"]))
    if style == "runs":                              # long runs of one label
        tg = np.repeat(rng.integers(0, V, size=(B, W + 1)), int(rng.integers(4, 61)), axis=1)[:, :W]
    elif style == "distinct":                        # all-distinct labels (distinct within every V of them)
        tg = np.stack([np.tile(rng.permutation(V), W // V + 1)[:W] for _ in range(B)]) if W else np.zeros((B, 0), np.int64)
    else:
        tg = rng.integers(0, V, size=(B, W))
        if style == "space" and sp >= 0:
            tg[rng.random((B, W)) < 0.2] = sp
    tl = rng.integers(0, W + 1, size=B)
    tl[0] = W
    if B > 1 and rng.random() < 0.4:                 # the target [sp] (Q10's neighbour) or the empty target
        tl[1] = 1 if sp >= 0 and W >= 1 else 0
        if W >= 1:
            tg[1, 0] = sp if sp >= 0 else tg[1, 0]
    xl = np.array([T] + [_lengths(rng, max(int(tl[b]), 1), K, T) for b in range(1, B)], dtype=np.int64)
    if mode == "sharp":
        xl[1:] = rng.integers(80, T + 1, size=B - 1)
    x, logprobs = _inputs(rng, B, T, V, mode, dtype)
    c = dict(x=x, logprobs=logprobs, tg=tg.astype(np.int64), tl=tl.astype(np.int64), xl=xl, V=V, sp=sp, mode=mode,
             pad=_wider(NB_BANDS, W, rng))
    return _common(rng, c, B)


def _nb_want(c):
    lp = (c["x"].double() if c["logprobs"] else torch.log_softmax(c["x"].double(), -1)).numpy()
    B, T, V = lp.shape
    want_l, want_g = np.zeros(B), np.zeros((B, T, V))
    for b in range(B):
        n, s = int(c["xl"][b]), int(c["tl"][b])
        want_l[b], want_g[b, :n] = NR.utterance(lp[b, :n], c["tg"][b, :s], c["sp"])
    return want_l, want_g


@pytest.mark.parametrize("dtype,seed,n", [(torch.float32, 20, 48), (torch.float64, 21, 48)], ids=["f32_seed20", "f64_seed21"])
def test_noblank_family_against_the_f64_restatement(dtype, seed, n):
    from end2end_amd.engines import CTCWithoutBlankLossEngine
    rng = np.random.default_rng(seed)
    bad, reached, reasons = [], set(), set()
    for case in range(n + 1):
        c = _nb_case(rng, case, dtype, big=case == n)
        want_l, want_g = _nb_want(c)
        r = _run_twice("noblank", c, CTCWithoutBlankLossEngine(c["sp"]), want_l, want_g, rng, nb_block, reached, reasons)
        if r:
            bad.append((case, c["mode"], tuple(c["x"].shape), int(c["tl"].max()), c["pad"], c["sp"], c["view"],
                        c["logprobs"], r))
    assert not bad, "mismatching cases of seed %d: %s" % (seed, bad)
    assert reached == set(range(1, 17)), "block sizes not reached: %s" % sorted(set(range(1, 17)) - reached)
    if dtype == torch.float32:
        assert {1, 2} <= reasons, "redo reasons reported: %s" % sorted(reasons)


# ---- gram ----
GC_MODES = {(2, 16): "sharp", (6, 16): "sharp", (3, 16): "low", (7, 16): "low", (8, 16): "one_gram"}


def _gc_table(rng, R, M):
    """{column: base ids} of max_order M over radix R: grams of every order 2..M, the prefix and the suffix of a longest one,
    'aa' and 'aaa'; R = 2 has only the runs of its one label; R = 234 holds the largest key, eight 233s"""
    seqs = set()
    if R == 2:
        seqs = {(1,) * k for k in range(2, M + 1)}
    elif M >= 2:
        a = int(rng.integers(1, R))
        seqs |= {(a, a), (a, a, a)} if M >= 3 else {(a, a)}
        for k in range(2, M + 1):
            seqs |= {tuple(int(v) for v in rng.integers(1, R, size=k)) for _ in range(int(rng.integers(1, 4)))}
        g = max(sorted(seqs), key=len)
        if len(g) >= 3:
            seqs |= {g[:-1], g[1:]}
        if R == 234:
            seqs.add((R - 1,) * M)
    return {R + i: list(s) for i, s in enumerate(sorted(seqs))}


def _gc_frames(tgt, l2i, M):
    """the fewest frames that spell tgt (every unigram is a column; two equal grams in a row need a blank between them)"""
    key = {tuple(v): c for c, v in l2i.items()}
    best = [dict() for _ in range(len(tgt) + 1)]     # boundary -> {column of the last gram: frames}
    best[0][0] = 0
    for j in range(len(tgt)):
        for last, f in best[j].items():
            for k in range(1, min(M, len(tgt) - j) + 1):
                c = tgt[j] if k == 1 else key.get(tuple(tgt[j:j + k]))
                if c is not None:
                    n = f + (2 if c == last else 1)
                    best[j + k][c] = min(n, best[j + k].get(c, n))
    return min(best[-1].values()) if len(tgt) else 1


def _gc_case(rng, case, dtype, big=False):
    """The exact width in the band of the (max_order, K) pair GC_PAIRS[case % 40]"""
    M, K = (1, 16) if big else GC_PAIRS[case % len(GC_PAIRS)]
    mode = "plain" if big else GC_MODES.get((M, K), "plain")
    lo, hi = GC_BANDS[M][K]
    if M == 1:
        R = int(rng.choice([1, 2, 5, 29])) if K == 16 and not big else int(rng.choice([2, 5, 29]))
    else:
        R = 234 if M == 8 and K in (4, 1) else int(rng.choice([2, 3, 5, 8, 29]))
    l2i = _gc_table(rng, R, M)
    V = R + len(l2i)
    grams = [g for g in l2i.values()]
    if R == 1:
        W = 0
    elif big:
        W = int(rng.integers(1, 21))
    elif mode in ("sharp", "low"):
        W = 30 if mode == "sharp" else 20
    elif mode == "one_gram":
        W = 8
    else:
        W = int(rng.integers(lo, (hi if K > 1 else hi - 1) + 1))
    B = 300 if big else int(rng.integers(4, 7)) if mode in ("sharp", "low") else int(rng.integers(1, 7 if W < 200 else 3))

    def spell(S):
        t = []
        while len(t) < S:
            g = grams[int(rng.integers(len(grams)))] if grams and rng.random() < 0.7 else [int(rng.integers(1, R))]
            t += list(g) * int(rng.integers(1, 3))   # the same gram twice in a row, often
        return t[:S]

    tg = np.zeros((B, W), dtype=np.int64)
    for b in range(B):
        eights = [g for g in grams if len(g) == 8]
        tg[b] = spell(W) if mode != "one_gram" else eights[b % len(eights)]
    tl = rng.integers(0, W + 1, size=B)
    tl[0] = W
    if mode == "one_gram":
        tl[:] = 8
    need = [_gc_frames(tg[b, :tl[b]].tolist(), l2i, M) for b in range(B)]
    if mode == "sharp":
        T = 600
    elif mode == "low":
        T = 120
    elif mode == "one_gram":
        T = 1
    else:
        T = need[0] + int(rng.choice([0, 0, 1, K - 1, K, K + 1, int(rng.integers(0, W + 3))]))
    xl = np.array([T] + [_lengths(rng, need[b], K, T) for b in range(1, B)], dtype=np.int64)
    if mode in ("sharp", "low"):
        xl[1:] = rng.integers(min(80, T), T + 1, size=B - 1)
    for b in range(1, B):                            # a bad target now and then: 0, or an id >= R
        if tl[b] >= 1 and rng.random() < 0.1:
            tg[b, int(rng.integers(0, tl[b]))] = int(rng.choice([0, R, V + 5]))
    x, logprobs = _inputs(rng, B, T, V, "plain" if mode == "one_gram" else mode, dtype)
    c = dict(x=x, logprobs=logprobs, tg=tg, tl=tl.astype(np.int64), xl=xl, V=V, R=R, M=M, l2i=l2i, mode=mode,
             pad=_wider(GC_BANDS[M], W, rng))
    return _common(rng, c, B)


def _gc_want(c):
    lp = (c["x"].double() if c["logprobs"] else torch.log_softmax(c["x"].double(), -1)).numpy()
    B, T, V = lp.shape
    grams = GR.grams_of(c["R"], V, c["l2i"])
    want_l, want_g = np.zeros(B), np.zeros((B, T, V))
    for b in range(B):
        n, s = int(c["xl"][b]), int(c["tl"][b])
        t = c["tg"][b, :s]
        if ((t < 1) | (t >= c["R"])).any():          # a bad target: NaN loss and slab
            want_l[b], want_g[b] = np.nan, np.nan
            continue
        want_l[b], post = GR.lattice(lp[b, :n], t, grams)
        with np.errstate(invalid="ignore"):
            want_g[b, :n] = np.exp(lp[b, :n]) - post
    return want_l, want_g


@pytest.mark.parametrize("dtype,seed,n", [(torch.float32, 30, 48), (torch.float64, 31, 48)], ids=["f32_seed30", "f64_seed31"])
def test_gram_family_against_the_f64_lattice(dtype, seed, n):
    from end2end_amd.engines import GramCTCLossEngine
    rng = np.random.default_rng(seed)
    bad, reached, reasons = [], set(), set()
    for case in range(n + 1):
        c = _gc_case(rng, case, dtype, big=case == n)
        want_l, want_g = _gc_want(c)
        eng = GramCTCLossEngine(0, c["R"], c["V"], c["l2i"])
        assert eng.max_order == c["M"]
        r = _run_twice("gram", c, eng, want_l, want_g, rng, lambda w: (c["M"], gc_block(w, c["M"])), reached, reasons)
        if r:
            bad.append((case, c["mode"], tuple(c["x"].shape), c["R"], c["M"], int(c["tl"].max()), c["pad"], c["view"],
                        c["logprobs"], r))
    assert not bad, "mismatching cases of seed %d: %s" % (seed, bad)
    assert reached == set(GC_PAIRS), "(max_order, K) not reached: %s" % sorted(set(GC_PAIRS) - reached)
    if dtype == torch.float32:
        assert {1, 2} <= reasons, "redo reasons reported: %s" % sorted(reasons)


# ---------------------------------------------------------------------------------------------------------------------
# callshape: cases of the generators above (new seeds) under a randomised CALL SHAPE -- what the families above never vary.
# The library picks its kernels from the targets tensor's width (Smax), not from the lengths, so a padded batch runs other
# kernels than the same batch at its exact width; grad_scale is applied by whichever kernel writes a gradient element and the
# reduction by whichever workgroup ends the call.  Expected values: the oracle on the exact-width targets, times the scale in
# f64.  Every draw of the shape comes from a generator of its own, so the case generators keep their streams.
# ---------------------------------------------------------------------------------------------------------------------
# around every edge of the dispatch (95/96: the compact alphabet of Smax + 1 columns reaches the lattice kernels' 96/97), one well beyond
CS_WIDTHS = [63, 64, 95, 96, 127, 128, 223, 224, 255, 256, 447, 448, 600]
CS_BANDS = [(0, 63), (64, 95), (96, 127), (128, 223), (224, 255), (256, 447), (448, 1 << 30)]
CS_PAD_KINDS = ["-1", "V", "blank", "valid", "2**40", "-2**63"]
CS_LAYOUTS = ["contiguous", "time_major", "strided", "pitch"]
CS_SCALES = [1.0, 0.37, None, -3.0]                                   # (None: 1 / B)
CS_REDUCTIONS = [None, "sum", "mean"]
# flag routes of a fast-path call (include/e2e_ctc_debug.h, e2e_debug_fast_state): what the flagged launch had to do
CS_FLAG_ROUTES = ["none", "segments4", "segments8", "extended", "full"]


def _cs_band(width):
    return next(i for i, (lo, hi) in enumerate(CS_BANDS) if lo <= width <= hi)


def _cs_shape(rs, tl, B, V, blank):
    """the call shape of one case, drawn from `rs`"""
    W = max(int(np.max(tl)), 1)
    wider = [w for w in CS_WIDTHS if w > W and _cs_band(w) != _cs_band(W)]
    width = W if (not wider or rs.random() < 0.2) else int(rs.choice(wider))
    labels = [v for v in range(V) if v != blank] or [blank]
    fill = {"-1": -1, "V": V, "blank": blank, "2**40": 1 << 40, "-2**63": -(1 << 63)}
    kinds = [str(rs.choice(CS_PAD_KINDS)) for _ in range(B)]
    padding = [fill[k] if k != "valid" else int(rs.choice(labels)) for k in kinds]
    row_stride = width if rs.random() < 0.5 else width + int(rs.integers(1, 41))
    scale = CS_SCALES[int(rs.integers(0, 4))]
    return dict(width=width, padded=width > W, half=2 * W <= width, padding=padding, row_stride=row_stride,
                layout=str(rs.choice(CS_LAYOUTS)), scale=1.0 / B if scale is None else scale,
                reduction=CS_REDUCTIONS[int(rs.integers(0, 3))])


def _cs_layout(x, layout):
    """x (B, T, V) on the host as the call gets it: contiguous, a time-major view, column-strided (sV = 2), or with a gap
    between the utterances (c_abi_loss keeps the strides on its way to the GPU)"""
    B, T, V = x.shape
    if layout == "time_major":
        return x.permute(1, 0, 2).contiguous().permute(1, 0, 2)
    if layout == "strided":
        w = torch.zeros(B, T, 2 * V, dtype=x.dtype)
        w[:, :, ::2] = x
        return w[:, :, ::2]
    if layout == "pitch":
        w = torch.zeros(B, T + 3, V, dtype=x.dtype)
        w[:, :T] = x
        return w[:, :T]
    return x.contiguous()


def _cs_flag_routes(keep, B, T, V):
    """what the flagged launch of a fast-path AUTO call did, from the flag words the chains and the segment kernel left
    (masked to the bits include/e2e_ctc_debug.h documents; 512 is the launch's own)"""
    L = _lib.load()
    flags, logz = (ctypes.c_int * B)(), (ctypes.c_double * (2 * B))()
    assert L.e2e_debug_fast_state(keep["workspace"].data_ptr(), B, T, V, keep["Smax"], flags, logz) == 0
    raw = np.array(flags[:], dtype=np.int64)
    f = raw & 511                                                  # what the chains and the segment kernel reported
    took_ext = (raw & 2048) != 0                                   # the extended-range redo ran this utterance's chains (round 0 or 1)
    full = ((f & (1 | 2 | 128 | 256)) != 0) | ((raw & 4096) != 0)
    rng_only = (f != 0) & ((f & ~(8 | 16)) == 0) & ~took_ext
    out = set()
    if not f.any():
        out.add("none")
    if full.any():
        out.add("full")
    if took_ext.any():
        out.add("extended")
    pairs = keep["route"] // 10 % 10
    if rng_only.any() and pairs in (4, 8):                         # settled by the f64 redo of their flagged segments
        out.add("segments%d" % pairs)
    return out


class _CsLog:
    """what the family reached: route code -> set of marks ('padded', 'scale', 'reduction'), the same per flag route,
    the bands in which a genuinely padded case (max(t_len) at most half the width) ran"""
    def __init__(self):
        self.routes, self.flag_routes, self.half_bands, self.row_forms = {}, {}, set(), {}

    def add(self, sh, keep, flag_routes):
        marks = {"any"} | ({"padded"} if sh["padded"] else set())
        if sh["padded"] and sh["scale"] != 1.0:
            marks.add("scale")
        if sh["padded"] and sh["reduction"]:
            marks.add("reduction")
        self.routes.setdefault(keep["route"], set()).update(marks)
        for fr in flag_routes:
            m = self.flag_routes.setdefault(fr, set())
            m.update(({"scale"} if sh["scale"] != 1.0 else set()) | ({"reduction"} if sh["reduction"] else set()))
            if sh["scale"] != 1.0 and sh["reduction"]:
                m.add("both")
        if sh["padded"] and sh["half"]:
            self.half_bands.add(_cs_band(sh["width"]))


CS_LOG = _CsLog()
CS_SEEN = []          # (style, seed) of the slices that ran: the coverage test below needs all of them


def _cs_run(c_x, logprobs, tg, xl, tl, blank, algo, sh, tol, log, io16=None):
    """One call under the shape `sh` against the oracle -> None, or the first difference.  c_x: what the call is given (a host
    tensor of the call's dtype).  tol = (loss rtol, loss atol, grad rtol, grad atol before the scale)."""
    tg, xl, tl = np.asarray(tg), np.asarray(xl), np.asarray(tl)
    B, T, V = c_x.shape
    lp = c_x.double() if logprobs else torch.log_softmax(c_x.double(), -1)
    l_o, g_o = O.ctc_loss(lp.numpy(), tg, xl, tl, blank)                  # (the exact-width targets)
    if not logprobs:
        for b in range(B):
            if np.isfinite(l_o[b]):
                g_o[b, int(xl[b]):] = 0.0                                  # (an infeasible utterance stays NaN everywhere, quirk Q2)
    g_o = g_o * sh["scale"]
    red = {None: _lib.REDUCE_NONE, "sum": _lib.REDUCE_SUM, "mean": _lib.REDUCE_MEAN}[sh["reduction"]]
    keep = {}
    la, ga, got_red = U.c_abi_loss(_cs_layout(c_x, sh["layout"]), tg, xl, tl, blank, logprobs, algo, keep=keep,
                                   opts=(sh["scale"], red), width=sh["width"], padding=sh["padding"], row_stride=sh["row_stride"])
    assert keep["route"] > 0, "the route diagnostic refuses a call that ran: %d" % keep["route"]
    flag_routes = _cs_flag_routes(keep, B, T, V) if (keep["route"] // 1000 == 2 and algo == _lib.ALGO_AUTO) else set()
    log.add(sh, keep, flag_routes)
    if io16 is not None:
        ga = torch.from_numpy(ga).to(io16).float().numpy()                 # (an up-cast call: the engine rounds the gradient back)
    lr, la_, gr, ga_ = tol
    try:
        U.assert_same(la, l_o, lr, la_, "losses")
        U.assert_same(ga, g_o, gr, ga_ * abs(sh["scale"]), "grads")
        if sh["reduction"]:
            # 1. against the oracle: the per-loss tolerance summed over the batch
            want = l_o.sum() if sh["reduction"] == "sum" else l_o.mean()
            if np.isnan(l_o).any():
                assert np.isnan(got_red), "reduced %r, want NaN" % got_red
            elif np.isinf(l_o).any():
                assert got_red == np.inf, "reduced %r, want +inf" % got_red
            else:
                bound = (lr * np.abs(l_o) + la_).sum() / (B if sh["reduction"] == "mean" else 1)
                assert abs(float(got_red) - want) <= bound, "reduced %r, oracle %r" % (got_red, want)
                # 2. against the f64 sum of the losses this call returned.  Every writer of the reduced loss accumulates in f64 and
                # rounds once to the result's type: the flagged launch (write_reduction in ctc_exact_kernel) and, behind the exact
                # kernel and the wide path (after its loss correction), reduce_losses_kernel.  So the bound is one rounding of the
                # result's type, plus B roundings of the f64 accumulation in whatever order
                l64 = la.astype(np.float64)
                own = l64.sum() / (B if sh["reduction"] == "mean" else 1)
                eps = 2.0 ** -53 if c_x.dtype == torch.float64 else 2.0 ** -24
                assert abs(float(got_red) - own) <= eps * abs(own) + (B + 1) * 2.0 ** -53 * np.abs(l64).sum(), \
                    "reduced %r, the call's own losses give %r" % (got_red, own)
        return None
    except AssertionError as e:
        return ["route %d %s" % (keep["route"], sorted(flag_routes))] + str(e).strip().splitlines()[:5]


def _cs_describe(sh):
    return "width %d stride %d %s scale %g %s pad %s" % (sh["width"], sh["row_stride"], sh["layout"], sh["scale"], sh["reduction"],
                                                         sorted(set(sh["padding"])))


def _takes_dtype(x, algo, width):
    """e2e_ctc_loss_takes_dtype as CTCLossEngine.compute asks it"""
    B, T, V = x.shape
    sB, sT, sV = x.stride()
    return bool(_lib.load().e2e_ctc_loss_takes_dtype(_lib.dtype_code(x.dtype), algo, T, V, width, sB, sT, sV, None, None))


G16 = {None: (1e-4, 2e-6), torch.bfloat16: (2.0 ** -7, 2.0 ** -8), torch.float16: (2.0 ** -10, 2.0 ** -11)}


@pytest.mark.parametrize("style,seed,n,dtype", [("ext", 40, 120, None), ("ext", 41, 40, torch.bfloat16), ("ext", 42, 40, torch.float16),
                                                ("fastauto", 43, 120, None), ("scaled", 44, 60, None), ("exact", 45, 40, None)],
                         ids=["ext_f32_seed40", "ext_bf16_seed41", "ext_f16_seed42", "fastauto_seed43", "scaled_seed44", "exact_seed45"])
def test_callshape_family_against_the_oracle(style, seed, n, dtype):
    rng = np.random.default_rng(seed)                   # the cases: the generators' own stream
    rs = np.random.default_rng(1000 + seed)             # the call shapes
    bad, marginal, done = [], [], 0
    for case in range(n):
        algo, io16, up16 = _lib.ALGO_AUTO, dtype, None
        if style == "ext":
            c = _ext_case(rng)
            if c["logprobs"] and dtype is not None:
                continue                                 # (16-bit log-probabilities cannot hold these: logits only)
            xt, logprobs, blank = torch.from_numpy(c["x"]), c["logprobs"], c["blank"]
            x = torch.log_softmax(xt, -1).float() if logprobs else (xt.float() if io16 is None else xt.to(io16))
            tg, xl, tl = c["tg"], c["xl"], c["tl"]
        elif style == "fastauto":
            c = _fast_case(rng)
            xt, logprobs, blank = torch.from_numpy(c["x"]), c["logprobs"], c["blank"]
            io16 = None if logprobs else [None, None, torch.bfloat16, torch.float16][case % 4]
            x = xt.float() if io16 is None else xt.to(io16)
            if logprobs:
                x = torch.log_softmax(x.double(), -1).float()
            tg, xl, tl = c["tg"], c["xl"], c["tl"]
        else:
            c = _small_case(rng, case, style, wide=(style == "scaled" and case % 3 == 0))
            x, logprobs, blank = c["inp"], not c["fused"], c["blank"]
            tg, xl, tl = c["tg"].numpy(), c["xl"].numpy(), c["tl"].numpy()
            algo = _lib.ALGO_AUTO if style == "scaled" else _lib.ALGO_EXACT
        B, T, V = x.shape
        sh = _cs_shape(rs, tl, B, V, blank)
        if io16 is not None and not _takes_dtype(_cs_layout(x, sh["layout"]), algo, sh["width"]):
            x, up16 = x.float(), io16                    # as CTCLossEngine.compute: up-cast, the gradient rounded back
        if style in ("scaled", "exact"):
            tol = (1e-9, 1e-12, 1e-9, 1e-12) if c["f64"] else (1e-4, 2e-6, 1e-4, 2e-6)
        else:
            tol = (1e-4, 2e-5) + G16[io16]
        r = _cs_run(x, logprobs, tg, xl, tl, blank, algo, sh, tol, CS_LOG, io16=up16)
        if r is not None and style == "ext":
            # the ext family's marginal rule, unchanged: single elements within 1e-5 (times |scale|), at most max(1, done // 50) cases
            r2 = _cs_run(x, logprobs, tg, xl, tl, blank, algo, sh, tol[:3] + (max(1e-5, 2 * tol[3]),), _CsLog(), io16=up16)
            if r2 is None:
                marginal.append(case)
                r = None
        done += 1
        _count("callshape_upcast" if up16 is not None else "callshape", B)
        if r is not None:
            bad.append((case, tuple(x.shape), str(x.dtype), int(np.max(tl)), blank, logprobs, _cs_describe(sh), r))
    CS_SEEN.append((style, seed))
    assert not bad, "mismatching cases of %s seed %d: %s" % (style, seed, bad)
    assert len(marginal) <= max(1, done // 50), "marginal cases (one element within 1e-5) of seed %d: %s" % (seed, marginal)


def _cs_key(route):
    """a route code without its row-kernel digit: (path, 10 * pairs + rule)"""
    return route // 1000, route % 100


# what the generators' alphabets and the widths above reach (B <= 8: not the ring of four blocks; no f32 chains; rows of
# 2049..4096 and of more than 8192 columns are in no generator)
CS_ROUTES = {(1, 0), (2, 16), (2, 24), (2, 26), (2, 44), (2, 45), (2, 46), (2, 41), (2, 81), (2, 82),
             (3, 16), (3, 24), (3, 26), (3, 41), (3, 81), (4, 0)}
CS_ROW_FORMS = {0, 2, 4}


def test_callshape_family_reached_every_route_padded_scaled_and_reduced():
    """A fuzz that never leaves one route proves little.  Runs a deterministic sweep -- unit noise, targets of at most 30 labels,
    every alphabet class at EVERY width of CS_WIDTHS, scale and reduction alternating -- and four batches built like
    tests/test_gpu_regimes.py's for the flag routes, then asserts over them and the random slices above: every route the
    generators can reach was reached by a padded case, with grad_scale != 1 and with a reduction; every flag route was seen with
    grad_scale != 1 and with a reduction; every band had a batch padded to at least twice its longest target."""
    for params in [("ext", 40, 120, None), ("ext", 41, 40, torch.bfloat16), ("ext", 42, 40, torch.float16),
                   ("fastauto", 43, 120, None), ("scaled", 44, 60, None), ("exact", 45, 40, None)]:
        if params[:2] not in CS_SEEN:                    # (this test selected alone: the slices run here)
            test_callshape_family_against_the_oracle(*params)
    bad = []
    rng = np.random.default_rng(50)
    combos = [(0.37, "sum"), (-3.0, "mean"), (0.125, None), (1.0, "sum")]
    k = 0
    for V in (29, 80, 150, 300, 1000, 8000):
        B, T, S = 3, 120, 30
        for width in CS_WIDTHS:
            x = torch.from_numpy(rng.standard_normal((B, T, V))).float()
            tg = rng.integers(1, V, size=(B, S)); tl = rng.integers(1, S + 1, size=B); tl[0] = S
            xl = np.array([T, T - 9, T // 2 + 20])
            for scale, reduction in (combos[k % 4], combos[(k + 1) % 4]):
                sh = dict(width=width, padded=True, half=True, padding=[-1, V, 1 << 40], row_stride=width + 5 * (k % 2),
                          layout=CS_LAYOUTS[k % 4], scale=scale, reduction=reduction)
                r = _cs_run(x, False, tg, xl, tl, 0, _lib.ALGO_AUTO, sh, (1e-4, 2e-5, 1e-4, 2e-6), CS_LOG)
                _count("callshape", B)
                if r is not None:
                    bad.append(("sweep", V, _cs_describe(sh), r))
            k += 1
    # flag routes, deterministic: (a) a trained model's batch with mislabelled utterances (extended range), sharp unrelated ones
    # (range flags: they join the extended-range redo) and a blank-valued target (full recomputation); (b) sharp unrelated
    # emissions at scale 3, flagged for range only: the f64 redo of single segments, in the four-pairs instance at the exact
    # width and, padded to 300 columns, in the eight-pairs instance
    from test_gpu_regimes import aligned
    rng = np.random.default_rng(77)
    x, tg, xl, tl = aligned(rng, 12, 1000, 29, 200, 10.0, short=[(5, 933)])
    tg[1], tl[1] = tg[2].copy(), tl[2]
    tg[5], tl[5] = tg[6].copy(), tl[6]
    x[7] = rng.standard_normal(x[7].shape) * 3.0
    x[8] = rng.standard_normal(x[8].shape) * 3.0
    tg[9, 3] = 0
    want = {}
    for width, scale, reduction in ((200, -3.0, "mean"), (224, 0.37, "sum")):
        sh = dict(width=width, padded=width > 200, half=False, padding=[-1] * 12, row_stride=width + 7, layout="contiguous",
                  scale=scale, reduction=reduction)
        log = _CsLog()
        r = _cs_run(torch.from_numpy(x), False, tg, xl, tl, 0, _lib.ALGO_AUTO, sh, (1e-4, 2e-5, 1e-4, 2e-6), log)
        _count("callshape", 12)
        want["a%d" % width] = ({"full"}, set(log.flag_routes))
        CS_LOG.add(sh, {"route": next(iter(log.routes))}, set(log.flag_routes))
        if r is not None:
            bad.append(("flags a", _cs_describe(sh), r))
    rng = np.random.default_rng(504)                     # (c) sharp unrelated emissions at scale 8: the extended-range redo
    B, T, V, S = 4, 500, 29, 100
    x = (rng.standard_normal((B, T, V)) * 8.0).astype(np.float32)
    tg = rng.integers(1, V, size=(B, S)); tl = rng.integers(S // 2, S + 1, size=B); xl = np.array([T, T - 21, T, T])
    for width, scale, reduction in ((100, 0.37, "sum"), (128, -3.0, "mean")):
        sh = dict(width=width, padded=width > 100, half=False, padding=[1 << 40] * B, row_stride=width + 1, layout="time_major",
                  scale=scale, reduction=reduction)
        log = _CsLog()
        r = _cs_run(torch.from_numpy(x), False, tg, xl, tl, 0, _lib.ALGO_AUTO, sh, (1e-4, 2e-5, 1e-4, 2e-6), log)
        _count("callshape", B)
        want["c%d" % width] = ({"extended"}, set(log.flag_routes))
        CS_LOG.add(sh, {"route": next(iter(log.routes))}, set(log.flag_routes))
        if r is not None:
            bad.append(("flags c", _cs_describe(sh), r))
    rng = np.random.default_rng(5)
    B, T, V, S = 8, 1000, 29, 200
    x = (rng.standard_normal((B, T, V)) * 3.0).astype(np.float32)
    tg = rng.integers(1, V, size=(B, S)); tl = rng.integers(S // 2, S + 1, size=B); xl = np.full(B, T)
    for width, scale, reduction in ((200, -3.0, "mean"), (300, 0.37, "sum"), (300, -3.0, "mean")):
        sh = dict(width=width, padded=width > 200, half=False, padding=[V] * B, row_stride=width, layout="pitch",
                  scale=scale, reduction=reduction)
        log = _CsLog()
        r = _cs_run(torch.from_numpy(x), False, tg, xl, tl, 0, _lib.ALGO_AUTO, sh, (1e-4, 2e-5, 1e-4, 2e-6), log)
        _count("callshape", B)
        want["b%d" % width] = ({"segments%d" % (4 if width == 200 else 8)}, set(log.flag_routes))
        CS_LOG.add(sh, {"route": next(iter(log.routes))}, set(log.flag_routes))
        if r is not None:
            bad.append(("flags b", _cs_describe(sh), r))
    L = CS_LOG
    print("callshape routes:", {r: sorted(m) for r, m in sorted(L.routes.items())})
    print("callshape flag routes:", {r: sorted(m) for r, m in sorted(L.flag_routes.items())}, {k: sorted(v[1]) for k, v in want.items()})
    assert not bad, "mismatching cases: %s" % bad
    for name, (need, got) in want.items():
        assert need <= got, "batch %s no longer takes the flag route it was built for: %s, not %s" % (name, sorted(got), sorted(need))

    keys = {}
    for route, marks in L.routes.items():
        keys.setdefault(_cs_key(route), set()).update(marks)
    need = CS_ROUTES | set(keys)
    missing = {k: sorted({"padded", "scale", "reduction"} - keys.get(k, set())) for k in sorted(need)
               if not {"padded", "scale", "reduction"} <= keys.get(k, set())}
    assert not missing, "routes (path, 10 * pairs + rule) not reached by a padded case / with grad_scale != 1 / with a reduction: %s" % missing
    rows = {r // 100 % 10 for r, m in L.routes.items() if r // 1000 in (3, 4) and {"padded", "scale", "reduction"} <= m}
    assert CS_ROW_FORMS <= rows, "row kernels of the wide path reached padded, scaled and reduced: %s" % sorted(rows)
    fmiss = {f: sorted({"scale", "reduction"} - L.flag_routes.get(f, set())) for f in CS_FLAG_ROUTES
             if not {"scale", "reduction"} <= L.flag_routes.get(f, set())}
    assert not fmiss, "flag routes not seen with grad_scale != 1 / with a reduction: %s" % fmiss
    assert set(range(1, len(CS_BANDS))) <= L.half_bands, "bands with a batch padded to twice its longest target: %s" % sorted(L.half_bands)


# ---------------------------------------------------------------------------------------------------------------------
# Labels that only fit in 64 bits.  include/e2e_ctc.h promises NaN for an utterance whose first t_len[b] targets hold a value
# outside [0, V).  Until this family was written the fast and wide paths narrowed a target to 32 bits BEFORE that test, so
# 2**32 + 3 or 3 - 2**32 inside t_len was computed as label 3: a finite loss under AUTO / FAST, NaN under EXACT.
# One shape per reader of the targets.
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,B,T,V,S,scale,algo,chains", [
    ("one_pair_LaneCells_load", 5, 200, 29, 60, 1.0, _lib.ALGO_AUTO, None),
    ("two_pairs_lean_halo", 5, 400, 29, 100, 1.0, _lib.ALGO_AUTO, None),
    ("four_pairs_lean_halo", 5, 600, 29, 200, 1.0, _lib.ALGO_AUTO, None),
    ("four_pairs_f32_chains", 5, 600, 29, 200, 1.0, _lib.ALGO_AUTO, _lib.CHAINS_F32),
    ("four_pairs_f64_halo_V80", 5, 600, 80, 200, 1.0, _lib.ALGO_AUTO, None),
    ("eight_pairs", 5, 800, 29, 300, 1.0, _lib.ALGO_AUTO, None),
    ("wide_rows_V150", 5, 400, 150, 100, 1.0, _lib.ALGO_AUTO, None),
    ("compaction_V8000", 5, 150, 8000, 50, 1.0, _lib.ALGO_AUTO, None),
    ("extended_range_redo", 5, 500, 29, 100, 8.0, _lib.ALGO_AUTO, None),
    ("f64_segment_redo", 8, 1000, 29, 200, 3.0, _lib.ALGO_AUTO, None),
    ("fast_only", 5, 400, 29, 100, 1.0, _lib.ALGO_FAST, None),
    ("exact", 5, 100, 29, 40, 1.0, _lib.ALGO_EXACT, None),
], ids=lambda v: v if isinstance(v, str) else "")
def test_a_label_beyond_32_bits_inside_t_len_poisons_its_utterance_only(name, B, T, V, S, scale, algo, chains):
    redo = name == "f64_segment_redo"          # (the batch of test_gpu_regimes.py's range-flag tests: seed 5, every utterance T frames long)
    rng = np.random.default_rng(5 if redo else len(name) + T)
    x = (rng.standard_normal((B, T, V)) * scale).astype(np.float32)
    tg = rng.integers(1, V, size=(B, S)).astype(np.int64)
    tl = rng.integers(S // 2, S + 1, size=B)
    xl = np.full(B, T)
    if not redo:
        tl[0], xl[B - 1] = S, T - 11
    lp = torch.log_softmax(torch.from_numpy(x).double(), -1).numpy()
    l_o, g_o = O.ctc_loss(lp, tg, xl, tl, 0)                                   # (before the labels are spoilt)
    for b in range(B):
        g_o[b, xl[b]:] = 0.0
    assert np.isfinite(l_o).all()
    bad = tg.copy()
    where = {1: (int(tl[1]) - 1, 1 << 32), 2: (0, -(1 << 32)), 3: (int(tl[3]) // 2, 1 << 40)}    # utterance: (position, offset)
    for b, (i, off) in where.items():
        bad[b, i] += off                                                       # the low 32 bits stay a valid non-blank label
        l_o[b], g_o[b] = np.nan, np.nan
    keep = {}
    la, ga = U.c_abi_loss(torch.from_numpy(x), bad, xl, tl, 0, False, algo, keep=keep, chains=chains)
    if algo == _lib.ALGO_FAST:                                                 # (FAST poisons whatever leaves the f32 lattice, too)
        assert np.isnan(la[[1, 2, 3]]).all() and np.isnan(ga[[1, 2, 3]]).all(), la
        return
    U.assert_same(la, l_o, 1e-4, 2e-5, "losses (route %d)" % keep["route"])
    U.assert_same(ga, g_o, 1e-4, 2e-5 if chains else 2e-6, "grads (route %d)" % keep["route"])
    want_route = {"one_pair_LaneCells_load": 2016, "two_pairs_lean_halo": 2024, "four_pairs_lean_halo": 2044, "four_pairs_f32_chains": 2043,
                  "four_pairs_f64_halo_V80": 2045, "eight_pairs": 2082, "wide_rows_V150": 2041, "compaction_V8000": 3416,
                  "extended_range_redo": 2024, "f64_segment_redo": 2044, "exact": 1000}[name]
    assert keep["route"] == want_route, (keep["route"], want_route)
    if name in ("extended_range_redo", "f64_segment_redo"):
        got = _cs_flag_routes(keep, B, T, V)
        assert {"extended_range_redo": "extended", "f64_segment_redo": "segments4"}[name] in got and "full" in got, got


# ---------------------------------------------------------------------------------------------------------------------
# The module on a headline-like batch whose targets tensor is padded, as a collate function pads it
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_module_on_a_padded_headline_like_batch(dtype):
    """CTCLoss(reduce=True, size_average=True / False) and reduce=False with a weighted backward on B=8, T=1000, V=29, S<=120,
    the targets padded with -1 to 129, 224, 300, 448 and 600 columns: four pairs per lane on the lean halo chains, the
    single-wave chains, eight pairs per lane, and -- from 448 columns on -- the exact kernel (16-bit logits up-cast by the
    engine).  Loss and input gradient against the oracle at every width."""
    from end2end_amd import CTCLoss
    rng = np.random.default_rng(8)
    B, T, V, S = 8, 1000, 29, 120
    x = torch.from_numpy(rng.standard_normal((B, T, V))).float().to(dtype)
    tg = rng.integers(1, V, size=(B, S)); tl = rng.integers(S // 2, S + 1, size=B); tl[0] = S
    xl = rng.integers(T // 2, T + 1, size=B); xl[0] = T
    l_o, g_o = O.ctc_loss(torch.log_softmax(x.double(), -1).numpy(), tg, xl, tl, 0)
    for b in range(B):
        g_o[b, xl[b]:] = 0.0
    w = np.array([1.0, -2.0, 0.5, 4.0, -1.0, 0.25, 2.0, -0.5])                 # the weights of the reduce=False backward: powers of two,
                                                                               # so that a 16-bit gradient is rounded once, by the kernel
    g_rtol, g_atol = G16[None if dtype == torch.float32 else dtype]
    for width in (129, 224, 300, 448, 600):
        pad = U.padded_targets(tg, tl, width, -1)
        for mode, want_l, want_g in (("mean", l_o.mean(), g_o / B), ("sum", l_o.sum(), g_o), ("none", l_o, g_o * w[:, None, None])):
            xd = x.to(DEV).requires_grad_()
            mod = CTCLoss(reduce=mode != "none", size_average=mode == "mean")
            loss = mod(xd, pad, torch.from_numpy(xl).to(DEV), torch.from_numpy(tl).to(DEV))
            if mode == "none":
                loss.backward(torch.from_numpy(w).to(DEV, loss.dtype))
            else:
                loss.backward()
            what = "%s, %d columns" % (mode, width)
            # (a 16-bit module returns its loss in the logits' dtype: one rounding of that type on top of the f32 bound)
            l_rtol = 1e-4 if dtype == torch.float32 else 1e-4 + 2.0 ** -8
            U.assert_same(loss.detach().double().cpu().numpy(), want_l, l_rtol, 2e-5, "loss (%s)" % what)
            wmax = 1.0 if mode != "none" else float(np.abs(w).max())
            U.assert_same(xd.grad.double().cpu().numpy(), want_g, g_rtol, g_atol * wmax, "gradient (%s)" % what)
