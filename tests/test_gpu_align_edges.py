"""-m gpu: forced alignment (e2e_ctc_align) at the shapes where its code branches -- the wide sweep and the switch between
the two sweeps, the back-trace's chunk edges, the widest lattice the call accepts, a non-zero blank, strided calls, and the
rows the header defines without a lattice.

Every labelling is compared with the oracle's (oracle/ctc_oracle.c: upstream's function restated, its tie rule included)
label for label, and every feasible utterance with tests/align_ref.py as well: the labelling is a legal walk through the
lattice and its f64 score is the best there is, EXACTLY (tests/test_align_ref_cpu.py pins that reference on the CPU).
The tests whose point is a row without a feasible walk are compared with the oracle only, and say so."""
import os

import numpy as np
import pytest
import torch

import align_ref as AR
import gpu_util as U
import oracle_lib as O
from end2end_amd import _lib
from test_gpu_align import c_abi_align

pytestmark = pytest.mark.gpu

DTYPES = {"f32": torch.float32, "f64": torch.float64, "f16": torch.float16, "bf16": torch.bfloat16}
PAD = -100
UNSUPPORTED = -2                        # E2E_ERR_UNSUPPORTED (include/e2e_ctc.h)
CTC_MAX_S, ASG_MAX_S = 3172, 6345       # the widest targets e2e_ctc_align accepts (include/e2e_ctc.h states them)


# ---- inputs ---------------------------------------------------------------------------------------------------------
def make_targets(rng, S, V, is_ctc, blank, doubles=0.05):
    """S labels (never the blank for CTC), no label twice in a row except at a fraction `doubles` of the positions."""
    labels = np.array([v for v in range(V) if not (is_ctc and v == blank)])
    idx = np.cumsum(rng.integers(1, len(labels), size=S)) % len(labels)          # neighbours differ
    if doubles and S > 1:
        for i in np.flatnonzero(rng.random(S) < doubles):
            if i > 0:
                idx[i] = idx[i - 1]
    return labels[idx]


def need(tg, is_ctc):
    tg = np.asarray(tg)
    return max(len(tg) + (int((tg[1:] == tg[:-1]).sum()) if is_ctc else 0), 1)


def emissions(rng, shape, quantised):
    """f64 (B,T,V): log-softmax of 2 * randn rounded to f32, or multiples of 1/8 in [-8, 0] (exact in every dtype)."""
    if quantised:
        return AR.quantised(rng, shape)
    x = torch.from_numpy(rng.standard_normal(shape) * 2.0)
    return torch.log_softmax(x, -1).float().double().numpy()


def check(got, lp64, tg, xl, tl, blank, is_ctc, what="", reference=True):
    """The whole batch against the oracle, label for label; every feasible utterance against the plain reference
    (reference=False: where every walk scores -inf the strict ">" never moves and the result is no walk)."""
    want = O.ctc_align(lp64, tg, xl, tl, blank, is_ctc, pad=PAD, n_threads=16)
    assert np.array_equal(got, want), (what, np.argwhere(got != want)[:5].tolist())
    for b in range(len(xl)):
        T, S = int(xl[b]), int(tl[b])
        assert (got[b, T:] == PAD).all()
        if reference and T >= 2 and (S >= 1 or is_ctc) and AR.feasible(tg[b, :S], T, is_ctc):
            AR.check_utterance(lp64[b], got[b], tg[b, :S], T, is_ctc, blank)
    return want


def run(lp64, tg, xl, tl, blank, is_ctc, dtype=torch.float32, what=""):
    got = c_abi_align(torch.from_numpy(lp64).to(dtype), tg, xl, tl, blank, is_ctc, PAD)
    check(got, lp64, np.asarray(tg).reshape(len(xl), -1), xl, tl, blank, is_ctc, what)
    return got


# ---- width edges ----------------------------------------------------------------------------------------------------
def width_batch(rng, S, is_ctc, tight, V, blank, quantised):
    """Four utterances: the full width S; one just below the switch between the two sweeps (L <= 512 cells) in a batch whose
    rows of codes are Lpad(S) apart; three labels; half the width.  tight: as many frames as the labelling needs (a blank
    between doubled labels) and not one more; otherwise about 2 S."""
    below = 255 if is_ctc else 512
    sizes = [S, min(below, S - 1), 3, S // 2]
    tg = np.stack([make_targets(rng, S, V, is_ctc, blank) for _ in sizes])       # (valid labels beyond t_len too)
    if tight:
        xl = [max(need(tg[b, :s], is_ctc), 2) for b, s in enumerate(sizes)]
    else:
        T = 2 * S + 5
        xl = [T, T - 3, 9, S + 7]
    lp = emissions(rng, (len(sizes), max(xl), V), quantised)
    return lp, tg, np.array(xl), np.array(sizes)


CTC_WIDTHS = [127, 128, 255, 256, 257, 383, 384, 511, 512]       # L = 255 .. 1025: the 512-cell switch, the 256-lane strides
ASG_WIDTHS = [255, 256, 257, 511, 512, 513, 768, 769]
WIDTHS = [(True, s) for s in CTC_WIDTHS] + [(False, s) for s in ASG_WIDTHS]
width_id = lambda w: ("ctc" if w[0] else "asg") + str(w[1])


@pytest.mark.parametrize("tight", [True, False], ids=["tight", "loose"])
@pytest.mark.parametrize("width", WIDTHS, ids=width_id)
def test_width_edges_random(width, tight):
    is_ctc, S = width
    rng = np.random.default_rng(1000 + S + 7 * is_ctc + tight)
    lp, tg, xl, tl = width_batch(rng, S, is_ctc, tight, 12, 0, False)
    run(lp, tg, xl, tl, 0, is_ctc, torch.float32, width_id(width))


@pytest.mark.parametrize("tight", [True, False], ids=["tight", "loose"])
@pytest.mark.parametrize("width", WIDTHS, ids=width_id)
def test_width_edges_quantised_give_one_labelling_in_every_dtype(width, tight):
    """Emissions that every dtype holds exactly and f64 adds exactly: ties everywhere (upstream's order stay, i-1, i-2
    decides, the oracle has it), one labelling whatever the dtype.  Blank 5 of 9 columns."""
    is_ctc, S = width
    rng = np.random.default_rng(2000 + S + 7 * is_ctc + tight)
    lp, tg, xl, tl = width_batch(rng, S, is_ctc, tight, 9, 5, True)
    first = run(lp, tg, xl, tl, 5, is_ctc, torch.float64, width_id(width))
    for name in ("f32", "f16", "bf16"):
        got = c_abi_align(torch.from_numpy(lp).to(DTYPES[name]), tg, xl, tl, 5, is_ctc, PAD)
        assert np.array_equal(got, first), name


@pytest.mark.parametrize("width", [(True, 100), (True, 300), (False, 100), (False, 600)], ids=width_id)
def test_flat_emissions_every_comparison_is_a_tie(width):
    """Every emission -2: all walks score alike, so every comparison of both sweeps is a tie, the choice of the end cell
    (blank or last label) included; upstream's order -- stay, then i-1, then i-2, the last blank at the end -- decides."""
    is_ctc, S = width
    rng = np.random.default_rng(2500 + S)
    _, tg, xl, tl = width_batch(rng, S, is_ctc, False, 9, 5, True)
    run(np.full((4, int(xl.max()), 9), -2.0), tg, xl, tl, 5, is_ctc, torch.float32, width_id(width))


# ---- chunk edges ----------------------------------------------------------------------------------------------------
def chunk_rows(Lpad):
    """Frames of back-pointer codes the back-trace stages per chunk (ctc_align.hip: kChunkBytes = 32 KiB of codes, rows Lpad
    bytes apart, at most kChunkBytes / 64 = 512 of them)."""
    return max(1, min(32768 // Lpad, 512))


CHUNK_SMAX = {(True, 16): 7, (True, 64): 31, (True, 80): 39, (True, 416): 207, (True, 1040): 519,
              (False, 16): 16, (False, 64): 63, (False, 80): 80, (False, 416): 401, (False, 1040): 1040}


@pytest.mark.parametrize("edge", ["rows-1", "rows", "rows+1", "2rows", "2rows+1", "2rows+3"])
@pytest.mark.parametrize("Lpad", [16, 64, 80, 416, 1040])
@pytest.mark.parametrize("is_ctc", [True, False], ids=["ctc", "asg"])
def test_back_trace_chunk_edges(is_ctc, Lpad, edge):
    """The back-trace stages rows = max(1, min(32768 / Lpad, 512)) frames of codes per chunk, Lpad = the lattice of the
    targets' WIDTH (2 Smax + 1, ASG: Smax) rounded up to 16; it walks a chunk four frames at a time with a remainder loop and
    replaces frame 0's codes in the last chunk.  T = rows - 1, rows, rows + 1, 2 rows, 2 rows + 1, 2 rows + 3 for Lpad = 16 and
    64 (rows = 512, the cap: T = 511 .. 1027), 80 (409), 416 (78), 1040 (31).  A change of kChunkBytes moves these edges:
    chunk_rows() above then has to follow.  (The width sets Lpad; t_len is what fits the frames.)"""
    Smax = CHUNK_SMAX[is_ctc, Lpad]
    assert (((2 * Smax + 1 if is_ctc else Smax) + 15) & ~15) == Lpad
    rows = chunk_rows(Lpad)
    T = {"rows-1": rows - 1, "rows": rows, "rows+1": rows + 1, "2rows": 2 * rows, "2rows+1": 2 * rows + 1, "2rows+3": 2 * rows + 3}[edge]
    rng = np.random.default_rng(3000 + Lpad + 10 * T + is_ctc)
    V = 7
    xl = np.array([T, T, T - 2])
    tl = np.array([min(Smax, T - 2), min(Smax, 3), min(Smax, max(T // 4, 1))])       # (the first: tight where the width allows)
    tg = np.stack([make_targets(rng, Smax, V, is_ctc, 0, doubles=0) for _ in xl])
    lp = emissions(rng, (3, T, V), quantised=bool(T & 1))
    run(lp, tg, xl, tl, 0, is_ctc, torch.float32, "Lpad=%d T=%d" % (Lpad, T))


@pytest.mark.parametrize("is_ctc", [True, False], ids=["ctc", "asg"])
def test_every_length_up_to_sixty(is_ctc):
    """B = 60, T = 60, x_len = 1 .. 60, one, three or x_len labels: every length against the sweep's register pipeline (three
    sets of eight steps).  x_len = 1 is upstream's quirk: targets[0], whatever t_len."""
    rng = np.random.default_rng(41 + is_ctc)
    B = T = 60
    V = 8
    xl = np.arange(1, B + 1)
    tl = np.array([(1, 3, n)[n % 3] for n in xl])
    tg = np.stack([make_targets(rng, T, V, is_ctc, 0, doubles=0) for _ in xl])
    lp = emissions(rng, (B, T, V), quantised=False)
    got = run(lp, tg, xl, tl, 0, is_ctc, torch.float32)
    assert got[0, 0] == tg[0, 0]
    run(AR.quantised(rng, (B, T, V)), tg, xl, tl, 0, is_ctc, torch.float16)


# ---- the limit ------------------------------------------------------------------------------------------------------
def raw_call(lp, tg, xl, tl, Smax, blank, is_ctc, B=None):
    """e2e_ctc_align as it is -> (return code, out as numpy; prefilled with 7).  B = 0: no launch, pointers unused."""
    L = _lib.load()
    d = U.dev()
    if B == 0:
        ws = torch.empty(256, dtype=torch.uint8, device=d)
        return L.e2e_ctc_align(None, _lib.F32, 0, 0, 1, None, Smax, None, None, 0, 1, 4, Smax, blank, int(is_ctc), None, PAD,
                               ws.data_ptr(), ws.numel(), _lib.stream_ptr(d)), None
    lp, tg, xl, tl = lp.to(d), tg.to(d), xl.to(d), tl.to(d)
    B, T, V = lp.shape
    out = torch.full((B, T), 7, dtype=torch.long, device=d)
    n = L.e2e_ctc_align_workspace_bytes(B, T, V, Smax, int(is_ctc))
    ws = torch.empty(max(n, 256), dtype=torch.uint8, device=d)
    rc = L.e2e_ctc_align(lp.data_ptr(), _lib.dtype_code(lp.dtype), *lp.stride(), tg.data_ptr(), tg.stride(0), xl.data_ptr(),
                         tl.data_ptr(), B, T, V, Smax, blank, int(is_ctc), out.data_ptr(), PAD, ws.data_ptr(), ws.numel(),
                         _lib.stream_ptr(d))
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


@pytest.mark.parametrize("is_ctc", [True, False], ids=["ctc", "asg"])
def test_the_widest_accepted_targets_are_what_the_header_states(is_ctc):
    """Smax is raised with B = 0 (checked, nothing launched) until the call refuses it."""
    lo, hi = 1, 1 << 20                                            # accepted, refused
    assert raw_call(None, None, None, None, lo, 0, is_ctc, B=0)[0] == 0
    assert raw_call(None, None, None, None, hi, 0, is_ctc, B=0)[0] == UNSUPPORTED
    while hi - lo > 1:
        mid = (lo + hi) // 2
        rc = raw_call(None, None, None, None, mid, 0, is_ctc, B=0)[0]
        assert rc in (0, UNSUPPORTED)
        lo, hi = (mid, hi) if rc == 0 else (lo, mid)
    assert lo == (CTC_MAX_S if is_ctc else ASG_MAX_S)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "e2e_ctc.h")).read()
    assert "Smax <= %d" % CTC_MAX_S in header and "Smax <= %d" % ASG_MAX_S in header


def test_ctc_at_the_limit():
    """One utterance of 3172 labels (6345 cells: all of a workgroup's 160 KiB of LDS) in 3212 frames, next to a short one."""
    rng = np.random.default_rng(51)
    S, V = CTC_MAX_S, 29
    tg = np.stack([make_targets(rng, S, V, True, 0, doubles=0.005) for _ in range(2)])
    T = S + 40
    assert need(tg[0], True) <= T
    xl, tl = np.array([T, 50]), np.array([S, 20])
    run(emissions(rng, (2, T, V), False), tg, xl, tl, 0, True, torch.float32)


def test_asg_at_the_limit():
    """Targets 6345 wide (the widest), 2000 and 6 of them used, 2100 frames."""
    rng = np.random.default_rng(52)
    S, V, T = ASG_MAX_S, 29, 2100
    tg = np.stack([make_targets(rng, S, V, False, 0) for _ in range(2)])
    xl, tl = np.array([T, 33]), np.array([2000, 6])
    run(emissions(rng, (2, T, V), False), tg, xl, tl, 0, False, torch.float32)


@pytest.mark.parametrize("is_ctc", [True, False], ids=["ctc", "asg"])
def test_one_label_over_the_limit_is_refused_with_the_limit(is_ctc):
    limit = CTC_MAX_S if is_ctc else ASG_MAX_S
    lp = torch.log_softmax(torch.randn(1, 8, 5), -1)
    tg = torch.ones(1, limit + 1, dtype=torch.long)
    rc, out = raw_call(lp, tg, torch.tensor([8]), torch.tensor([2]), limit + 1, 0, is_ctc)
    msg = _lib.load().e2e_last_error().decode()
    assert rc == UNSUPPORTED and "Smax=%d" % (limit + 1) in msg and str(limit) in msg.replace("Smax=%d" % (limit + 1), ""), msg
    assert (out == 7).all()
    rc, out = raw_call(lp, tg[:, :limit].contiguous(), torch.tensor([8]), torch.tensor([2]), limit, 0, is_ctc)
    assert rc == 0 and (out != 7).all()                              # (the width alone is no obstacle)


# ---- blank and membership -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blank", [0, 2, 5])
def test_every_label_is_the_blank_or_a_target(blank):
    """V = 6, blank 0, 2 and V - 1.  An empty target: `blank` on every frame.  One frame and a target: targets[0] (upstream's
    quirk).  One frame and no target: blank."""
    rng = np.random.default_rng(60 + blank)
    V, T, W = 6, 40, 12
    xl = np.array([40, 33, 40, 1, 1, 17, 2])
    tl = np.array([12, 5, 0, 4, 0, 0, 1])
    tg = np.stack([make_targets(rng, W, V, True, blank) for _ in xl])
    for quantised in (False, True):
        lp = emissions(rng, (len(xl), T, V), quantised)
        got = run(lp, tg, xl, tl, blank, True, torch.float32)
        for b in range(len(xl)):
            assert set(got[b, :xl[b]].tolist()) <= {blank} | set(tg[b, :tl[b]].tolist()), b
        assert (got[2, :40] == blank).all() and (got[5, :17] == blank).all()
        assert got[3, 0] == tg[3, 0] and got[4, 0] == blank


def test_asg_labels_are_targets():
    """No blank in the ASG lattice (the argument is ignored): every label is one of the targets; one frame: targets[0]."""
    rng = np.random.default_rng(64)
    V, T, W = 6, 30, 10
    xl, tl = np.array([30, 21, 1, 10]), np.array([10, 4, 3, 10])
    tg = np.stack([make_targets(rng, W, V, False, 0) for _ in xl])
    lp = emissions(rng, (len(xl), T, V), False)
    for blank in (0, 3):
        got = run(lp, tg, xl, tl, blank, False, torch.float32)
        for b in range(len(xl)):
            assert set(got[b, :xl[b]].tolist()) <= set(tg[b, :tl[b]].tolist())
        assert got[2, 0] == tg[2, 0]


def test_word_segments_do_not_cut_an_utterance_without_targets():
    """blank 3, space 0: the frames of an utterance with an empty target are aligned to the blank, not to label 0 -- which
    here is the space, and where the model's arg-max is the space too every such frame would be a recognised boundary
    (min_word_length 0).  The plan is the restatement's on the oracle's alignment, and that utterance is one WHOLE segment."""
    import segmented_ref as SR
    from test_gpu_segmented import checker, table_of
    rng = np.random.default_rng(66)
    B, T, V, blank, space = 3, 30, 6, 3, 0
    x = torch.from_numpy(rng.standard_normal((B, T, V))).float()
    x[1, :, space] += 6.0                                            # the empty one: the model says "space" almost everywhere
    x[1, ::7, blank] += 12.0
    tg = torch.tensor([[1, 2, 0, 4, 5, 1, 0, 2], [0] * 8, [4, 0, 5, 0, 1, 2, 4, 0]])
    xl, tl = torch.tensor([30, 26, 30]), torch.tensor([8, 0, 7])
    got = table_of(x, tg, xl, tl, space, blank, 0)
    want, align, _ = checker(x, tg, xl, tl, space, blank, 0, with_losses=False)
    assert (align[1, :26] == blank).all()
    assert got == want
    assert [s for s in got if s[0] == 1] == [(1, 0, 26, SR.WHOLE, [])]


# ---- call shape -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [(True, 257), (False, 513)], ids=width_id)
def test_call_shapes_give_one_labelling(width):
    """A column stride of 2, time-major input, a gap between utterances, target rows further apart than they are wide with
    garbage beyond t_len, CPU tensors through get_alignment_3d, keep_on_device: the contiguous call's labelling every time."""
    from end2end_amd.utils.alignment import get_alignment_3d
    is_ctc, S = width
    rng = np.random.default_rng(70 + S)
    lp64, tg, xl, tl = width_batch(rng, S, is_ctc, False, 12, 0, False)
    base = run(lp64, tg, xl, tl, 0, is_ctc, torch.float32)
    d = U.dev()
    lp = torch.from_numpy(lp64).float().to(d)
    B, T, V = lp.shape
    nan = float("nan")
    every_other = torch.full((B, T, 2 * V), nan, device=d)[:, :, ::2]
    time_major = torch.full((T, B, V), nan, device=d).permute(1, 0, 2)
    gap = torch.full((B, T + 3, V), nan, device=d)[:, :T]
    both = torch.full((T, B + 1, 2 * V + 1), nan, device=d).permute(1, 0, 2)[:B, :, 1::2][:, :, :V]
    for name, view in (("sV=2", every_other), ("time-major", time_major), ("batch gap", gap), ("all three", both)):
        view.copy_(lp)
        assert not view.is_contiguous()
        assert np.array_equal(c_abi_align(view, tg, xl, tl, 0, is_ctc, PAD), base), name
    assert every_other.stride(2) == 2 and both.stride(2) == 2
    for garbage in (-5, V, 1 << 40):
        wide = U.padded_targets(tg, tl, S, garbage, row_stride=S + 5)
        assert wide.stride(0) == S + 5
        assert np.array_equal(c_abi_align(lp, wide, xl, tl, 0, is_ctc, PAD), base), garbage
    args = (torch.from_numpy(tg), torch.from_numpy(xl), torch.from_numpy(tl))
    cpu = get_alignment_3d(lp.cpu(), *args, is_ctc=is_ctc)
    assert cpu.device.type == "cpu" and np.array_equal(cpu.numpy(), base)
    kept = get_alignment_3d(every_other, *(a.to(d) for a in args), is_ctc=is_ctc, keep_on_device=True)
    assert kept.is_cuda and np.array_equal(kept.cpu().numpy(), base)


# ---- rows the header defines without a feasible walk: against the oracle only -----------------------------------------
def neighbours(rng, V, T, W, is_ctc):
    tg = np.stack([make_targets(rng, W, V, is_ctc, 0) for _ in range(3)])
    return tg, np.array([T, T, T - 1]), np.array([min(W, T // 3), 1, min(W, T // 3)])


def test_asg_with_fewer_frames_than_labels():
    """Oracle only (there is no legal walk): not an error upstream; the back-trace walks cells outside the band."""
    rng = np.random.default_rng(80)
    V, T, W = 7, 20, 30
    tg, xl, tl = neighbours(rng, V, T, W, False)
    xl[1], tl[1] = 9, 30
    lp = emissions(rng, (3, T, V), False)
    got = c_abi_align(torch.from_numpy(lp).float(), tg, xl, tl, 0, False, PAD)
    check(got, lp, tg, xl, tl, 0, False)
    wide = np.stack([make_targets(rng, 600, V, False, 0) for _ in range(3)])         # and in the wide sweep
    xl, tl = np.array([620, 300, 2]), np.array([600, 600, 550])
    lp = emissions(rng, (3, 620, V), True)
    check(c_abi_align(torch.from_numpy(lp).float(), wide, xl, tl, 0, False, PAD), lp, wide, xl, tl, 0, False)


def test_ctc_with_fewer_frames_than_the_labelling_needs():
    """Oracle only: the same walk over -inf cells as upstream's, in both sweeps."""
    rng = np.random.default_rng(81)
    V = 7
    tg = np.stack([make_targets(rng, 300, V, True, 0, doubles=0.2) for _ in range(4)])
    xl, tl = np.array([300, 299, 40, 310]), np.array([300, 300, 90, 300])
    assert need(tg[3], True) > 310
    lp = emissions(rng, (4, 310, V), False)
    check(c_abi_align(torch.from_numpy(lp).float(), tg, xl, tl, 0, True, PAD), lp, tg, xl, tl, 0, True)


def test_asg_without_targets_is_all_zeros():
    """Oracle only: t_len = 0 has no lattice; the row is zeros (upstream would index targets[0])."""
    rng = np.random.default_rng(82)
    V, T, W = 7, 20, 6
    tg, xl, tl = neighbours(rng, V, T, W, False)
    tl[1] = 0
    lp = emissions(rng, (3, T, V), False)
    got = c_abi_align(torch.from_numpy(lp).float(), tg, xl, tl, 3, False, PAD)
    check(got, lp, tg, xl, tl, 3, False)
    assert (got[1, :T] == 0).all()


def test_minus_infinity_on_the_only_walk():
    """A tight CTC row (one walk) with a -inf emission on it, and a loose row one of whose labels is -inf on every frame:
    every score is -inf, the comparisons are all ties.  Oracle only."""
    rng = np.random.default_rng(83)
    V, T, W = 7, 24, 24
    tg = np.stack([make_targets(rng, W, V, True, 0, doubles=0) for _ in range(3)])
    xl, tl = np.array([24, 24, 20]), np.array([24, 6, 5])
    lp = emissions(rng, (3, T, V), False)
    lp[0, 9, tg[0, 9]] = -np.inf
    lp[1, :, tg[1, 2]] = -np.inf
    got = c_abi_align(torch.from_numpy(lp).float(), tg, xl, tl, 0, True, PAD)
    check(got, lp, tg, xl, tl, 0, True, reference=False)
    AR.check_utterance(lp[2], got[2], tg[2, :5], 20, True, 0)           # (the neighbour)


@pytest.mark.parametrize("is_ctc", [True, False], ids=["ctc", "asg"])
def test_no_frames_and_a_target_outside_the_alphabet_are_rows_of_padding(is_ctc):
    """x_len = 0 and a target == V: a row of pad_value each, the neighbours as the oracle has them.  (The oracle does not
    look targets up in a range: it gets that row without its targets and the row is compared with the padding.)"""
    rng = np.random.default_rng(84 + is_ctc)
    V, T, W = 7, 20, 6
    tg = np.stack([make_targets(rng, W, V, is_ctc, 0) for _ in range(5)])
    xl, tl = np.array([20, 0, 19, 20, 12]), np.array([6, 3, 5, 6, 2])
    tg[3, 4] = V
    lp = emissions(rng, (5, T, V), False)
    got = c_abi_align(torch.from_numpy(lp).float(), tg, xl, tl, 0, is_ctc, PAD)
    assert (got[1] == PAD).all() and (got[3] == PAD).all()
    keep = [0, 1, 2, 4]
    check(got[keep], lp[keep], tg[keep], xl[keep], tl[keep], 0, is_ctc)


# ---- AlignedTargetsLoss on wide lattices ----------------------------------------------------------------------------
@pytest.mark.parametrize("width", [(True, 300), (False, 600)], ids=width_id)
def test_aligned_targets_loss_on_a_wide_lattice(width):
    """The module's value is the NLL of the oracle's alignment per frame, computed in f64 (tolerance: the module's own in
    tests/test_gpu_noblank.py, rtol 1e-6 + atol 1e-6)."""
    from end2end_amd import AlignedTargetsLoss
    is_ctc, S = width
    rng = np.random.default_rng(90 + S)
    lp64, tg, xl, tl = width_batch(rng, S, is_ctc, False, 12, 0, False)
    d = U.dev()
    loss = AlignedTargetsLoss(is_ctc)(torch.from_numpy(lp64).to(d), torch.from_numpy(tg).to(d), torch.from_numpy(xl).to(d),
                                     torch.from_numpy(tl).to(d))
    a = O.ctc_align(lp64, tg, xl, tl, 0, is_ctc, n_threads=16)
    want = np.array([-lp64[b, np.arange(xl[b]), a[b, :xl[b]]].sum() / xl[b] for b in range(len(xl))])
    assert loss.device.type == "cuda"
    np.testing.assert_allclose(loss.cpu().numpy(), want, rtol=1e-6, atol=1e-6)
