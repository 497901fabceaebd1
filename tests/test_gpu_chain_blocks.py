"""-m gpu: the lean halo chain kernel (end2end_amd/csrc/ctc_loss_fast_h1.hip) at the seams of its block structure, against the
f64 oracle.

Every case runs with ALGO_FAST (a flagged utterance would come back as NaN), is held to the default tolerances -- losses 6e-7
relative, gradients 2e-6 + 1e-4 |g| --, asserts flag word 0 for every utterance (e2e_debug_fast_state) and asserts that the
call's route is the fast path with the lean halo chains (rule 4 of launch_fast_ppl's list).  The kernel is selected by the
WIDTH of the targets tensor, not by the lengths in it, so short utterances sit behind a wide tensor with short t_len.
Logits are unit-variance normal unless stated; targets have no adjacent repeats unless the case is about repeats, so that a
target of S labels needs S frames.

The cases (B <= 8 each):
  * T in 1, 7, 8, 9, 15, 16, 17, 33, 129, 136, 137, 144, 145, 152, 153, 160, 273, targets tensor 128 wide, target lengths
    {1, T/4, T/3, min(T/2, 128)} (at least 1): first / last partial blocks (T = 0, 1, 7 mod 8), checkpoint rows at the ends
    (15, 16, 17, 33), the eight-at-a-time loop (from T = 137: M = (T-1)>>3 >= 17) with both parities of M (137..144 against
    145..152: beta's checkpoint parity), several rounds of eight plus a tail (273);
  * x_len ragged inside one batch, {T, T-1, T-7, T-8, ceil(T/2)}, for T = 153 and T = 273 (target length 60);
  * t_len 1, 55, 56, 57, 111, 112, 113 (T = 273, tensor 128 wide) and 167, 168, 200 (T = 417, tensor 223 wide): 56 is the
    boundary of a wave's own lanes, 111 / 112 one or two waves per direction;
  * repeated labels across the wave seam, two waves per direction (T = 417, tensor 223 wide, 150 labels): t[110] == t[111],
    t[111] == t[112], and four equal labels over 110..113;
  * targets tensor 64 wide, B = 4 (the two-pairs-per-lane instance of the same kernel): t_len 1, 32, 63, 64 at T = 153;
  * alphabets V = 5, 29, 33, 78 (the producers' brackets of 2, 4, 6, 12 column groups) with blank 0 and blank V-1, and V = 16
    with blank 8, at T = 153 (target lengths 1, 38, 51, 76).  78 columns are the most this kernel takes: its LDS layout needs
    60.4 KB + 1280 (V + 1) bytes of the CU's 160 KB.  V = 96 runs too, held to the same tolerances and flag words, but the
    dispatch gives it to the halo chains of ctc_loss_fast.hip (rule 5), which the case asserts instead;
  * input forms at T = 153, V = 29: log-probabilities; bf16 and f16 logits (against the oracle on the rounded logits, at the
    tolerances tests/test_gpu_regimes.py holds 16-bit input to: losses 1e-4 relative + 2e-5, gradients 2 eps relative + 2e-6,
    eps = 2^-7 / 2^-10); a time-major strided view.
The commit before the chain waves' hand-off words moved to fixed LDS offsets returns flag 0 for every utterance of this list
too (run once against it), so no case had to take other lengths.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import oracle_lib as O
import gpu_util as U
from end2end_amd import _lib

pytestmark = pytest.mark.gpu

LOSS_RTOL = 6e-7
GRAD_RTOL, GRAD_ATOL = 1e-4, 2e-6


def log_softmax(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max(axis=-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


def fast_flags(keep, B, T, V):
    L = _lib.load()
    flags, logz = (ctypes.c_int * B)(), (ctypes.c_double * (2 * B))()
    assert L.e2e_debug_fast_state(keep["workspace"].data_ptr(), B, T, V, keep["Smax"], flags, logz) == 0
    return list(flags)


def no_repeat_targets(rng, B, S, labels):
    """(B, S) labels drawn from `labels`, no two adjacent ones equal"""
    labels = np.asarray(labels)
    k = rng.integers(0, len(labels), size=(B, S))
    step = rng.integers(1, len(labels), size=(B, S))
    for j in range(1, S):
        same = k[:, j] == k[:, j - 1]
        k[same, j] = (k[same, j] + step[same, j]) % len(labels)
    return labels[k]


def check(x, tg, xl, tl, blank=0, logprobs=False, pairs=4, x_dev=None, tol=None, rule=4):
    """x: (B, T, V) f64/f32 array, what the oracle sees; x_dev: the tensor the call gets (default: x as contiguous f32).
    tol: (loss rtol, loss atol, grad rtol, grad atol), default the f32 tolerances."""
    B, T, V = x.shape
    xl, tl = np.asarray(xl), np.asarray(tl)
    need = tl + np.array([int((tg[b, 1:tl[b]] == tg[b, :tl[b] - 1]).sum()) for b in range(B)])
    assert (need <= xl).all(), "infeasible case: %s frames for %s" % (xl.tolist(), need.tolist())
    lp = np.asarray(x, dtype=np.float64) if logprobs else log_softmax(x)
    l_o, g_o = O.ctc_loss(lp, tg, xl, tl, blank)
    if not logprobs:
        for b in range(B):
            g_o[b, xl[b]:] = 0.0
    if x_dev is None:
        x_dev = torch.from_numpy(np.asarray(x, dtype=np.float32))
    keep = {}
    la, ga = U.c_abi_loss(x_dev, tg, xl, tl, blank, logprobs, _lib.ALGO_FAST, keep=keep)
    route = keep["route"]
    flags = fast_flags(keep, B, T, V)
    with np.errstate(invalid="ignore", divide="ignore"):
        print("route", route, "flags", flags, "max |dloss|/loss %.3g" % np.max(np.abs(la - l_o) / np.abs(l_o)),
              "max |dgrad| %.3g" % np.max(np.abs(ga - g_o)))
    assert route // 1000 == 2 and route % 10 == rule and route % 100 // 10 == pairs, "route %d: not chain rule %d" % (route, rule)
    assert flags == [0] * B, "flag words %s" % flags
    lr, la_, gr, ga_ = tol or (LOSS_RTOL, 0.0, GRAD_RTOL, GRAD_ATOL)
    U.assert_same(la, l_o, lr, la_, "losses")
    U.assert_same(ga, g_o, gr, ga_, "grads")


def case(seed, T, width, tl, V=29, blank=0, xl=None):
    rng = np.random.default_rng(seed)
    B = len(tl)
    x = rng.standard_normal((B, T, V)).astype(np.float32)
    tg = no_repeat_targets(rng, B, width, [v for v in range(V) if v != blank])
    return x, tg, np.full(B, T) if xl is None else np.asarray(xl), np.asarray(tl)


@pytest.mark.parametrize("T", [1, 7, 8, 9, 15, 16, 17, 33, 129, 136, 137, 144, 145, 152, 153, 160, 273])
def test_frame_counts_at_the_block_seams(T):
    tl = sorted({1, max(T // 4, 1), max(T // 3, 1), min(max(T // 2, 1), 128)})
    check(*case(1000 + T, T, 128, tl))


@pytest.mark.parametrize("T", [153, 273])
def test_ragged_frame_counts_in_one_batch(T):
    check(*case(2000 + T, T, 128, [60] * 5, xl=[T, T - 1, T - 7, T - 8, (T + 1) // 2]))


@pytest.mark.parametrize("T,width,tl", [(273, 128, (1, 55, 56, 57, 111, 112, 113)), (417, 223, (167, 168, 200))],
                         ids=["T273_w128", "T417_w223"])
def test_target_lengths_at_the_lane_and_wave_seams(T, width, tl):
    check(*case(3000 + T, T, width, tl))


def test_repeated_labels_across_the_wave_seam():
    x, tg, xl, tl = case(4000, 417, 223, (150, 150, 150))
    others = lambda *v: next(c for c in range(1, 29) if c not in v)     # noqa: E731
    tg[0, 111] = tg[0, 110]
    tg[0, 112] = others(tg[0, 111], tg[0, 113])
    tg[1, 112] = tg[1, 111]
    tg[1, 113] = others(tg[1, 112], tg[1, 114])
    tg[2, 110:114] = tg[2, 110]
    tg[2, 109] = others(tg[2, 108], tg[2, 110])
    tg[2, 114] = others(tg[2, 113], tg[2, 115])
    rep = [(tg[b, 1:150] == tg[b, :149]).nonzero()[0].tolist() for b in range(3)]
    assert rep == [[110], [111], [110, 111, 112]], rep
    check(x, tg, xl, tl)


def test_targets_tensor_of_64_columns():
    check(*case(5000, 153, 64, (1, 32, 63, 64)), pairs=2)


@pytest.mark.parametrize("V,blank", [(5, 0), (5, 4), (29, 0), (29, 28), (33, 0), (33, 32), (78, 0), (78, 77), (96, 0), (96, 95),
                                      (16, 8)])
def test_alphabet_brackets_and_blank_positions(V, blank):
    check(*case(6000 + 100 * V + blank, 153, 128, (1, 38, 51, 76), V=V, blank=blank), blank=blank, rule=4 if V <= 78 else 5)


@functools.lru_cache(maxsize=None)
def base_case():
    return case(7000, 153, 128, (1, 38, 51, 76))


def test_log_probabilities():
    x, tg, xl, tl = base_case()
    lp = log_softmax(x).astype(np.float32)
    check(lp, tg, xl, tl, logprobs=True)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_sixteen_bit_logits(dtype):
    x, tg, xl, tl = base_case()
    x16 = torch.from_numpy(x).to(dtype)
    eps = 2.0 ** -7 if dtype == torch.bfloat16 else 2.0 ** -10
    check(x16.double().numpy(), tg, xl, tl, x_dev=x16, tol=(1e-4, 2e-5, 2 * eps, 2e-6))


def test_time_major_strided_view():
    x, tg, xl, tl = base_case()
    xt = torch.from_numpy(x).permute(1, 0, 2).contiguous().permute(1, 0, 2)      # (B, T, V) view of a (T, B, V) buffer
    assert xt.stride() == (29, 4 * 29, 1)
    check(x, tg, xl, tl, x_dev=xt)
