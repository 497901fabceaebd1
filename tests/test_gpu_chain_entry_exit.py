"""-m gpu: the lean halo chain kernel (end2end_amd/csrc/ctc_loss_fast_h1.hip) around and beside its chain steps -- the first
rows and targets a workgroup reads at kernel entry, the producers' stream, and the lanes that write log Z at the exit --
against the f64 oracle and, bit for bit, against a recording of what the kernel computed when this file was written.  It is
the net under any change to those parts: loads issued before the utterance's lengths are known (clamped rows and targets,
rows guessed for a full-length utterance), a leaner producer loop, logarithms moved to other waves.
tests/test_gpu_chain_blocks.py has the block seams, wave seams, brackets, dtypes and strides; nothing of it is repeated here.

Every case has B <= 8, T <= 273 and a targets tensor 128 wide, and asserts that the call's route is the fast path with the lean
halo chains (rule 4).  Tolerances are the project's defaults: losses 6e-7 relative, gradients 2e-6 + 1e-4 |g|.  Log Z of either
side (e2e_debug_fast_state) is held to -loss of the oracle at the losses' tolerance.

  entry, rows (what goes wrong if the producers' first blocks are asked for as if the utterance had T frames):
    * T = 153 with x_len = 153, 152, 145, 144, 137, 16, 8, 1 in one batch, and the same batch reversed (the last utterance's
      rows then end where the logits end); T = 9 and T = 17 with x_len = T, 1;
  entry, targets (what goes wrong if they are asked for with indices clamped to the tensor's width):
    * t_len = 0, 1, 2, 127, 128 with every entry behind t_len set to -1, V, 2^40 or the blank: flag word 0;
    * a blank inside t_len raises flag 2 (ALGO_AUTO: every utterance equals the oracle), a bad x_len / t_len raises flag 1
      and nothing else (ALGO_AUTO: those utterances come back NaN, the others equal the oracle);
  producers:
    * V = 9, 16, 17, 24, 25, 29, 32 with the blank at 0, 7, 8, V - 1 (partly dead column groups; the blank in every group and
      in the last lane of one); every second column of a wider buffer; a log-probability of -inf on a symbol outside the targets;
    * one frame with a column at max - 68.5, max - 69.5, max - 78.5 (logits), and the same three as log-probabilities: flag
      words exactly 0, 64, 64 | 256, and under ALGO_AUTO the outputs equal the oracle;
    (flag words are read after an ALGO_FAST call and compared whole: 0, 0, 64, 64 | 256 exactly.  After an ALGO_AUTO call the
    word of a flagged utterance also carries what the flagged launch noted while it redid it -- a column at max - 69.5 reads
    26688 = 64 + 2048 + 8192 + 16384 --, so that run is for the outputs and its words are compared in the chain kernel's bits,
    1, 2, 4, 64, 128, 256.  Behind a blank inside t_len the segment kernel adds its bits 8 / 32 under either algorithm -- the
    words read 10 and 42 --: there every bit but the segment kernel's three must be as stated)
    * one NaN and one +inf logit: flag bit 4, and 4 | 64 | 256; under ALGO_FAST loss and whole gradient NaN as the oracle has
      them, under ALGO_AUTO the loss, the frame that holds the value, and the other utterance untouched;
  exit:
    * log Z from both sides and the losses with one and two waves per direction (t_len 100, 120), for T = 1 and for t_len = 0;
  bit identity with the recording:
    * tests/golden/chain_entry_parent.npz (written by tests/golden/make_chain_entry_golden.py on the GPU, from the library of
      the commit before this file, whose kernel is the one in the tree) holds, for every unflagged case, the losses, log Z,
      flag words and a SHA-256 of the gradient's bytes under ALGO_FAST, and the whole gradient of three cases.  Flagged cases
      are not in it: their f64 redo sums with atomics.
"""
import ctypes
import functools
import hashlib
import os

import numpy as np
import pytest
import torch

import oracle_lib as O
import gpu_util as U
from end2end_amd import _lib

pytestmark = pytest.mark.gpu

LOSS_RTOL = 6e-7
GRAD_RTOL, GRAD_ATOL = 1e-4, 2e-6
WIDTH = 128
CHAIN_BITS = 1 | 2 | 4 | 64 | 128 | 256          # the flag bits the chain kernel raises
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chain_entry_parent.npz")
FULL_GRADS = ("ragged_T153", "T17_full_and_one_frame", "exit_one_and_two_waves")     # cases whose whole gradient is in the fixture


def log_softmax(x):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        m = x.max(axis=-1, keepdims=True)
        return x - m - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


def no_repeat_targets(rng, B, S, labels):
    labels = np.asarray(labels)
    k = rng.integers(0, len(labels), size=(B, S))
    step = rng.integers(1, len(labels), size=(B, S))
    for j in range(1, S):
        same = k[:, j] == k[:, j - 1]
        k[same, j] = (k[same, j] + step[same, j]) % len(labels)
    return labels[k]


def base(seed, T, tl, V=29, blank=0, xl=None, exclude=()):
    """unit-variance logits, targets without adjacent repeats (a target of S labels needs S frames) and without `exclude`"""
    rng = np.random.default_rng(seed)
    B = len(tl)
    x = rng.standard_normal((B, T, V)).astype(np.float32)
    tg = no_repeat_targets(rng, B, WIDTH, [v for v in range(V) if v != blank and v not in exclude])
    return dict(x=x, tg=tg, xl=np.full(B, T) if xl is None else np.asarray(xl), tl=np.asarray(tl), blank=blank, logprobs=False,
                padding=-1, every_second_column=False)


RAGGED_XL, RAGGED_TL = [153, 152, 145, 144, 137, 16, 8, 1], [40, 39, 38, 37, 36, 5, 3, 1]


def _ragged(rev):
    return base(8100 + rev, 153, RAGGED_TL[::-1] if rev else RAGGED_TL, xl=RAGGED_XL[::-1] if rev else RAGGED_XL)


def _garbage():
    c = base(8200, 273, [0, 1, 2, 127, 128])
    c["padding"] = [-1, 29, 2 ** 40, 0, -1]          # what every entry behind t_len[b] holds: -1, V, 2^40, the blank
    return c


def _alphabet(V, blank):
    return base(8300 + 100 * V + blank, 153, (1, 38, 51, 76), V=V, blank=blank)


def _strided():
    c = base(8400, 153, (1, 38, 51, 76))
    c["every_second_column"] = True
    return c


def _neginf_logprob():
    c = base(8500, 153, (1, 38, 51, 76), exclude=(11,))
    lp = log_softmax(c["x"]).astype(np.float32)
    lp[:, ::3, 11] = -np.inf
    c.update(x=lp, logprobs=True)
    return c


ALPHABETS = [(V, bl) for V in (9, 16, 17, 24, 25, 29, 32) for bl in sorted({0, 7, 8, V - 1}) if bl < V]

# name -> builder; every one of these runs unflagged under ALGO_FAST and is in the fixture
UNFLAGGED = {
    "ragged_T153": lambda: _ragged(0),
    "ragged_T153_reversed": lambda: _ragged(1),
    "T9_full_and_one_frame": lambda: base(8109, 9, [3, 1], xl=[9, 1]),
    "T17_full_and_one_frame": lambda: base(8117, 17, [5, 1], xl=[17, 1]),
    "targets_garbage_behind_t_len": _garbage,
    "every_second_column": _strided,
    "neginf_logprob_outside_targets": _neginf_logprob,
    "exit_one_and_two_waves": lambda: base(8600, 273, [100, 120]),
    "exit_T1": lambda: base(8601, 1, [1, 0]),
    "exit_t_len_0": lambda: base(8602, 153, [0, 0, 40]),
}
for _V, _bl in ALPHABETS:
    UNFLAGGED["V%d_blank%d" % (_V, _bl)] = functools.partial(_alphabet, _V, _bl)


def device_logits(c):
    x = torch.from_numpy(np.asarray(c["x"], dtype=np.float32))
    if c["every_second_column"]:
        wide = torch.zeros(x.shape[0], x.shape[1], 2 * x.shape[2])
        wide[:, :, ::2] = x
        x = wide[:, :, ::2]
        assert x.stride(2) == 2
    return x


def run(c, algo, raw_targets=False):
    """one call; returns losses, grads, flag words and log Z (B, 2).  raw_targets: the call gets c["tg"] as it is (WIDTH columns)
    instead of a tensor padded behind t_len, which cannot be built for a t_len outside the tensor"""
    B, T, V = c["x"].shape
    keep = {}
    pad = {} if raw_targets else dict(width=WIDTH, padding=c["padding"])
    la, ga = U.c_abi_loss(device_logits(c), c["tg"], c["xl"], c["tl"], c["blank"], c["logprobs"], algo, keep=keep, **pad)
    assert keep["Smax"] == WIDTH
    L = _lib.load()
    flags, logz = (ctypes.c_int * B)(), (ctypes.c_double * (2 * B))()
    assert L.e2e_debug_fast_state(keep["workspace"].data_ptr(), B, T, V, keep["Smax"], flags, logz) == 0
    route = keep["route"]
    assert route // 1000 == 2 and route % 10 == 4 and route % 100 // 10 == 4, "route %d: not the lean halo chains" % route
    return la, ga, list(flags), np.array(logz[:]).reshape(B, 2)


def oracle(c):
    lp = np.asarray(c["x"], dtype=np.float64) if c["logprobs"] else log_softmax(c["x"])
    l_o, g_o = O.ctc_loss(lp, c["tg"], c["xl"], c["tl"], c["blank"])
    if not c["logprobs"]:
        for b in range(len(l_o)):
            if np.isfinite(l_o[b]):
                g_o[b, c["xl"][b]:] = 0.0
    return l_o, g_o


@functools.lru_cache(maxsize=None)
def unflagged(name):
    c = UNFLAGGED[name]()
    return c, run(c, _lib.ALGO_FAST), oracle(c)


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(GOLDEN)


def report(la, ga, flags, l_o, g_o):
    with np.errstate(invalid="ignore", divide="ignore"):
        print("flags", flags, "max |dloss|/|loss| %.3g" % np.nanmax(np.abs(la - l_o) / np.abs(l_o)), "max |dgrad| %.3g" % np.nanmax(np.abs(ga - g_o)))


@pytest.mark.parametrize("name", list(UNFLAGGED))
def test_unflagged_case_equals_the_oracle(name):
    c, (la, ga, flags, logz), (l_o, g_o) = unflagged(name)
    assert np.isfinite(l_o).all(), "infeasible case"
    report(la, ga, flags, l_o, g_o)
    assert flags == [0] * len(la), "flag words %s" % flags
    U.assert_same(la, l_o, LOSS_RTOL, 0.0, "losses")
    U.assert_same(ga, g_o, GRAD_RTOL, GRAD_ATOL, "grads")
    for side in (0, 1):
        U.assert_same(logz[:, side], -l_o, LOSS_RTOL, 0.0, "log Z, side %d" % side)


@pytest.mark.parametrize("name", list(UNFLAGGED))
def test_unflagged_case_equals_the_recording_bit_for_bit(name):
    _, (la, ga, flags, logz), _ = unflagged(name)
    g = golden()
    assert np.array_equal(np.asarray(flags), g[name + "/flags"])
    assert np.array_equal(la.view(np.uint32), g[name + "/losses"].view(np.uint32)), "losses"
    assert np.array_equal(logz.view(np.uint64), g[name + "/logz"].view(np.uint64)), "log Z"
    if name in FULL_GRADS:
        want = g[name + "/grads"]
        diff = np.flatnonzero(ga.view(np.uint32).ravel() != want.view(np.uint32).ravel())
        assert diff.size == 0, "gradient differs at %d elements, first %s" % (diff.size, np.unravel_index(diff[0], ga.shape))
    assert hashlib.sha256(np.ascontiguousarray(ga).tobytes()).hexdigest() == str(g[name + "/grads_sha256"]), "gradient"


def test_fixture_holds_exactly_the_unflagged_cases():
    names = {k.split("/")[0] for k in golden().files}
    assert names == set(UNFLAGGED)
    assert os.path.getsize(GOLDEN) < 1 << 20


SEGMENT_BITS = 8 | 16 | 32                       # ... and the ones the segment kernel raises


def check_flagged(c, fast_words, segment_bits=0):
    """ALGO_FAST for the flag words -- exactly `fast_words`, but for `segment_bits` on the flagged utterances --, ALGO_AUTO for the
    outputs (after an ALGO_AUTO call a flagged word also carries what the flagged launch noted while it redid the utterance)"""
    flags = run(c, _lib.ALGO_FAST)[2]
    print("ALGO_FAST flag words", flags)
    assert [f & ~(segment_bits if w else 0) for f, w in zip(flags, fast_words)] == fast_words, "flag words %s" % flags
    la, ga, auto_flags, _ = run(c, _lib.ALGO_AUTO)
    l_o, g_o = oracle(c)
    report(la, ga, auto_flags, l_o, g_o)
    assert [f & CHAIN_BITS for f in auto_flags] == [w & CHAIN_BITS for w in fast_words], "flag words after ALGO_AUTO %s" % auto_flags
    U.assert_same(la, l_o, LOSS_RTOL, 0.0, "losses")
    U.assert_same(ga, g_o, GRAD_RTOL, GRAD_ATOL, "grads")


def test_a_blank_inside_t_len_raises_flag_2():
    c = base(8700, 153, (1, 38, 51, 76))
    c["tg"][1, 20] = 0
    c["tg"][3, 75] = 0
    # (the segment kernel then runs over a lattice the chains gave up and adds its own range / self-check bits: the words read
    # 10 and 42; the exact kernel redoes the utterances: a blank among the targets has a loss, the oracle's)
    check_flagged(c, [0, 2, 0, 2], segment_bits=SEGMENT_BITS)


def test_bad_lengths_raise_flag_1_and_nothing_else():
    c = base(8701, 153, (40, 40, 40, 40, 40))
    c["xl"] = np.array([153, 0, 154, 153, 153])
    c["tl"] = np.array([40, 40, 40, 129, -1])
    la, ga, flags, _ = run(c, _lib.ALGO_AUTO, raw_targets=True)
    assert flags == [0, 1, 1, 1, 1], flags
    l_o, g_o = oracle(dict(c, xl=np.full(5, 153), tl=np.full(5, 40)))      # (asked for utterance 0: the others come back NaN)
    l_o[1:], g_o[1:] = np.nan, np.nan
    U.assert_same(la, l_o, LOSS_RTOL, 0.0, "losses")
    U.assert_same(ga, g_o, GRAD_RTOL, GRAD_ATOL, "grads")


def threshold_case(logprobs):
    """utterance b has, in frame 70, column 11 (not a target) at the row's maximum - (nothing, 68.5, 69.5, 78.5)"""
    c = base(8800 + logprobs, 153, (38, 38, 38, 38), exclude=(11,))
    x = log_softmax(c["x"]).astype(np.float32) if logprobs else c["x"]
    for b, below in ((1, 68.5), (2, 69.5), (3, 78.5)):
        x[b, 70, 11] = np.float32(-below) if logprobs else x[b, 70].max() - np.float32(below)
    c.update(x=x, logprobs=bool(logprobs))
    return c


@pytest.mark.parametrize("logprobs", [0, 1], ids=["logits", "logprobs"])
def test_small_probabilities_raise_flags_64_and_256_at_their_thresholds(logprobs):
    check_flagged(threshold_case(logprobs), [0, 0, 64, 64 | 256])


@pytest.mark.parametrize("value,chain_bits", [(float("nan"), 4), (float("inf"), 4 | 64 | 256)], ids=["nan", "plus_inf"])
def test_a_nan_or_infinite_logit_poisons_its_utterance_only(value, chain_bits):
    """NaN: the row's probabilities are NaN, so is Z (bit 4); no comparison of the smallest log-probability holds.  +inf: the
    row's maximum is +inf, every other column lies -inf below it (bits 64 and 256) and the column itself gives inf - inf (bit 4).
    The oracle has NaN for the utterance's loss and for its whole gradient.  ALGO_FAST returns exactly that.  ALGO_AUTO's
    redo leaves part of that gradient finite (3 069 of its 4 437 elements are NaN), so after ALGO_AUTO the utterance's
    gradient is held to NaN in the frame that has the value and the rest of the outputs to the oracle."""
    c = base(8900, 153, (38, 38))
    c["x"][1, 70, 5] = value
    l_o, g_o = oracle(c)
    assert np.isnan(l_o[1]) and np.isnan(g_o[1]).all() and np.isfinite(l_o[0])
    la, ga, flags, _ = run(c, _lib.ALGO_FAST)
    print("ALGO_FAST flag words", flags)
    assert flags[0] == 0 and flags[1] & ~SEGMENT_BITS == chain_bits, "flag words %s" % flags
    U.assert_same(la, l_o, LOSS_RTOL, 0.0, "losses")
    U.assert_same(ga, g_o, GRAD_RTOL, GRAD_ATOL, "grads")
    la, ga, flags, _ = run(c, _lib.ALGO_AUTO)
    assert flags[0] == 0 and flags[1] & CHAIN_BITS == chain_bits, "flag words after ALGO_AUTO %s" % flags
    U.assert_same(la, l_o, LOSS_RTOL, 0.0, "losses")
    U.assert_same(ga[0], g_o[0], GRAD_RTOL, GRAD_ATOL, "grads of the untouched utterance")
    assert np.isnan(ga[1, 70]).all(), "the frame that holds the value"
