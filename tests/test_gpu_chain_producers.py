"""-m gpu: the producers of the lean halo chain kernel (hx_prep_wave, end2end_amd/csrc/ctc_loss_fast_h1.hip) -- the waves that
read the logits, take the softmax of every frame, fill the f64 probability ring and the probability table (ytab), and vote
on flag bits 64 / 256 -- against the f64 oracle and, bit for bit, against a recording of what the kernel computed before the
producers' instruction stream was cut (tests/golden/chain_producers_parent.npz, written by
tests/golden/make_chain_producers_golden.py from the library of the commit before this file).  It is the net under any
change to the producers' loop: a body without row tests for blocks whose eight rows are all live, 32-bit addressing,
another way to track the smallest log-probability.

tests/test_gpu_chain_blocks.py has the chain waves' seams and tests/test_gpu_chain_entry_exit.py the kernel's entry and exit;
the shapes here are the smallest at which a producer can go wrong.  Every case has B <= 8 and T <= 200 and asserts that the
call's route is the fast path with the lean halo chains (rule 4): the two-pairs instance behind a targets tensor 64 wide, the
four-pairs instance behind one 128 wide.

  frames     T in 1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 71, 72, 73, 129, 200 (a block is 8 frames, a segment 16, the ring eight
             blocks = 64 frames: from the ninth block on a producer waits for the readers), target lengths 1, T/4, T/2 and
             T + 3 (capped at the tensor's width): up to T = 63 the last utterance has more labels than frames, no alignment,
             and must carry flag 4;
             x_len ragged inside batches of T = 17, 73 and 200: one below, at and one above multiples of 8 (the only blocks
             with dead rows are an utterance's last ones for alpha and first one for beta; all others take the steady body);
  alphabets  V in 2, 7, 8, 9, 16, 17, 24, 25, 29, 32, 33, 48, 49, 64, 65, 78, 96: both ends of every bracket of column groups
             (2, 4, 6, 8, 12 groups of 8 columns) and of the groups whose columns are tested against V.  78 columns are the most
             this kernel takes (its LDS layout: 60.4 KB + 1280 (V + 1) bytes of 160 KB); V = 96 runs too and is held to the
             same oracle, but the dispatch gives it to the single-wave chains of ctc_loss_fast.hip (rule 6), which the case asserts;
  blank      at 0, at V - 1 and at 8 (the second column group);
  inputs     f32 contiguous; f32 with rows 40 apart (padded sT) and with every second column (sV = 2): the strided forms;
             f16 and bf16 (against the oracle on the rounded logits at the tolerances tests/test_gpu_chain_blocks.py holds 16-bit
             input to -- the gradient comes back in 16 bits: losses 1e-4 relative + 2e-5, gradients 2 eps relative + 2e-6, eps =
             2^-7 / 2^-10); log-probabilities; -inf in live columns, as logits and as log-probabilities (on symbols outside the
             targets, and on a target's symbol in one utterance, which then has no alignment); whole rows scaled by 30.
             (A view whose T * sT exceeds 2^31 elements cannot be had without allocating it: the host's choice of the 32-bit
             addressing is tested on the CPU, tests/test_chain_producers_host_cpu.py.)

What is asserted.  Under ALGO_FAST the flag words: the chain kernel's bits (1, 2, 4, 64, 128, 256) must be exactly
  4        iff the oracle finds no alignment (loss not finite),
  64, 256  iff the smallest float32(x - max of the row) over live frames and finite entries is below -69, -78 (for
           log-probabilities: the smallest finite x itself) -- the producers' rule, restated in numpy;
utterances whose word is 0 equal the oracle in loss and gradient at the project's default tolerances (losses 6e-7 relative,
gradients 2e-6 + 1e-4 |g|); utterances with a word are compared after an ALGO_AUTO call, every utterance of which equals the
oracle.  Against the recording: losses, gradients (a SHA-256 per case, the whole gradient of three cases) and flag words
under ALGO_FAST, bit for bit, for every utterance whose flag word is 0, and the flag words of all.  (A flagged utterance's
outputs under ALGO_FAST are not the product's: the flagged launch replaces them.  Its flag word is.)
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
CHAIN_BITS = 1 | 2 | 4 | 64 | 128 | 256          # the flag bits the chain kernel raises
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chain_producers_parent.npz")
FULL_GRADS = ("ragged_T73", "T200", "V33_blank8")      # cases whose whole gradient is in the fixture
FRAMES = (1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 71, 72, 73, 129, 200)
ALPHABETS = (2, 7, 8, 9, 16, 17, 24, 25, 29, 32, 33, 48, 49, 64, 65, 78, 96)
MAX_V = 78                                       # the widest alphabet of the lean halo chains


def log_softmax(x):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = x.max(axis=-1, keepdims=True)
        m = np.where(np.isfinite(m), m, 0.0)
        return x - m - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


def targets(rng, B, width, V, blank, exclude=()):
    """(B, width) labels without the blank and without adjacent repeats (S labels then need S frames); V = 2 has one label"""
    labels = np.asarray([v for v in range(V) if v != blank and v not in exclude])
    if len(labels) == 1:
        return np.full((B, width), labels[0])
    k = rng.integers(0, len(labels), size=(B, width))
    step = rng.integers(1, len(labels), size=(B, width))
    for j in range(1, width):
        same = k[:, j] == k[:, j - 1]
        k[same, j] = (k[same, j] + step[same, j]) % len(labels)
    return labels[k]


def base(seed, T, tl, V=29, blank=0, xl=None, width=64, exclude=()):
    rng = np.random.default_rng(seed)
    B = len(tl)
    x = rng.standard_normal((B, T, V)).astype(np.float32)
    return dict(x=x, tg=targets(rng, B, width, V, blank, exclude), xl=np.full(B, T) if xl is None else np.asarray(xl),
                tl=np.asarray(tl), blank=blank, logprobs=False, width=width, form="contiguous", dtype=torch.float32)


def _frames(T):
    width = 64 if T < 129 else 128
    return base(9000 + T, T, [1, max(T // 4, 1), min(max(T // 2, 1), width), min(T + 3, width)], width=width)


def _ragged(T):
    xl = {17: [17, 16, 15, 9, 8, 7, 2, 1], 73: [73, 72, 71, 65, 64, 63, 9, 1], 200: [200, 199, 193, 192, 191, 129, 17, 8]}[T]
    return base(9300 + T, T, [max(min(n // 3, 60), 1) for n in xl], xl=xl, width=64 if T < 129 else 128)


def _alphabet(V, blank):
    # (V = 2: the one label repeats, 20 labels need 39 frames)
    return base(9400 + 100 * V + blank, 73, (1, 10, 18, 20), V=V, blank=blank, xl=[73, 72, 65, 40])


def _form(form, dtype=torch.float32, V=29, blank=0):
    c = base(9500 + V, 73, (1, 10, 18, 20), V=V, blank=blank, xl=[73, 72, 65, 40])
    c.update(form=form, dtype=dtype)
    if dtype != torch.float32:
        c["x"] = torch.from_numpy(c["x"]).to(dtype).float().numpy()          # the oracle sees the rounded logits
    return c


def _logprobs(V=29, form="contiguous"):
    c = base(9600 + V, 73, (1, 10, 18, 20), V=V, xl=[73, 72, 65, 40])
    c.update(x=log_softmax(c["x"]).astype(np.float32), logprobs=True, form=form)
    return c


def _neginf(logprobs, V=29):
    """-inf on symbol 11 (in no target) in every third frame of all utterances, on symbol 3 (V >= 25: and on 20, another column
    group) in frame 30; utterance 3 has symbol 11 as a target in a stretch where it is impossible: no alignment"""
    c = base(9700 + V + logprobs, 73, (1, 10, 18, 20), V=V, xl=[73, 72, 65, 40], exclude=(11,))
    x = log_softmax(c["x"]).astype(np.float32) if logprobs else c["x"]
    x[:, ::3, 11] = -np.inf
    x[:2, 30, 3] = -np.inf
    if V >= 25:
        x[:2, 30, 20] = -np.inf
    x[3, :, 11] = -np.inf
    c["tg"][3, 5] = 11
    c.update(x=x, logprobs=bool(logprobs))
    return c


def _scaled(V=29):
    """whole rows times 30: frames 8..10 and the last frame of utterance 1, frame 0 of utterance 2 (its flag word: 64 | 256);
    utterance 3: one frame times 17 (a spread of about 70: near the first threshold)"""
    c = base(9800 + V, 73, (10, 10, 10, 10), V=V, xl=[73, 72, 65, 40])
    c["x"][1, 8:11] *= 30
    c["x"][1, 71] *= 30
    c["x"][2, 0] *= 30
    c["x"][3, 20] *= 17
    return c


CASES = {}
for _T in FRAMES:
    CASES["T%d" % _T] = functools.partial(_frames, _T)
for _T in (17, 73, 200):
    CASES["ragged_T%d" % _T] = functools.partial(_ragged, _T)
for _V in ALPHABETS:
    CASES["V%d" % _V] = functools.partial(_alphabet, _V, 0)
for _V, _bl in ((2, 1), (9, 8), (16, 8), (16, 15), (29, 8), (29, 28), (33, 8), (33, 32), (49, 8), (49, 48), (78, 8), (78, 77)):
    CASES["V%d_blank%d" % (_V, _bl)] = functools.partial(_alphabet, _V, _bl)
CASES.update({
    "padded_sT": lambda: _form("padded_sT"),
    "padded_sT_V33": lambda: _form("padded_sT", V=33),
    "sV2": lambda: _form("sV2"),
    "sV2_V17_blank8": lambda: _form("sV2", V=17, blank=8),
    "f16": lambda: _form("contiguous", torch.float16),
    "bf16": lambda: _form("contiguous", torch.bfloat16),
    "bf16_V33_blank32": lambda: _form("contiguous", torch.bfloat16, V=33, blank=32),
    "f16_padded_sT": lambda: _form("padded_sT", torch.float16),
    "logprobs": _logprobs,
    "logprobs_V49": lambda: _logprobs(49),
    "logprobs_sV2": lambda: _logprobs(form="sV2"),
    "neginf_logits": lambda: _neginf(0),
    "neginf_logits_V12": lambda: _neginf(0, 12),
    "neginf_logprobs": lambda: _neginf(1),
    "rows_times_30": _scaled,
    "rows_times_30_V33": lambda: _scaled(33),
})


def device_logits(c):
    x = torch.from_numpy(np.asarray(c["x"], dtype=np.float32)).to(c["dtype"])
    B, T, V = x.shape
    if c["form"] == "padded_sT":
        wide = torch.zeros(B, T, 40 if V <= 40 else V + 7, dtype=x.dtype)
        wide[:, :, :V] = x
        x = wide[:, :, :V]
        assert x.stride(2) == 1 and x.stride(1) > V
    elif c["form"] == "sV2":
        wide = torch.zeros(B, T, 2 * V, dtype=x.dtype)
        wide[:, :, ::2] = x
        x = wide[:, :, ::2]
        assert x.stride(2) == 2
    else:
        assert c["form"] == "contiguous" and x.is_contiguous()
    return x


def run(c, algo):
    """one call; returns losses, grads and flag words, and asserts the route"""
    B, T, V = c["x"].shape
    keep = {}
    la, ga = U.c_abi_loss(device_logits(c), c["tg"], c["xl"], c["tl"], c["blank"], c["logprobs"], algo, keep=keep,
                          width=c["width"], padding=-1)
    assert keep["Smax"] == c["width"]
    L = _lib.load()
    flags, logz = (ctypes.c_int * B)(), (ctypes.c_double * (2 * B))()
    assert L.e2e_debug_fast_state(keep["workspace"].data_ptr(), B, T, V, keep["Smax"], flags, logz) == 0
    route, pairs = keep["route"], 2 if c["width"] == 64 else 4
    assert B <= 8 and route // 1000 == 2 and route % 100 // 10 == pairs, "route %d" % route
    assert route % 10 == (4 if V <= MAX_V else 6), "route %d: not the lean halo chains" % route
    return la, ga, list(flags)


def oracle(c):
    lp = np.asarray(c["x"], dtype=np.float64) if c["logprobs"] else log_softmax(c["x"])
    l_o, g_o = O.ctc_loss(lp, c["tg"], c["xl"], c["tl"], c["blank"])
    if not c["logprobs"]:
        for b in range(len(l_o)):
            if np.isfinite(l_o[b]):
                g_o[b, c["xl"][b]:] = 0.0
    return l_o, g_o


def expected_chain_bits(c, l_o):
    """the chain kernel's flag bits as the producers' rule and the oracle give them"""
    x = np.asarray(c["x"], dtype=np.float32)
    want = []
    for b in range(len(l_o)):
        rows = x[b, :c["xl"][b]]
        with np.errstate(invalid="ignore"):
            d = rows if c["logprobs"] else (rows - rows.max(axis=-1, keepdims=True)).astype(np.float32)
        d = d[np.isfinite(rows) & ~np.isnan(d)]
        lo = min(float(d.min()), 0.0) if d.size else 0.0
        want.append((0 if np.isfinite(l_o[b]) else 4) | (64 if lo < -69.0 else 0) | (256 if lo < -78.0 else 0))
    return want


@functools.lru_cache(maxsize=None)
def computed(name):
    c = CASES[name]()
    return c, run(c, _lib.ALGO_FAST), oracle(c)


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(GOLDEN)


def tolerances(c):
    if c["dtype"] == torch.float32:
        return LOSS_RTOL, 0.0, GRAD_RTOL, GRAD_ATOL
    eps = 2.0 ** -7 if c["dtype"] == torch.bfloat16 else 2.0 ** -10
    return 1e-4, 2e-5, 2 * eps, 2e-6


@pytest.mark.parametrize("name", list(CASES))
def test_case_equals_the_oracle_and_its_flag_words_are_the_rule(name):
    c, (la, ga, flags), (l_o, g_o) = computed(name)
    want_bits = expected_chain_bits(c, l_o)
    ok = np.array([f == 0 for f in flags])
    with np.errstate(invalid="ignore", divide="ignore"):
        print("flags", flags, "expected chain bits", want_bits,
              "max |dloss|/|loss| %.3g" % np.max(np.abs(la[ok] - l_o[ok]) / np.abs(l_o[ok]), initial=0.0),
              "max |dgrad| %.3g" % np.max(np.abs(ga[ok] - g_o[ok]), initial=0.0))
    assert [f & CHAIN_BITS for f in flags] == want_bits, "flag words %s" % flags
    lr, la_, gr, ga_ = tolerances(c)
    U.assert_same(la[ok], l_o[ok], lr, la_, "losses")
    U.assert_same(ga[ok], g_o[ok], gr, ga_, "grads")
    if not ok.all():
        la2, ga2, flags2 = run(c, _lib.ALGO_AUTO)
        assert [f & CHAIN_BITS for f in flags2] == want_bits, "flag words after ALGO_AUTO %s" % flags2
        U.assert_same(la2, l_o, lr, la_, "losses, ALGO_AUTO")
        U.assert_same(ga2, g_o, gr, ga_, "grads, ALGO_AUTO")


def recorded_parts(la, ga, flags):
    """what the recording keeps of a case: the flag words of all utterances, losses and gradients of the unflagged ones"""
    ok = np.array([f == 0 for f in flags])
    return np.asarray(flags, dtype=np.int32), np.ascontiguousarray(la[ok]), np.ascontiguousarray(ga[ok])


@pytest.mark.parametrize("name", list(CASES))
def test_case_equals_the_recording_bit_for_bit(name):
    _, (la, ga, flags), _ = computed(name)
    g = golden()
    flags, la, ga = recorded_parts(la, ga, flags)
    assert np.array_equal(flags, g[name + "/flags"]), "flag words %s, recorded %s" % (flags.tolist(), g[name + "/flags"].tolist())
    assert np.array_equal(la.view(np.uint32), g[name + "/losses"].view(np.uint32)), "losses"
    if name in FULL_GRADS:
        want = g[name + "/grads"]
        diff = np.flatnonzero(ga.view(np.uint32).ravel() != want.view(np.uint32).ravel())
        assert diff.size == 0, "gradient differs at %d elements, first %s" % (diff.size, np.unravel_index(diff[0], ga.shape))
    assert hashlib.sha256(ga.tobytes()).hexdigest() == str(g[name + "/grads_sha256"]), "gradient"


def test_fixture_holds_exactly_the_cases():
    assert {k.split("/")[0] for k in golden().files} == set(CASES)
    assert os.path.getsize(GOLDEN) < 1 << 18


def test_the_cases_cover_what_they_claim():
    """no GPU work: every frame count, alphabet, blank position and input form of the list above is in CASES, with dead rows
    and steady blocks, an utterance without an alignment, and -inf in a live column"""
    cs = {k: f() for k, f in CASES.items()}
    assert {c["x"].shape[1] for c in cs.values()} >= set(FRAMES)
    assert {c["x"].shape[2] for c in cs.values()} >= set(ALPHABETS)
    assert {(c["blank"] == 0, c["blank"] == c["x"].shape[2] - 1, c["blank"] == 8) for c in cs.values()} >= \
        {(True, False, False), (False, True, False), (False, False, True)}
    assert {(c["form"], c["dtype"]) for c in cs.values()} >= {("contiguous", torch.float32), ("padded_sT", torch.float32),
                                                               ("sV2", torch.float32), ("contiguous", torch.float16),
                                                               ("contiguous", torch.bfloat16)}
    assert any(c["logprobs"] for c in cs.values())
    xl = np.concatenate([c["xl"] for c in cs.values()])
    assert {int(n) % 8 for n in xl} >= {7, 0, 1}
    assert all((c["tl"] > c["xl"]).any() for k, c in cs.items() if k[0] == "T" and c["x"].shape[1] + 3 <= 64)
    assert np.isneginf(cs["neginf_logits"]["x"]).any() and np.isneginf(cs["neginf_logprobs"]["x"]).any()
