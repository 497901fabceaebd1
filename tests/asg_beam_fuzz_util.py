"""The seeded cases of the ASG beam search fuzz (TEST INFRASTRUCTURE ONLY), shared by tests/test_asg_beam_fuzz_cpu.py (margins,
coverage) and tests/test_gpu_asg_beam_fuzz.py (the kernel).  draw(family, seed) is a pure function of its arguments; inputs are
drawn in f32, so that the f32 and the f64 call see the same numbers; reference(family, seed) is asg_beam_ref.beam of the case,
computed once per process.

Three families:
  plain  132 seeds: every pair of V in PLAIN_V and W in PLAIN_W once (the two cycles are coprime), R, the space, B, ragged
         lengths (now and then one outside [1, T]), scales, wip, masked (-inf) emissions, dtype, call shape, nbest.
         T <= min(70, PLAIN_BUDGET / (min(W, 4 V) V)): the restatement costs a few us per (member, label) pair
  long   6 seeds: T in 300..700, W <= 8, V in {5, 29}, R in {0, 2}, B = 2 with one utterance of one frame
  lm     24 seeds over the three ARPA models of tests/golden: the alphabet is the characters of the model's words (lower or
         upper case) with the space at a random place or absent, R in {0, 1, 2}, W in LM_W, T <= 30

A case whose margin (asg_beam_ref.Search.min_gap) is below asg_beam_util.MIN_GAP is not compared on the GPU: compared();
test_asg_beam_fuzz_cpu.py holds each family to at most 3 % of such cases.

Measured with the restatement on one CPU core (the figures test_gpu_asg_beam_fuzz.py's docstring repeats), none left out:
  plain  132 cases, 33 s in total, the slowest 1.8 s (V=128, W=128, B=4, T=8); smallest margin 2.4e-7;
         8 masked cases with a dead beam beside a living one, 27 cases with a beam that never fills, 111 with a full one
  long   6 cases, 2.5 s, the slowest 0.9 s (V=29, W=6, T=610); smallest margin 1.0e-3
  lm     24 cases, 0.4 s, the slowest 0.07 s; smallest margin 6.9e-6
(PLAIN_BUDGET is the 250000 the draw was first run with: ranking by total first and asking for a key only among equal totals
took the slowest case from 9 s to under 2 s, so T needed no trimming.)
"""
import functools
import math
import os
from types import SimpleNamespace

import numpy as np

import asg_beam_ref as REF
import asg_beam_util as U

PLAIN_V = (1, 2, 3, 5, 29, 31, 32, 33, 64, 65, 127, 128)
PLAIN_W = (1, 2, 3, 7, 31, 32, 33, 64, 100, 127, 128)
PLAIN_BUDGET = 250000
FAMILIES = {"plain": 132, "long": 6, "lm": 24}
SEED0 = {"plain": 35000, "long": 36000, "lm": 37000}
LEFT_OUT_CAP = 0.03                         # of a family, for margin
LEFT_OUT = {"plain": (), "long": (), "lm": ()}      # the seeds below MIN_GAP (test_asg_beam_fuzz_cpu.py computes them: equal)

LM_FILES = ("tiny_3gram.arpa", "lm_order4.arpa", "lm_order3_nounk.arpa")
LM_W = (2, 7, 33, 64, 128)
MASK_SHARE = 0.3


def plain_labels(n, space):
    """n distinct one-character strings, none a space, with the space at `space` (negative: none)."""
    out = [chr(0x41 + i) for i in range(n)]
    if space >= 0:
        out[space] = " "
    return out


@functools.lru_cache(maxsize=None)
def model_chars(model):
    """The characters the model's words are spelled with, sorted."""
    chars, grams = set(), False
    with open(os.path.join(U.GOLDEN, model)) as f:
        for line in f:
            line = line.strip()
            if line.startswith("\\"):
                grams = line == "\\1-grams:"
                continue
            if grams and line:
                w = line.split("\t")[1]
                if not w.startswith("<"):
                    chars.update(w)
    return sorted(chars)


def lengths(rng, B, T, outside=True):
    """Ragged lengths in [1, T] with one utterance at T; one time in eight another utterance is outside the range."""
    xl = rng.integers(1, T + 1, size=B)
    full = int(rng.integers(B))
    xl[full] = T
    if outside and B > 1 and int(rng.integers(8)) == 0:
        xl[(full + 1) % B] = (0, T + 1)[int(rng.integers(2))]
    return [int(n) for n in xl]


def emissions(rng, B, T, V, scale, masked):
    """N(0,1) times `scale` in f32; masked: MASK_SHARE of the emissions are -inf, in every utterance but one when there are
    several (a small alphabet's beam dies of it: the utterance left alone is the living one beside it)."""
    x = (rng.standard_normal((B, T, V)) * scale).astype(np.float32)
    if masked:
        mask = rng.random((B, T, V)) < MASK_SHARE
        if B > 1:
            mask[int(rng.integers(B))] = False
        x[mask] = -np.inf
    return x


def call_shape(rng):
    return {"time_major": bool(rng.integers(2)), "strided": bool(rng.integers(2)), "cpu": bool(rng.integers(4) == 0),
            "transposed_A": bool(rng.integers(2))}


def draw_plain(seed):
    rng = np.random.default_rng(SEED0["plain"] + seed)
    V, W = PLAIN_V[seed % len(PLAIN_V)], PLAIN_W[seed % len(PLAIN_W)]
    c = SimpleNamespace(family="plain", seed=seed, V=V, W=W, model=None, case_sensitive=True, lmwt=0.0, oov=0.0)
    c.dtype = ("f32", "f64")[(seed // len(PLAIN_V)) % 2]
    c.R = int(rng.integers(0, min(2, V - 1) + 1))
    c.space = int(rng.integers(V - c.R)) if rng.integers(2) else -1
    c.chars = plain_labels(V - c.R, c.space)
    B = int(rng.integers(1, 5))
    T = int(rng.integers(1, max(1, min(70, PLAIN_BUDGET // (min(W, 4 * V) * V))) + 1))
    c.x_scale, c.a_scale = (1.0, 8.0, 30.0)[int(rng.integers(3))], (0.0, 1.0, 5.0)[int(rng.integers(3))]
    c.wip = (0.0, 0.25)[int(rng.integers(2))]
    c.masked = bool(rng.integers(4) == 0)
    c.lens = lengths(rng, B, T)
    c.x = emissions(rng, B, T, V, c.x_scale, c.masked)
    c.A = (rng.standard_normal((V, V)) * c.a_scale).astype(np.float32)
    c.no_A = c.a_scale == 0.0 and bool(rng.integers(2))          # zero transitions: passed as None
    c.shape = call_shape(rng)
    c.nbest = int(rng.integers(1, W + 1)) if rng.integers(2) else None
    return c


def draw_long(seed):
    rng = np.random.default_rng(SEED0["long"] + seed)
    c = SimpleNamespace(family="long", seed=seed, model=None, case_sensitive=True, lmwt=0.0, oov=0.0, masked=False, no_A=False)
    c.V, c.R = (5, 29)[seed % 2], (0, 2)[(seed // 2) % 2]
    c.W = int(rng.integers(2, 9))
    c.dtype = ("f32", "f64")[(seed // 3) % 2]
    c.space = int(rng.integers(c.V - c.R)) if rng.integers(2) else -1
    c.chars = plain_labels(c.V - c.R, c.space)
    T = int(rng.integers(300, 701))
    c.x_scale, c.a_scale = (1.0, 8.0, 30.0)[int(rng.integers(3))], (0.0, 1.0, 5.0)[int(rng.integers(3))]
    c.wip = (0.0, 0.25)[int(rng.integers(2))]
    c.lens = [T, 1] if rng.integers(2) else [1, T]
    c.x = emissions(rng, 2, T, c.V, c.x_scale, False)
    c.A = (rng.standard_normal((c.V, c.V)) * c.a_scale).astype(np.float32)
    c.shape = call_shape(rng)
    c.nbest = int(rng.integers(1, c.W + 1)) if rng.integers(2) else None
    return c


def draw_lm(seed):
    rng = np.random.default_rng(SEED0["lm"] + seed)
    c = SimpleNamespace(family="lm", seed=seed, no_A=False)
    c.model = LM_FILES[seed % len(LM_FILES)]
    c.W = LM_W[seed % len(LM_W)]
    c.R = (seed // len(LM_FILES)) % 3
    c.dtype = ("f32", "f64")[(seed // 2) % 2]
    chars = list(model_chars(c.model))
    upper = bool(rng.integers(2))
    if upper:
        chars = U.upper_chars(chars)
    c.case_sensitive = bool(rng.integers(2))
    c.space = int(rng.integers(len(chars) + 1)) if rng.integers(4) else -1
    if c.space >= 0:
        chars.insert(c.space, " ")
    c.chars = chars
    c.V = len(chars) + c.R
    B = int(rng.integers(1, 4))
    T = int(rng.integers(2, 31))
    c.x_scale, c.a_scale = (1.0, 2.0, 8.0)[int(rng.integers(3))], (0.0, 1.0, 5.0)[int(rng.integers(3))]
    c.lmwt, c.wip = (0.0, 0.7, 2.0)[int(rng.integers(3))], (0.0, 0.4)[int(rng.integers(2))]
    c.oov = (-1.3, -1000.0)[int(rng.integers(2))]
    c.masked = bool(rng.integers(4) == 0)
    c.lens = lengths(rng, B, T, outside=False)
    c.x = emissions(rng, B, T, c.V, c.x_scale, c.masked)
    c.A = (rng.standard_normal((c.V, c.V)) * c.a_scale).astype(np.float32)
    c.shape = call_shape(rng)
    c.nbest = int(rng.integers(1, c.W + 1)) if rng.integers(2) else None
    return c


@functools.lru_cache(maxsize=None)
def draw(family, seed):
    return {"plain": draw_plain, "long": draw_long, "lm": draw_lm}[family](seed)


@functools.lru_cache(maxsize=None)
def reference(family, seed):
    """(the whole final ranking of every utterance, the case's margin)."""
    c = draw(family, seed)
    lm = U.oracle_lm(c.model) if c.model else None
    return REF.beam(c.x.tolist(), c.A.tolist(), c.lens, c.V, c.R, c.space, W=c.W, chars=c.chars, lm=lm,
                    case_sensitive=c.case_sensitive, lmwt=c.lmwt, wip=c.wip, oov_penalty=c.oov)


def compared(family, seed):
    """Is the case compared on the GPU?  Its cuts and its final order are at least MIN_GAP apart."""
    return reference(family, seed)[1] >= U.MIN_GAP


def alive(c, b):
    return 1 <= c.lens[b] <= c.x.shape[1]


def facts(family, seed):
    """What the coverage test counts: per utterance within the range, the members of the final beam."""
    c = draw(family, seed)
    ranking, gap = reference(family, seed)
    n = [len(ranking[b]) for b in range(len(c.lens)) if alive(c, b)]
    return SimpleNamespace(case=c, ranking=ranking, gap=gap, members=n, full=any(k == c.W for k in n),
                           dead_beside_living=any(k == 0 for k in n) and any(k > 0 for k in n),
                           partial=any(0 < k < c.W for k in n))
