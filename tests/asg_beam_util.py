"""Shared cases of the ASG beam search tests (TEST INFRASTRUCTURE ONLY): the inputs are drawn once in f32 -- so that the
f32 and f64 calls see the same numbers -- and every reference is computed once per process."""
import functools
import os

import numpy as np

import asg_beam_ref as REF

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# (V, T, R, space_id): at most 256 paths per utterance
TINY_GRID = [(2, 8, 0, -1), (3, 5, 0, -1), (4, 3, 0, -1), (5, 3, 0, -1), (4, 3, 1, -1), (5, 3, 2, 1)]
TINY_LENS = {8: [8, 1, 5], 5: [5, 1, 3], 3: [3, 1, 2]}

# the pruned cases: V = 29 (27 characters with the space at 0, 2 repeat labels), T = 40, B = 3 ragged
PRUNED_V, PRUNED_T, PRUNED_R, PRUNED_SPACE = 29, 40, 2, 0
PRUNED_LENS = [40, 23, 31]
PRUNED_WIDTHS = [1, 2, 7, 32, 100]
PRUNED_SEED = 11
WIDE_V, WIDE_T, WIDE_W, WIDE_SEED = 128, 12, 16, 5
WIDE_LENS = [12, 7, 9]

MIN_GAP = 1e-7         # a cut decided by less is decided by f64 evaluation order (about 1e-12 here)


def draw(seed, B, T, V, scale=1.0):
    """(x (B,T,V) f32, A (V,V) f32), both N(0,1) (x times `scale`)."""
    g = np.random.default_rng(seed)
    x = (g.standard_normal((B, T, V)) * scale).astype(np.float32)
    A = g.standard_normal((V, V)).astype(np.float32)
    return x, A


@functools.lru_cache(maxsize=None)
def tiny_case(i):
    V, T, R, space = TINY_GRID[i]
    x, A = draw(100 + i, 3, T, V)
    lens = TINY_LENS[T]
    enum = [REF.enumerate_paths(x[b].tolist(), A.tolist(), lens[b], V, R, space) for b in range(3)]
    return x, A, lens, enum


@functools.lru_cache(maxsize=None)
def tiny_unbounded(i):
    V, T, R, space = TINY_GRID[i]
    x, A, lens, _ = tiny_case(i)
    return REF.beam(x.tolist(), A.tolist(), lens, V, R, space, W=None)[0]


@functools.lru_cache(maxsize=None)
def pruned_case():
    return draw(PRUNED_SEED, 3, PRUNED_T, PRUNED_V)


@functools.lru_cache(maxsize=None)
def pruned_ref(W):
    x, A = pruned_case()
    return REF.beam(x.tolist(), A.tolist(), PRUNED_LENS, PRUNED_V, PRUNED_R, PRUNED_SPACE, W=W)


@functools.lru_cache(maxsize=None)
def wide_case():
    return draw(WIDE_SEED, 3, WIDE_T, WIDE_V)


@functools.lru_cache(maxsize=None)
def wide_ref():
    x, A = wide_case()
    return REF.beam(x.tolist(), A.tolist(), WIDE_LENS, WIDE_V, 0, -1, W=WIDE_W)


# ---- with a language model: labels that spell the models' words, one repeat label ----
LM_MODELS = {
    "tiny_3gram.arpa": dict(chars=["a", "b", " "], seed=21),
    "lm_order4.arpa": dict(chars=[" ", "a", "b", "c", "d", "e", "'"], seed=22),
}
LM_T, LM_LENS, LM_R = 14, [14, 9, 1], 1
LM_WIDTHS = [2, 7, 32]
LM_KNOBS = dict(lmwt=0.7, wip=0.4, oov_penalty=-1.3)


def upper_chars(chars):
    """The same alphabet in upper case: only a case-insensitive look-up finds the models' (lower-case) words."""
    return [c.upper() for c in chars]


@functools.lru_cache(maxsize=None)
def lm_case(model):
    m = LM_MODELS[model]
    V = len(m["chars"]) + LM_R
    return draw(m["seed"], 3, LM_T, V, scale=2.0)


@functools.lru_cache(maxsize=None)
def oracle_lm(model):
    import oracle_lib as O
    return O.OracleLM(os.path.join(GOLDEN, model))


@functools.lru_cache(maxsize=None)
def lm_ref(model, W, case_sensitive):
    m = LM_MODELS[model]
    chars = m["chars"] if case_sensitive else upper_chars(m["chars"])
    x, A = lm_case(model)
    V = len(chars) + LM_R
    return REF.beam(x.tolist(), A.tolist(), LM_LENS, V, LM_R, chars.index(" "), W=W, chars=chars, lm=oracle_lm(model),
                    case_sensitive=case_sensitive, **LM_KNOBS)
