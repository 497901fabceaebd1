"""Shared cases of the restricted ASG beam search tests (TEST INFRASTRUCTURE ONLY): tests/test_asg_lexicon_cpu.py (the
restatement against enumeration, margins, coverage) and tests/test_gpu_asg_lexicon.py (the kernel).  Inputs are drawn once in
f32, so that the f32 and the f64 call see the same numbers; every reference is computed once per process and left unchanged.

  grids   (V, R, T) = (3,0,5), (4,1,4), (5,2,3), (4,2,4) with a word list each: at most 256 paths per utterance
  pruned  V = 29 (27 characters, the space at 0, 2 repeat labels), T = 40, B = 4 (one ragged, one length outside [1, T]),
          widths 2 / 7 / 32 / 100, three models: tests/golden/tiny_3gram.arpa in both case modes and a list of 20 words
  wide    V = 128 (126 characters, 2 repeat labels), W = 16, T = 24, a list of words drawn from the alphabet
  fuzz    48 seeds: draw(seed) is a pure function of the seed
"""
import functools
import os
from types import SimpleNamespace

import numpy as np

import asg_beam_fuzz_util as F
import asg_beam_util as U
import asg_lexicon_ref as LR

MIN_GAP = U.MIN_GAP
LETTERS = [" "] + [chr(97 + i) for i in range(26)]

# ---- the grids ---------------------------------------------------------------------------------------------------------
GRIDS = [
    dict(V=3, R=0, T=5, chars=["a", "b", " "], words=["ab", "a", "bab"]),
    dict(V=4, R=1, T=4, chars=["a", " ", "b"], words=["aab", "ba", "b"]),
    dict(V=5, R=2, T=3, chars=["a", " ", "b"], words=["aaa", "ab", "bb"]),
    dict(V=4, R=2, T=4, chars=["a", "b"], words=["aaab", "bba", "ab", "abb"]),
]


def space_of(chars):
    return chars.index(" ") if " " in chars else -1


@functools.lru_cache(maxsize=None)
def grid_case(i):
    """(x, A, lens, [per utterance {admissible labelling: ac}], [per utterance number of spellable labellings])."""
    g = GRIDS[i]
    V, R, T = g["V"], g["R"], g["T"]
    x, A = U.draw(300 + i, 3, T, V)
    lens = [T, 1, T - 1]
    lex = LR.Lexicon(g["words"])
    enum, total = [], []
    for b in range(3):
        every = LR.enumerate_paths(x[b].tolist(), A.tolist(), lens[b], V, R, space_of(g["chars"]))
        total.append(len(every))
        enum.append({s: ac for s, ac in every.items() if LR.admissible(s, V, R, space_of(g["chars"]), g["chars"], lex)})
    return x, A, lens, enum, total


@functools.lru_cache(maxsize=None)
def grid_unbounded(i):
    g = GRIDS[i]
    x, A, lens, _, _ = grid_case(i)
    return LR.beam(x.tolist(), A.tolist(), lens, g["V"], g["R"], space_of(g["chars"]), W=None, chars=g["chars"],
                   lm=LR.WordListLM(g["words"]), lexicon=LR.Lexicon(g["words"]))[0]


# ---- the pruned cases --------------------------------------------------------------------------------------------------
P_V, P_T, P_R, P_SEED = 29, 40, 2, 41
P_LENS = [40, 23, 41, 31]
P_WIDTHS = [2, 7, 32, 100]
P_WORDS = ["add", "all", "bee", "been", "book", "cool", "egg", "eel", "fee", "feel", "go", "good", "ill", "inn", "no", "noon",
           "odd", "off", "see", "seen", "too", "zoo"][:20]
P_KNOBS = dict(lmwt=0.7, wip=0.4, oov_penalty=-1.3)
P_MODELS = {
    "arpa": dict(model="tiny_3gram.arpa", case_sensitive=True, chars=LETTERS),
    "arpa_folded": dict(model="tiny_3gram.arpa", case_sensitive=False, chars=U.upper_chars(LETTERS)),
    "words": dict(model=None, case_sensitive=True, chars=LETTERS),
}


@functools.lru_cache(maxsize=None)
def pruned_case():
    return U.draw(P_SEED, 4, P_T, P_V, scale=2.0)


def model_and_lexicon(model, words, case_sensitive):
    """(the restatement's model, its lexicon) of an ARPA file of tests/golden or of a word list."""
    if model:
        return U.oracle_lm(model), LR.Lexicon(LR.arpa_words(os.path.join(U.GOLDEN, model)), case_sensitive)
    return LR.WordListLM(words, case_sensitive), LR.Lexicon(words, case_sensitive)


@functools.lru_cache(maxsize=None)
def pruned_ref(name, W):
    m = P_MODELS[name]
    x, A = pruned_case()
    lm, lex = model_and_lexicon(m["model"], P_WORDS, m["case_sensitive"])
    knobs = P_KNOBS if m["model"] else dict(lmwt=0.0, wip=P_KNOBS["wip"], oov_penalty=0.0)
    return LR.beam(x.tolist(), A.tolist(), P_LENS, P_V, P_R, 0, W=W, chars=m["chars"], lm=lm, case_sensitive=m["case_sensitive"],
                   lexicon=lex, **knobs)


def alphabet(n, space=-1, upper=False):
    """n distinct label strings: letters first, then other ASCII but '<' (no label begins <unk>, <s> or </s>), then two-byte
    characters; the space at `space` (negative: none)."""
    pool = [chr(c) for c in range(97, 123)] + [chr(c) for c in range(33, 127) if not chr(c).isalpha() and chr(c) != "<"] + \
        [chr(c) for c in range(0xDF, 0x250) if chr(c).lower() == chr(c)]     # (str.lower, the restatement's, leaves them)
    out = pool[:n]
    if upper:
        out = [c.upper() if "a" <= c <= "z" else c for c in out]
    if space >= 0:
        out[space] = " "
    return out


def draw_words(rng, chars, n, longest=6):
    """n words over the characters (the space excluded), a doubled letter in about a third of them."""
    letters = [c for c in chars if c != " "]
    first = [letters[int(k)] for k in rng.integers(len(letters), size=max(1, min(len(letters), 1 + n // 3)))]
    words = []
    for _ in range(n):
        w = [first[int(rng.integers(len(first)))]]
        for _ in range(int(rng.integers(0, longest))):
            w.append(w[-1] if rng.integers(3) == 0 else letters[int(rng.integers(len(letters)))])
        words.append("".join(w))
    return list(dict.fromkeys(words))


WIDE_V, WIDE_R, WIDE_T, WIDE_W, WIDE_SEED = 128, 2, 24, 16, 43
WIDE_LENS = [24, 13, 17]


@functools.lru_cache(maxsize=None)
def wide_case():
    rng = np.random.default_rng(WIDE_SEED)
    chars = alphabet(WIDE_V - WIDE_R, space=5)
    words = draw_words(rng, chars, 40)
    x, A = U.draw(WIDE_SEED, 3, WIDE_T, WIDE_V, scale=2.0)
    return x, A, chars, words


@functools.lru_cache(maxsize=None)
def wide_ref():
    x, A, chars, words = wide_case()
    return LR.beam(x.tolist(), A.tolist(), WIDE_LENS, WIDE_V, WIDE_R, 5, W=WIDE_W, chars=chars, lm=LR.WordListLM(words),
                   wip=0.25, lexicon=LR.Lexicon(words))


# ---- the fuzz ----------------------------------------------------------------------------------------------------------
FUZZ_N = 48
FUZZ_SEED0 = 52000
FUZZ_V = (3, 5, 29, 31, 128)
FUZZ_W = (1, 2, 3, 7, 32, 33, 100, 128)
FUZZ_BUDGET = 250000
LEFT_OUT_CAP = 0.03
LEFT_OUT = ()                               # the seeds below MIN_GAP (test_asg_lexicon_cpu.py computes them: equal)


@functools.lru_cache(maxsize=None)
def draw(seed):
    rng = np.random.default_rng(FUZZ_SEED0 + seed)
    c = SimpleNamespace(seed=seed, V=FUZZ_V[seed % len(FUZZ_V)], W=FUZZ_W[seed % len(FUZZ_W)])
    c.dtype = ("f32", "f64")[(seed // 2) % 2]
    c.timesteps = seed % 2 == 0
    c.masked = seed % 4 == 1
    c.R = int(rng.integers(0, min(2, c.V - 2) + 1))
    c.model = F.LM_FILES[(seed // 4) % len(F.LM_FILES)] if seed % 4 == 3 else None
    upper = bool(rng.integers(2))
    with_space = bool(rng.integers(4))
    if c.model:
        own = list(F.model_chars(c.model))
        if len(own) + 1 + c.R > c.V:
            c.V = 29
        rest = [ch for ch in alphabet(c.V) if ch not in own]
        chars = (own + rest)[: c.V - c.R]
        c.case_sensitive = not upper
        if upper:
            chars = [ch.upper() if "a" <= ch <= "z" else ch for ch in chars]
        c.space = int(rng.integers(len(chars))) if with_space else -1
        if c.space >= 0:
            chars[-1] = chars[c.space]           # (the character the space displaces moves to the end: it may spell a word)
            chars[c.space] = " "
        c.chars, c.words = chars, None
        c.lmwt, c.oov = (0.0, 0.7, 2.0)[int(rng.integers(3))], (-1.3, -1000.0)[int(rng.integers(2))]
    else:
        c.space = int(rng.integers(c.V - c.R)) if with_space else -1
        c.chars = alphabet(c.V - c.R, c.space, upper)
        c.case_sensitive = bool(rng.integers(2))
        c.words = draw_words(rng, c.chars, int(rng.integers(3, 25)), longest=(3 if c.V <= 5 else 6))
        c.lmwt, c.oov = 0.0, 0.0
    c.wip = (0.0, 0.4)[int(rng.integers(2))]
    B = int(rng.integers(1, 4))
    T = int(rng.integers(1, max(1, min(48, FUZZ_BUDGET // (c.W * c.V))) + 1))
    c.x_scale, c.a_scale = (1.0, 2.0, 8.0)[int(rng.integers(3))], (0.0, 1.0, 5.0)[int(rng.integers(3))]
    c.lens = F.lengths(rng, B, T)
    c.x = F.emissions(rng, B, T, c.V, c.x_scale, c.masked)
    c.A = (rng.standard_normal((c.V, c.V)) * c.a_scale).astype(np.float32)
    c.no_A = c.a_scale == 0.0 and bool(rng.integers(2))
    c.shape = {"time_major": bool(rng.integers(2)), "strided": bool(rng.integers(2)), "cpu": False, "transposed_A": False}
    c.nbest = int(rng.integers(1, c.W + 1)) if rng.integers(2) else None
    return c


@functools.lru_cache(maxsize=None)
def reference(seed):
    """(the whole final ranking of every utterance, the case's margin, the search's stats)."""
    c = draw(seed)
    lm, lex = model_and_lexicon(c.model, c.words, c.case_sensitive)
    stats = {}
    out, gap = LR.beam(c.x.tolist(), c.A.tolist(), c.lens, c.V, c.R, c.space, W=c.W, chars=c.chars, lm=lm,
                       case_sensitive=c.case_sensitive, lmwt=c.lmwt, wip=c.wip, oov_penalty=c.oov, lexicon=lex, stats=stats)
    return out, gap, stats, lex


def compared(seed):
    return reference(seed)[1] >= MIN_GAP


def facts(seed):
    """What the coverage test counts."""
    c = draw(seed)
    ranking, gap, stats, lex = reference(seed)
    alive = [b for b in range(len(c.lens)) if 1 <= c.lens[b] <= c.x.shape[1]]
    n = [len(ranking[b]) for b in alive]
    unfinished = False
    for b in alive:
        for h in ranking[b]:
            w = LR.last_word(h["ids"], c.chars, c.space)
            if h["ids"][-1] != c.space and lex.fold(w.encode()) not in lex.words:
                unfinished = True
    return SimpleNamespace(case=c, ranking=ranking, gap=gap, members=n, died=any(k == 0 for k in n),
                           never_fills=any(0 < k < c.W for k in n), full=any(k == c.W for k in n), unfinished=unfinished)
