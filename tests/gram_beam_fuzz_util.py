"""The seeded cases of the Gram-CTC decoding fuzz (TEST INFRASTRUCTURE ONLY), shared by tests/test_gram_beam_fuzz_cpu.py
(margins, coverage), tests/test_gpu_gram_beam_fuzz.py (the kernels) and tests/test_gpu_gram_stream_fuzz.py (the stream).
draw(family, seed) is a pure function of its arguments.  Emissions are log-probabilities drawn in f32 (the f32 rounding of the
f64 log-softmax of f32 logits; masked ones set to -inf afterwards), so that the f32 and the f64 call see the same numbers;
reference(family, seed) runs the restatement on them once per process, per utterance.  The restatements are imported, not
edited: what the coverage test wants to know of a search's frames (how many members, how many of them stayed) is read off
the candidate lists they rank, through a recording wrapper around their `_ranked` (trace()).

Five families:
  plain   132 seeds: every pair of V in PLAIN_V and W in PLAIN_W once (the two cycles are coprime; W is held to
          max_width(V), and `cap` is that width itself), tables of random_table -- unigrams only, largest order 2, 3 and 8 --,
          B 1..4, ragged lengths with 0, 1 and T (now and then T + 1, which the header clamps), scales 1 / 3 / 10, one case in
          four masked, dtype, call shape, nbest.  T <= PLAIN_BUDGET / (W V) + 1, at most 30 (20 from W = 100 on)
  long    6 seeds: T in 300..700, W <= 8, V in {21, 33}, B = 2 with one utterance of one frame, scales 1 / 10 / 30
  lm      28 seeds over the three ARPA models of tests/golden (gram_decode_lm_ref.beam_search): base labels the characters of
          the model's words, lower or upper case, the space at a random place or absent; random grams over them and, with a
          space, one gram each with an inner, a leading and a trailing space; W in LM_W; the knobs drawn; a fifth of the cases
          without a model; a third with one frame that is nearly all blank (every member stays); under every other wide beam
          one frame in which a single letter's column is not -inf (most members of the full beam stay with a total of zero)
  lex     28 seeds: the lm draw restricted to the model's words or to a word list drawn from them (gram_lexicon_ref.beam_search
          with a Rule), timesteps asked for in every case
  greedy  30 seeds: every pair of V in GREEDY_V and T in GREEDY_T, the four dtypes, constructed ties of the maximum

An utterance whose margin -- the smaller of the smallest gap at any cut and the smallest gap between neighbours of the final
ranking whose scores differ (relative for the masses, absolute for log totals) -- is below gram_decode_lm_ref.MIN_GAP is not
compared on the GPU: compared(); test_gram_beam_fuzz_cpu.py holds each family to at most LEFT_OUT_CAP of its utterances and
LEFT_OUT to what it recomputes.

Measured with the restatements on one CPU core (the figures test_gpu_gram_beam_fuzz.py's docstring repeats):
  plain   132 cases, 285 utterances, 38 s in total, the slowest 1.5 s (seed 29: V=1023, W=32, B=4, T=9); one utterance left
          out (seed 115, utterance 0: 7.9e-7), smallest margin of the others 2.1e-6
  long    6 cases, 12 utterances, 3.1 s, the slowest 1.0 s (seed 5: V=33, W=6, T=680); none left out, smallest margin 1.2e-5
  lm      28 cases, 52 utterances, 14 s, the slowest 2.4 s (seed 20: V=47, W=128, B=2, T=19); none left out,
          smallest margin 1.2e-6
  lex     28 cases, 50 utterances, 5.8 s, the slowest 1.2 s (seed 5: V=67, W=127, B=2, T=13); none left out,
          smallest margin 4.9e-6
  greedy  30 cases: the definition is three lines of numpy
"""
import functools
import math
import os
from types import SimpleNamespace

import numpy as np

import asg_beam_fuzz_util as AF
import gram_decode_lm_ref as LR
import gram_decode_ref as DR
import gram_lexicon_ref as XR
import gram_ref as GR
from lexicon_ref import Lexicon, WordListLM, arpa_words

PLAIN_V = (2, 3, 21, 63, 64, 65, 379, 1023, 1024, 1025, 1100)
PLAIN_W = (1, 2, 3, 7, 31, 32, 33, 64, 100, 127, 128, "cap")
PLAIN_KINDS = ("unigrams", "order2", "order3", "order8")
PLAIN_BUDGET = 450000                       # (member, column) pairs of one utterance: the restatement takes some 2.3 us each
PLAIN_SCALES = (1.0, 3.0, 10.0)
LONG_SCALES = (1.0, 10.0, 30.0)
LM_FILES = AF.LM_FILES
LM_W = (2, 7, 33, 64, 100, 127, 128)
LM_BUDGET = 150000                          # ... of the scored restatements, which take 6 to 16 us each
LMWT, WIP, OOV = (0.0, 0.7, 2.0), (0.0, 0.4), (-1.3, -1000.0)
GREEDY_V = (2, 63, 64, 65, 1025)
GREEDY_T = (1, 2, 63, 64, 65, 257)
GREEDY_DTYPES = ("f32", "f64", "f16", "bf16")
FAMILIES = {"plain": 132, "long": 6, "lm": 28, "lex": 28, "greedy": 30}
SEARCHES = ("plain", "long", "lm", "lex")   # the families with a beam (and a margin)
SEED0 = {"plain": 45000, "long": 46000, "lm": 47000, "lex": 48000, "greedy": 49000}
MIN_GAP = LR.MIN_GAP
LEFT_OUT_CAP = 0.10                         # of a family's utterances, for margin (gram_lexicon_ref.LEFT_OUT's cap)
LEFT_OUT = {"plain": ((115, 0),), "long": (), "lm": (), "lex": ()}    # (seed, utterance) below MIN_GAP (the CPU test recomputes them)
MASK_SHARE = AF.MASK_SHARE
K_MAX_W, K_MAX_PAIRS = 128, 131072          # include/e2e_ctc.h: e2e_gram_beam_max_width = min(128, 131072 / V)


def max_width(V):
    return min(K_MAX_W, K_MAX_PAIRS // V)


# ---- tables -----------------------------------------------------------------------------------------------------------------
def _capacity(R, k):
    """How many distinct grams of order k a draw may ask random_table for (it rejects repeats: well below all of them)."""
    n = (R - 1) ** k
    return n if n <= 4 else int(0.6 * n)


def _counts(R, V, kind):
    """random_table's arguments for V - R grams of this kind, or None where they do not fit."""
    n = V - R
    if n == 0:
        return (), ()
    if kind == "order2":
        counts, extra = (n,), ()
    elif kind == "order3":
        n3 = max(1, n // 3)
        counts, extra = (n - n3, n3), ()
    else:
        extra = (4, 5, 6, 7, 8) if n >= 12 else (8,)
        rest = n - len(extra)
        if rest < 0:
            return None
        n3 = rest // 3
        counts = (rest - n3, n3)
    return (counts, extra) if all(c <= _capacity(R, k) for k, c in enumerate(counts, start=2)) else None


def draw_table(rng, V, kind):
    """-> (R, label2ids): unigrams only (R = V), or the smallest R (plus a few) whose grams of this kind fill V columns."""
    if kind == "unigrams" or V == 2:
        return V, {}
    R = next(r for r in range(2, V + 1) if _counts(r, V, kind) is not None)
    R = min(V - 1, R + int(rng.integers(0, 6))) if R < V else R
    while _counts(R, V, kind) is None:
        R -= 1
    counts, extra = _counts(R, V, kind)
    l2i, total = DR.random_table(rng, R, *counts, extra=extra)
    assert total == V
    return R, l2i


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def log_softmax32(x):
    """The f32 rounding of the f64 log-softmax of f32 logits: what both calls are given."""
    return DR.log_softmax(x.astype(np.float64)).astype(np.float32)


def emissions(rng, B, T, V, scale, masked, blank_frame=None):
    """Log-probabilities (B,T,V) f32 of N(0,1) logits times `scale`; blank_frame: that frame's blank logit is raised by 40 (what
    is left of every other column is below any member's share).  masked: MASK_SHARE of the emissions are -inf, in every
    utterance but one when there are several (a small table's beam dies of it, and every other time one frame of another
    utterance is masked throughout: the one left alone is the living one beside it)."""
    x = (rng.standard_normal((B, T, V)) * scale).astype(np.float32)
    if blank_frame is not None:
        x[:, blank_frame, 0] += 40.0
    lp = log_softmax32(x)
    if masked:
        mask = rng.random((B, T, V)) < MASK_SHARE
        if B > 1:
            alone = int(rng.integers(B))
            mask[alone] = False
            if rng.integers(2):                 # ... and dies for certain of a frame that is masked throughout
                mask[(alone + 1) % B, int(rng.integers(T))] = True
        lp[mask] = -np.inf
    return lp


def lengths(rng, B, T, beyond=False):
    """Ragged lengths: one utterance at T, the others 0, 1, T or anything between (beyond: one time in eight, one at T + 1)."""
    full = int(rng.integers(B))
    xl = [T if b == full else (0, 1, T, int(rng.integers(0, T + 1)))[int(rng.integers(4))] for b in range(B)]
    if beyond and B > 1 and int(rng.integers(8)) == 0:
        xl[(full + 1) % B] = T + 1
    return xl


def call_shape(rng):
    return {"time_major": bool(rng.integers(2)), "strided": bool(rng.integers(2)), "cpu": bool(rng.integers(4) == 0),
            "keep_on_device": bool(rng.integers(2))}


def draw_nbest(rng, W):
    return int(rng.integers(1, W + 1)) if rng.integers(2) else None


def draw_plain(seed):
    rng = np.random.default_rng(SEED0["plain"] + seed)
    V, w = PLAIN_V[seed % len(PLAIN_V)], PLAIN_W[seed % len(PLAIN_W)]
    c = SimpleNamespace(family="plain", seed=seed, V=V, W=max_width(V) if w == "cap" else min(w, max_width(V)), at_cap=w == "cap")
    c.kind = PLAIN_KINDS[(seed // len(PLAIN_V)) % len(PLAIN_KINDS)]
    c.R, c.l2i = draw_table(rng, V, c.kind)
    c.dtype = ("f32", "f64")[(seed // 2) % 2]
    pairs = c.W * V
    B = int(rng.integers(1, 5 if pairs <= 40000 else 3))
    t_max = max(1, min(20 if c.W >= 100 else 30, PLAIN_BUDGET // pairs + 1))
    T = int(rng.integers((t_max + 1) // 2, t_max + 1))
    c.scale = PLAIN_SCALES[int(rng.integers(3))]
    c.masked = bool(rng.integers(4) == 0)
    c.lens = lengths(rng, B, T, beyond=True)
    c.x = emissions(rng, B, T, V, c.scale, c.masked)
    c.shape = call_shape(rng)
    c.nbest = draw_nbest(rng, c.W)
    c.raw = seed % 4 == 1                       # through the C call, into buffers of garbage
    return c


def draw_long(seed):
    rng = np.random.default_rng(SEED0["long"] + seed)
    c = SimpleNamespace(family="long", seed=seed, V=(21, 33)[seed % 2], W=int(rng.integers(2, 9)), at_cap=False, masked=False)
    c.kind = ("order3", "order8")[(seed // 2) % 2]
    c.R, c.l2i = draw_table(rng, c.V, c.kind)
    c.dtype = ("f32", "f64")[(seed // 3) % 2]
    T = int(rng.integers(300, 701))
    c.scale = LONG_SCALES[seed % 3]
    c.lens = [T, 1] if rng.integers(2) else [1, T]
    c.x = emissions(rng, 2, T, c.V, c.scale, False)
    c.shape = call_shape(rng)
    c.nbest = draw_nbest(rng, c.W)
    c.raw = seed % 4 == 1
    return c


def _scored(family, seed):
    """What lm and lex share: the model, the labels, the table, the knobs, the inputs."""
    rng = np.random.default_rng(SEED0[family] + seed)
    c = SimpleNamespace(family=family, seed=seed, at_cap=False)
    c.model = LM_FILES[seed % len(LM_FILES)]
    c.W = LM_W[seed % len(LM_W)]
    c.dtype = ("f32", "f64")[(seed // 2) % 2]
    chars = list(AF.model_chars(c.model))
    c.upper = bool(rng.integers(2))
    if c.upper:
        chars = [s.upper() for s in chars]
    c.case_sensitive = bool(rng.integers(2))
    space = int(rng.integers(len(chars) + 1)) if rng.integers(4) else -1
    if space >= 0:
        chars.insert(space, " ")
    c.labels = ["_"] + chars
    c.space = space + 1 if space >= 0 else -1   # the space's base id
    c.R = R = len(c.labels)
    c.big = seed % 9 == 4                       # a table of some 200 columns (over the larger alphabets)
    n2 = int(rng.integers(1, min(30, _capacity(R, 2)) + 1))
    n3 = int(rng.integers(1, min(30, _capacity(R, 3)) + 1))
    if c.big:
        n2, n3 = _capacity(R, 2), min(int(rng.integers(120, 161)), _capacity(R, 3))
    extra = ((4,), (4, 6), (8,), (5, 8))[int(rng.integers(4))]
    l2i, V = DR.random_table(rng, R, n2, n3, extra=extra)
    if c.space >= 0:                            # an inner, a leading and a trailing space
        a, b = (int(v) for v in rng.choice([i for i in range(1, R) if i != c.space], size=2))
        for g in ([a, c.space, b], [c.space, a], [b, c.space]):
            if g not in l2i.values():
                l2i[V] = g
                V += 1
    c.l2i, c.V = l2i, V
    B = int(rng.integers(1, 4 if c.W < 64 else 3))
    t_max = max(3, min(20 if c.W >= 100 else 24, LM_BUDGET // (c.W * V) + 1))
    T = int(rng.integers((t_max + 1) // 2, t_max + 1))
    c.scale = (1.0, 2.0, 8.0)[int(rng.integers(3))]
    c.lmwt, c.wip, c.oov = LMWT[int(rng.integers(3))], WIP[int(rng.integers(2))], OOV[int(rng.integers(2))]
    c.masked = bool(rng.integers(4) == 0)
    c.blank_frame = int(rng.integers(2, T)) if T > 2 and rng.integers(3) == 0 else None
    c.lens = lengths(rng, B, T)
    c.x = emissions(rng, B, T, V, c.scale, c.masked, c.blank_frame)
    c.shape = call_shape(rng)
    c.nbest = draw_nbest(rng, c.W)
    c.raw = seed % 4 == 1
    c.words, c.restricted = None, False
    # a frame of one column, under the wide beams of every other seed: the blank and every column but one letter's are -inf, so
    # most members of a full beam stay with a total of zero -- they are no candidates and no part of the floor filter's
    # n_stay -- while the few that end in that letter live on a run, and new members rank below the least of them
    c.sparse_frame = c.sparse_col = None
    if c.W >= 100 and seed % 2 == 0 and T > 4 and c.blank_frame != 3 + seed % 2:
        c.sparse_frame = 3 + seed % 2
        c.sparse_col = next(i for i in range(1 + seed % (R - 1), 2 * R) if 1 <= i % R != c.space) % R
        keep = c.x[:, c.sparse_frame, c.sparse_col].copy()
        c.x[:, c.sparse_frame, :] = -np.inf
        c.x[:, c.sparse_frame, c.sparse_col] = np.where(np.isfinite(keep), keep, np.float32(-1.0))
    return c, rng


def draw_lm(seed):
    c, rng = _scored("lm", seed)
    c.timesteps = bool(rng.integers(2))
    if seed % 5 == 3:                           # no model: wip alone
        c.model, c.lmwt = None, 0.0
    return c


def draw_lex(seed):
    c, rng = _scored("lex", seed)
    c.timesteps, c.restricted = True, True
    if c.upper:                                 # (upper-case labels spell no word of a case-sensitive vocabulary)
        c.case_sensitive = False
    if seed % 2:                                # a word list drawn from the model's words: lmwt and oov_penalty count as 0
        words = arpa_words(os.path.join(LR.GOLDEN, c.model))
        n = int(rng.integers(min(3, len(words)), len(words) + 1))
        c.words = sorted(str(w) for w in rng.choice(words, size=n, replace=False))
        c.lmwt, c.oov = 0.0, 0.0
    return c


def draw_greedy(seed):
    rng = np.random.default_rng(SEED0["greedy"] + seed)
    V, T = GREEDY_V[seed % len(GREEDY_V)], GREEDY_T[seed % len(GREEDY_T)]
    c = SimpleNamespace(family="greedy", seed=seed, V=V, dtype=GREEDY_DTYPES[(seed // 3) % 4])
    c.kind = PLAIN_KINDS[(seed // len(GREEDY_V)) % len(PLAIN_KINDS)]
    c.R, c.l2i = draw_table(rng, V, c.kind)
    B = int(rng.integers(1, 5))
    c.x = (rng.standard_normal((B, T, V)) * 2.0).astype(np.float32)
    # exactly tied maxima, in a third of the frames: two columns share a value above all the others.  (16-bit inputs tie on
    # their own as well; a multiple of 1/8 below 16 is exact in f16 and bf16, so these survive the conversion)
    c.tied = rng.random((B, T)) < 1.0 / 3
    for b, t in zip(*np.nonzero(c.tied)):
        top = math.ceil(float(c.x[b, t].max())) + 1.0 + float(rng.integers(0, 8)) / 8.0
        assert top < 16.0
        c.x[b, t, rng.choice(V, size=2, replace=False)] = top
    c.lens = [int(n) for n in rng.integers(1, T + 1, size=B)]
    c.lens[int(rng.integers(B))] = T
    c.shape = {"time_major": bool(rng.integers(2)), "strided": bool(rng.integers(2))}
    return c


@functools.lru_cache(maxsize=None)
def draw(family, seed):
    return {"plain": draw_plain, "long": draw_long, "lm": draw_lm, "lex": draw_lex, "greedy": draw_greedy}[family](seed)


def frames_of(c, b):
    """The frames utterance b is searched over: the header clamps a length to 0 .. T."""
    return max(0, min(c.lens[b], c.x.shape[1]))


# ---- the restatements -------------------------------------------------------------------------------------------------------
class trace:
    """Records, while it is open, the candidate list every frame's cut ranks (the argument of the restatements' `_ranked`,
    which are not edited): per call the ranked sequences.  The plain restatement ranks its result once more at the end."""

    def __init__(self):
        self.calls = []

    def __enter__(self):
        self.saved = (DR._ranked, LR._ranked)

        def wrap(fn):
            def ranked(rows):
                out = fn(rows)
                self.calls.append([r[1] for r in out])
                return out
            return ranked
        DR._ranked, LR._ranked = wrap(DR._ranked), wrap(LR._ranked)
        return self

    def __exit__(self, *exc):
        DR._ranked, LR._ranked = self.saved


def fields_and_rule(c):
    """The language model's and the vocabulary's side of a scored case -> (gram_decode_lm_ref.Fields, Rule or None)."""
    if c.words is not None:
        F = LR.Fields(c.labels, WordListLM(c.words, c.case_sensitive), c.case_sensitive, 0.0, c.wip, 0.0)
        return F, XR.Rule(c.labels, Lexicon(c.words, c.case_sensitive))
    lm = LR.oracle_lm(c.model) if c.model else None
    F = LR.Fields(c.labels, lm, c.case_sensitive, c.lmwt, c.wip, c.oov)
    rule = XR.Rule(c.labels, Lexicon(arpa_words(os.path.join(LR.GOLDEN, c.model)), c.case_sensitive)) if c.restricted else None
    return F, rule


def final_gap(scores, relative):
    """The smallest gap between neighbours of a final ranking whose scores differ (exact ties are decided by key)."""
    gap = math.inf
    for hi, lo in zip(scores, scores[1:]):
        if hi != lo:
            gap = min(gap, -math.expm1(lo - hi) if relative else hi - lo)
    return gap


def search(c, b, n_frames=None, restricted=None):
    """The restatement on utterance b (its first n_frames frames) -> (ranking, margin, members per frame).  ranking: dicts of
    ids, total, ac and -- scored -- lm, words, oov, frames.  members per frame: the sequences kept by every cut, in rank order."""
    n = frames_of(c, b) if n_frames is None else n_frames
    lp = c.x[b, :n].astype(np.float64)
    grams = GR.grams_of(c.R, c.V, c.l2i)
    with trace() as tr:
        if c.family in ("plain", "long"):
            got, gap = DR.beam_search(lp, grams, c.W)
            ranking = [dict(ids=seq, total=s, ac=s) for seq, s in got]
            gap = min(gap, final_gap([r["total"] for r in ranking], relative=True))
        else:
            F, rule = fields_and_rule(c)
            if c.restricted or c.timesteps:     # (without a rule: gram_decode_lm_ref's search, and the frames)
                ranking, gap = XR.beam_search(lp, grams, F, rule if restricted in (None, True) else None, c.W)
            else:
                ranking, gap = LR.beam_search(lp, grams, F, c.W)
    return ranking, gap, [calls[:c.W] for calls in tr.calls[:n]]


@functools.lru_cache(maxsize=None)
def reference(family, seed):
    """[(ranking, margin, members per frame) per utterance] of a case of SEARCHES, once per process."""
    c = draw(family, seed)
    return [search(c, b) for b in range(len(c.lens))]


def compared(family, seed, b):
    """Is the utterance compared on the GPU?  Its cuts and its final order are at least MIN_GAP apart."""
    return reference(family, seed)[b][1] >= MIN_GAP


def utterances(family):
    return [(s, b) for s in range(FAMILIES[family]) for b in range(len(draw(family, s).lens))]


def facts(family, seed):
    """What the coverage test counts, of the compared utterances of a case: per utterance the final members, the frames with a
    full beam, and per frame behind the first how many members are new and how many stayed."""
    c = draw(family, seed)
    ref = reference(family, seed)
    f = SimpleNamespace(case=c, utts=[])
    for b, (ranking, gap, members) in enumerate(ref):
        if gap < MIN_GAP:
            continue
        u = SimpleNamespace(b=b, frames=frames_of(c, b), ranking=ranking, gap=gap, n=len(ranking))
        u.full_frames = sum(len(m) == c.W for m in members)
        u.moves = []                            # (members before, stayed, new) per frame behind the first
        for was, now in zip(members, members[1:]):
            stay = len(set(was) & set(now))
            u.moves.append((len(was), stay, len(now) - stay))
        # the sparse frame under a full beam: members that end in another letter are dead for certain, and the floor filter is
        # put to the test if a new member ranks below the least staying one (or none stays while new ones come)
        u.dead_stays_in_a_full_beam = False
        t = getattr(c, "sparse_frame", None)
        if t is not None and len(members) > t:
            was, now = members[t - 1], members[t]
            dead = [s for s in was if s[-1:] != (c.sparse_col,)]
            stays = [i for i, s in enumerate(now) if s in set(was)]
            u.dead_stays_in_a_full_beam = bool(len(was) == c.W and dead and now and (not stays or stays[-1] < len(now) - 1))
        f.utts.append(u)
    alive = [u for u in f.utts if u.frames > 0]
    f.full = any(u.n == c.W for u in alive)
    f.partial = any(0 < u.n < c.W for u in alive)
    f.dead_beside_living = any(u.n == 0 for u in alive) and any(u.n > 0 for u in alive)
    return f
