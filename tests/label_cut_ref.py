"""Per-frame label pruning (TEST INFRASTRUCTURE ONLY): a numpy f64 restatement of the definition in include/e2e_ctc.h
(e2e_ctc_label_cut, steps 1 to 5), the pruned search as a restatement (CutSearch: lexicon_ref.Search whose step loops over the
frame's kept ids), and the seeded cases that tests/test_label_cut_cpu.py (margins, caps), tests/test_gpu_label_cut.py (the
selection kernel) and tests/test_gpu_ctc_beam_cut.py (the pruned search) share.

P_j is a sequential f64 sum here and a scan of fixed shape on the GPU, and exp() may differ by an ulp: a frame one of whose P_j
lies within BOUNDARY of cutoff_prob (relative) may keep one label more or fewer on the GPU.  Such frames are not compared
(LEFT_OUT_FRAMES; an utterance of the search cases with such a frame, or with a search margin below ctc_beam_fuzz_util.MIN_GAP:
LEFT_OUT_UTTS); the CPU test recomputes both lists and holds them to LEFT_OUT_CAP.  BOUNDARY = 1e-9 is some 10^6 times the
error of a sum of at most 1024 terms, so nothing else is uncertain.
"""
import functools
import os
from types import SimpleNamespace

import numpy as np

import ctc_beam_fuzz_util as F
import lexicon_ref as LR
import transcription_ref as TR

BOUNDARY = 1e-9
LEFT_OUT_CAP = F.LEFT_OUT_CAP
CUT_MAX = 1024                                   # e2e_ctc_label_cut_max()


# ---- the definition -----------------------------------------------------------------------------------------------------------
def _sums(row, cutoff_top_n):
    """(the first K labels of the order, P_1 .. P_K)."""
    lp = np.asarray(row, dtype=np.float64)
    lp = np.where(np.isnan(lp), -np.inf, lp)
    V = lp.shape[0]
    order = np.lexsort((np.arange(V), -lp))      # lp descending, ties by id ascending
    first = order[:min(int(cutoff_top_n), V)]
    return first, np.cumsum(np.exp(lp[first]))


def cut_frame(row, blank, cutoff_top_n, cutoff_prob):
    """The kept labels of one frame, ascending."""
    first, P = _sums(row, cutoff_top_n)
    k = len(first)
    if cutoff_prob < 1.0:
        hit = np.nonzero(P >= cutoff_prob)[0]
        if len(hit):
            k = int(hit[0]) + 1
    return sorted(set(int(c) for c in first[:k]) | {int(blank)})


def boundary_margin(row, cutoff_top_n, cutoff_prob):
    """min_j |P_j - cutoff_prob| / cutoff_prob; inf when cutoff_prob == 1 (step 3 is skipped: nothing is compared)."""
    if cutoff_prob >= 1.0:
        return np.inf
    _, P = _sums(row, cutoff_top_n)
    return float(np.min(np.abs(P - cutoff_prob)) / cutoff_prob)


def cut(lp, lens, blank, cutoff_top_n, cutoff_prob):
    """e2e_ctc_label_cut's outputs for lp (B,T,V): ids (B,T,K+1) int32, -1 behind a frame's labels and in the frames at or past
    an utterance's length, n (B,T) int32, and the frames' boundary margins (B,T), inf past the length."""
    B, T, V = lp.shape
    K = min(int(cutoff_top_n), V)
    ids = np.full((B, T, K + 1), -1, np.int32)
    n = np.zeros((B, T), np.int32)
    margin = np.full((B, T), np.inf)
    for b in range(B):
        for t in range(max(0, min(int(lens[b]), T))):
            kept = cut_frame(lp[b, t], blank, cutoff_top_n, cutoff_prob)
            ids[b, t, :len(kept)] = kept
            n[b, t] = len(kept)
            margin[b, t] = boundary_margin(lp[b, t], cutoff_top_n, cutoff_prob)
    return ids, n, margin


# ---- the pruned search --------------------------------------------------------------------------------------------------------
class _CutStep:
    """step() of lexicon_ref.Search restricted to the frame's kept labels: a label outside the set creates no child, gives no
    share to a living child and no repeated-label share to the member.  Everything else is inherited, margins included."""
    cutoff_top_n, cutoff_prob = None, 1.0
    min_boundary = np.inf                        # the smallest boundary margin of the frames searched

    def set_cut(self, cutoff_top_n, cutoff_prob):
        self.cutoff_top_n, self.cutoff_prob = cutoff_top_n, cutoff_prob
        return self

    def step(self, beam, row, t=-1):
        self.t, self.row = t, row
        top_n = len(row) if self.cutoff_top_n is None else self.cutoff_top_n
        kept = cut_frame(row, self.blank, top_n, self.cutoff_prob)
        self.min_boundary = min(self.min_boundary, boundary_margin(row, top_n, self.cutoff_prob))
        fresh = []
        for ch in kept:                                                  # ascending: the order the search expands in
            cur = row[ch]
            for p in beam:
                if ch == self.blank:
                    p.pb = LR.lse(p.pb, cur + LR.lse(p.prev_pnb, p.prev_pb))
                    continue
                q, is_new = self.next_prefix(p, ch)
                if is_new:
                    fresh.append(q)
                if ch == p.last_char:
                    if q is not None:
                        q.pnb = LR.lse(q.pnb, cur + p.prev_pb)
                    p.pnb = LR.lse(p.pnb, cur + p.prev_pnb)
                elif q is not None:
                    q.pnb = LR.lse(q.pnb, cur + LR.lse(p.prev_pnb, p.prev_pb))
        beam = beam + fresh
        for p in beam:
            p.prev_pb, p.prev_pnb, p.pb, p.pnb = p.pb, p.pnb, LR.NEG_INF, LR.NEG_INF
        if len(beam) > self.W:
            beam = self.ranked(beam, cut=True)[: self.W]
        return beam


class CutSearch(_CutStep, LR.Search):
    pass


class CutTransSearch(_CutStep, TR.Search):
    """... over a transcription lexicon (transcription_ref.Search)."""


# ---- the selection kernel's cases (tests/test_gpu_label_cut.py) -------------------------------------------------------------------
CUT_V = (2, 5, 29, 64, 65, 257, 1000, 8000)
CUT_DTYPES = ("f32", "f64", "f16", "bf16")
CUT_PROBS = (1.0, 0.999999, 0.99, 0.9, 0.5, 1e-6)
CUT_VIEWS = ("contiguous", "time_major", "strided")


def cut_top_ns(V):
    """cutoff_top_n in {1, 2, 40, V, 1024 where V allows}: a K above CUT_MAX is refused, so V = 8000 goes without V."""
    return tuple(dict.fromkeys(n for n in (1, 2, 40, V, 1024) if min(n, V) <= CUT_MAX and (n != 1024 or V >= 1024)))


def cut_shape(V):
    return (2, 16) if V == 8000 else (3, 24) if V == 1000 else (3, 48)


@functools.lru_cache(maxsize=None)
def cut_input(V, dtype):
    """(lp (B,T,V) f32 holding numbers of `dtype` (f64: the f32 ones), lens).  Randn logits at scales 1 and 4 through a
    log-softmax; the first frames of utterance 0 are the edges: an all-equal row, a one-hot row (P_1 = 1), a row on a grid of
    0.5 (bit-equal columns straddling every place), a row half -inf, a row with NaN, a row whose ties are at the top."""
    B, T = cut_shape(V)
    rng = np.random.default_rng(71000 + V)
    x = rng.standard_normal((B, T, V)).astype(np.float32)
    x[:, T // 2:] *= np.float32(4.0)
    lp = F.GF.log_softmax32(x)
    lp[0, 0] = np.float32(np.log(1.0 / V))
    hot = int(rng.integers(V))
    lp[0, 1] = -np.inf
    lp[0, 1, hot] = 0.0
    lp[0, 2] = np.round(lp[0, 2] * 2.0) / 2.0
    lp[0, 3, rng.random(V) < 0.5] = -np.inf
    lp[0, 4, int(rng.integers(V))] = np.nan
    top = np.argsort(-lp[0, 5])[:min(V, 5)]
    lp[0, 5, top] = lp[0, 5, top[0]]
    lp = F.rounded(lp, dtype)
    lens = [T, 1] if B == 2 else [T, 0, 1]
    return lp, lens


def cut_blank(V, which):
    """The blank of a combination: column 0, column V - 1, or `low` -- the column that utterance 0 never has among its top."""
    return (0, V - 1, "low")[which % 3]


def cut_case(V, dtype, top_n, prob):
    """One call of the selection test: the input with the combination's blank (a `low` blank: that column lowered by 30 in
    every frame, so it is never among the top and always added), its view, and the restatement."""
    lp, lens = cut_input(V, dtype)
    i = cut_top_ns(V).index(top_n) * len(CUT_PROBS) + CUT_PROBS.index(prob)
    blank = cut_blank(V, i)
    if blank == "low":
        blank = V // 2
        lp = lp.copy()
        lp[:, :, blank] = F.rounded(np.where(np.isfinite(lp[:, :, blank]), lp[:, :, blank] - np.float32(30.0),
                                             lp[:, :, blank]).astype(np.float32), dtype)
    ids, n, margin = cut(lp.astype(np.float64), lens, blank, top_n, prob)
    return SimpleNamespace(lp=lp, lens=lens, blank=blank, view=CUT_VIEWS[(i // 3) % 3], ids=ids, n=n, margin=margin)


def cut_left_out(V, dtype):
    """[(top_n, prob, b, t)] of the family's frames below BOUNDARY, and the number of frames compared or not."""
    out, frames = [], 0
    for top_n in cut_top_ns(V):
        for prob in CUT_PROBS:
            c = cut_case(V, dtype, top_n, prob)
            frames += int(sum(max(0, min(n, c.lp.shape[1])) for n in c.lens))
            out += [(top_n, prob, int(b), int(t)) for b, t in zip(*np.nonzero(c.margin < BOUNDARY))]
    return out, frames


# (V, dtype) -> the frames below BOUNDARY as (top_n, prob, b, t): sharp frames (the logits at scale 4) whose tail
# probabilities are around 1e-9, so that the sums near 0.999999 lie that close together (the CPU test recomputes them)
_NEAR = {64: ((64, 0.999999, 0, 42),), 65: ((65, 0.999999, 0, 34),), 257: ((257, 0.999999, 0, 40),),
         1000: ((1000, 0.999999, 0, 19), (1000, 0.999999, 0, 20))}
LEFT_OUT_FRAMES = {(V, dtype): frames for V, frames in _NEAR.items() for dtype in ("f32", "f64")}


# ---- the pruned search's cases (tests/test_gpu_ctc_beam_cut.py) -------------------------------------------------------------------
SEARCH_V = (6, 29, 300)
SEARCH_W = (2, 8, 32)
VARIANTS = ("plain", "lm", "lex_lm", "lex_words", "trans")
MODEL = "tiny_3gram.arpa"
SEARCH_SHAPE = {6: (4, 40, [40, 0, 1, 37]), 29: (3, 30, [30, 1, 0]), 300: (2, 12, [12, 7])}


def search_cuts(V):
    return ((1, 1.0), (3, 1.0), (V // 2, 0.9), (40, 0.99))


@functools.lru_cache(maxsize=None)
def search_case(variant, V, W, ci):
    """A case as ctc_beam_fuzz_util's draws shape them (blank_case), with its cut."""
    rng = np.random.default_rng(72000 + 1000 * VARIANTS.index(variant) + 10 * V + W + 7 * ci)
    c = F.blank_case("cut_" + variant, ci, V=V, W=W, blank=0, dtype=("f32", "f64")[(ci + W) % 2], timesteps=True)
    c.cut = search_cuts(V)[ci]
    B, T, lens = SEARCH_SHAPE[V]
    c.scale = (1.0, 2.0)[ci % 2]
    c.wip = (0.0, 0.4)[(ci + W) % 2]
    word_cols = None
    if variant == "plain":
        c.labels = F.AF.plain_labels(V, V // 2)
    elif variant == "trans":
        toks = list(F.TOKENS[:4]) + [" "] + ["P%d" % i for i in range(V - 6)]
        c.labels = ["_"] + toks
        # homophones: a / ab share `A`, b / ba share `AH K`; a variant of ab; a word the model does not list is dropped
        c.entries = [("a", ["A"]), ("ab", ["A"]), ("b", ["AH", "K"]), ("ba", ["AH", "K"]), ("ab", ["A", "HK"]),
                     ("ba", ["K", "A"]), ("zz0", ["HK"])]
        c.model, c.restricted = MODEL, bool(ci % 2)
        c.lmwt, c.oov = (0.7, 2.0)[ci % 2], (-1.3, -1000.0)[(ci // 2) % 2]
        word_cols = list(range(1, 6))
    else:
        chars = list(F.AF.model_chars(MODEL)) + [" "] + [chr(0x100 + 2 * i) for i in range(V - 2 - len(F.AF.model_chars(MODEL)))]
        c.labels = ["_"] + chars
        c.model = MODEL if variant != "lex_words" else MODEL
        c.restricted = variant in ("lex_lm", "lex_words")
        c.lmwt, c.oov = (0.7, 2.0)[ci % 2], (-1.3, -1000.0)[(ci // 2) % 2]
        if variant == "lex_words":
            c.words = sorted(F.model_words(MODEL))[: 3]
            c.lmwt, c.oov = 0.0, 0.0
        word_cols = [i for i, s in enumerate(c.labels) if i and ord(s[0]) < 0x100]
    assert len(c.labels) == V, (variant, V, len(c.labels))
    c.x = F.emissions(rng, B, T, V, c.scale, False, c.dtype)
    c.lens = list(lens)
    if word_cols is not None and V > 6:
        F.favour(c, rng, word_cols)
    return c


def make_cut_search(c):
    if c.entries is not None:
        s = CutTransSearch(c.labels, c.blank, c.W, F.ref_lm(c), F.table_of(c), c.restricted, c.lmwt, c.wip, c.oov)
    else:
        lexicon = None
        if c.restricted:
            lexicon = LR.Lexicon(c.words if c.words is not None else F.model_words(c.model), c.case_sensitive)
        s = CutSearch(c.labels, c.blank, c.W, F.ref_lm(c), c.case_sensitive, c.lmwt, c.wip, c.oov, lexicon=lexicon)
    return s.set_cut(*c.cut)


@functools.lru_cache(maxsize=None)
def search_reference(variant, V, W, ci):
    """[(ranking, search margin, smallest boundary margin) per utterance], once per process."""
    c = search_case(variant, V, W, ci)
    out = []
    for b in range(len(c.lens)):
        n = F.frames_of(c, b)
        s = make_cut_search(c)
        ranking = s.run(c.x[b, :n].astype(np.float64), n)
        out.append((ranking, s.margin(), s.min_boundary))
    return out


def search_cases(variant):
    return [(V, W, ci) for V in SEARCH_V for W in SEARCH_W for ci in range(4)]


def search_compared(variant, V, W, ci, b):
    _, gap, boundary = search_reference(variant, V, W, ci)[b]
    return gap >= F.MIN_GAP and boundary >= BOUNDARY


def search_left_out(variant):
    """[(V, W, ci, b)] of the variant's utterances that are not compared, and the number of its utterances."""
    out, total = [], 0
    for V, W, ci in search_cases(variant):
        for b in range(len(search_case(variant, V, W, ci).lens)):
            total += 1
            if not search_compared(variant, V, W, ci, b):
                out.append((V, W, ci, b))
    return out, total


# variant -> the utterances left out (the CPU test recomputes them)
LEFT_OUT_UTTS = {v: () for v in VARIANTS}
