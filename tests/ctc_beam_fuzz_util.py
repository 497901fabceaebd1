"""The seeded cases of the CTC decoder's fuzz (TEST INFRASTRUCTURE ONLY), shared by tests/test_ctc_beam_fuzz_cpu.py (margins,
coverage), tests/test_gpu_ctc_beam_fuzz.py (the kernels) and tests/test_gpu_ctc_stream_fuzz.py (the stream).
draw(family, seed) is a pure function of its arguments.  Emissions are log-probabilities drawn in f32 (the f32 rounding of the
f64 log-softmax of f32 logits; masked ones set to -inf afterwards; for an f16 / bf16 case rounded once more to that type), so
that every call and the restatement see the same numbers.  reference(family, seed) runs the restatement (lexicon_ref.Search,
transcription_ref.Search) once per process and utterance, through a recording subclass that notes what the coverage test asks
of a search's frames (facts()).

Six families:
  plain   132 seeds: every pair of V in PLAIN_V and W in PLAIN_W (V by seed % 11, W by seed // 11; `fastcap` is the largest
          width the one-workgroup kernel takes at that alphabet, read off the workspace query), the blank at 0, at V - 1 or
          anywhere, a space or none, wip, B 1..4, ragged lengths with 0, 1 and T, scales 1 / 3 / 10, one case in four masked,
          one in four with a tied frame (k bit-equal columns; where the general kernel runs and the alphabet allows it,
          k > 4 W + 64 of them at the last frame's maximum), dtype, call shape, nbest.  T <= PLAIN_BUDGET / (W V) + 1, at most 30
  long    6 seeds: T in 300..700, W <= 8, V in {5, 29}, B = 2 with one utterance of one frame, timesteps
  lm      36 seeds over the three ARPA models of tests/golden, each as it is or with one listed context removed (the id
          tables): labels are the characters of the model's words, lower or upper case, the space at a random place, and 0, 40
          or 300 padding labels that spell no word; W in LM_W; the knobs drawn; a fifth of the cases without a model
  lex     36 seeds: the lm draw restricted to the model's words or to a word list drawn from them, timesteps in every case, a
          quarter of the cases without a space label
  trans   36 seeds: transcription lexicons over the same models (transcription_ref.Table / Search): multi-character labels,
          variants, homophone keys of 2..4 words and one key with as many as the model allows (up to 16), entries whose word
          the model does not list, with a model, with its pruned variant and without one, restricted or not
  greedy  30 seeds: V in GREEDY_V, T in GREEDY_T, the four dtypes, constructed ties of the maximum, contiguous or a view with gaps

An utterance whose margin (lexicon_ref.Search.margin: the smallest positive gap at a cut, the smallest gap between neighbours
of the final ranking whose totals differ, for transcriptions the closest choice among homophones; 0 where an exact tie is not
the same arithmetic) is below MIN_GAP is not compared on the GPU: compared(); test_ctc_beam_fuzz_cpu.py holds each family to
at most LEFT_OUT_CAP of its utterances and LEFT_OUT to what it recomputes.
"""
import atexit
import functools
import math
import os
import shutil
import tempfile
import time
from types import SimpleNamespace

import numpy as np

import asg_beam_fuzz_util as AF
import gram_beam_fuzz_util as GF
import lexicon_ref as LR
import transcription_ref as TR
from asg_beam_util import MIN_GAP

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PLAIN_V = (2, 3, 4, 29, 53, 54, 55, 81, 82, 300, 1000)
PLAIN_W = (2, 3, 7, 33, 64, 100, "fastcap", "fastcap+1", 256, 257, 512)
PLAIN_BUDGET = 300000                       # (member, column) pairs of one utterance: the restatement takes some 2.5 us each
PLAIN_SCALES = (1.0, 3.0, 10.0)
PLAIN_WIP = (0.0, 0.4, 2.5)
PLAIN_DTYPES = ("f32", "f64", "f32", "f64", "f16", "bf16")
LM_FILES = AF.LM_FILES
LM_W = (2, 7, 33, 64, "fastcap", "fastcap+1", 128, 256, 512)
LM_PADS = (0, 40, 300)
LM_BUDGET = 100000                          # ... of the scored restatements, which take 3 to 7 us each
LMWT, WIP, OOV = (0.0, 0.7, 2.0), (0.0, 0.4), (-1.3, -1000.0)
GREEDY_V = (2, 29, 32, 64, 65, 8000)
GREEDY_T = (1, 63, 64, 65, 1023, 1025, 2047, 2048, 2049, 4097)
GREEDY_DTYPES = ("f32", "f64", "f16", "bf16")
FAMILIES = {"plain": 132, "long": 6, "lm": 36, "lex": 36, "trans": 36, "greedy": 30}
SEARCHES = ("plain", "long", "lm", "lex", "trans")
SEED0 = {"plain": 55000, "long": 56000, "lm": 57000, "lex": 58000, "trans": 59000, "greedy": 60000}
LEFT_OUT_CAP = 0.03                         # of a family's utterances, for margin (the ASG fuzz's cap)
LEFT_OUT = {"plain": ((52, 0), (53, 0), (53, 1), (53, 3), (78, 0), (101, 3)), "long": (), "lm": (), "lex": (), "trans": ()}    # (seed, utterance) below MIN_GAP (the CPU test recomputes them)
MASK_SHARE = AF.MASK_SHARE
TOKENS = ("A", "AH", "HK", "K", "B", "EH", "D")      # multi-character labels: `A HK` and `AH K` spell alike and differ


# ---- the host queries ---------------------------------------------------------------------------------------------------------
def takes_general(V, W, lm):
    from end2end_amd import _C
    return _C.ctc_beam_stream_workspace_bytes(1, V, W, bool(lm)) > 0


@functools.lru_cache(maxsize=None)
def max_width(V, lm):
    from end2end_amd import _C
    return _C.ctc_beam_max_width(V, bool(lm))


@functools.lru_cache(maxsize=None)
def fastcap(V, lm):
    """The largest width the one-workgroup kernel takes at this alphabet (the fit is monotone in the width)."""
    lo, hi = 0, max_width(V, lm)
    while lo < hi:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if not takes_general(V, mid, lm) else (lo, mid - 1)
    return lo


def width(w, V, lm):
    w = fastcap(V, lm) if w == "fastcap" else fastcap(V, lm) + 1 if w == "fastcap+1" else w
    return max(2, min(w, max_width(V, lm)))


# ---- models -------------------------------------------------------------------------------------------------------------------
_tmp = None


def pruned_text(model):
    """The ARPA file with one listed context removed: the first (n-1)-gram line, n the model's order, that is the context of an
    n-gram (which stays: its context is then unlisted, and the model takes the id tables)."""
    lines = open(os.path.join(GOLDEN, model), encoding="utf-8").read().split("\n")
    marks = [i for i, l in enumerate(lines) if l.startswith("\\") and l.endswith("-grams:")]
    n = len(marks)
    top = {tuple(l.split("\t")[1].split()[:-1]) for l in lines[marks[-1] + 1:] if "\t" in l}
    for i in range(marks[-2] + 1, marks[-1]):
        f = lines[i].split("\t")
        if len(f) >= 2 and tuple(f[1].split()) in top:
            del lines[i]
            break
    else:
        raise AssertionError(model)
    j = next(k for k, l in enumerate(lines) if l.startswith("ngram %d=" % (n - 1)))
    lines[j] = "ngram %d=%d" % (n - 1, int(lines[j].split("=")[1]) - 1)
    return "\n".join(lines)


def model_path(model, pruned=False):
    """The model's file; a pruned variant is written to a temporary directory once per process."""
    global _tmp
    if not pruned:
        return os.path.join(GOLDEN, model)
    if _tmp is None:
        _tmp = tempfile.mkdtemp(prefix="ctc_fuzz_lm_")
        atexit.register(shutil.rmtree, _tmp, True)
    path = os.path.join(_tmp, "pruned_" + model)
    if not os.path.exists(path):
        with open(path, "w", encoding="utf-8") as f:
            f.write(pruned_text(model))
    return path


@functools.lru_cache(maxsize=None)
def oracle_lm(model, pruned):
    import oracle_lib as O
    return O.OracleLM(model_path(model, pruned))


@functools.lru_cache(maxsize=None)
def model_words(model):
    return tuple(LR.arpa_words(os.path.join(GOLDEN, model)))


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def rounded(lp, dtype):
    """f32 log-probabilities as the 16-bit case holds them (f32 / f64: unchanged)."""
    if dtype in ("f32", "f64"):
        return lp
    import torch
    return torch.from_numpy(lp).to(torch.float16 if dtype == "f16" else torch.bfloat16).float().numpy()


def emissions(rng, B, T, V, scale, masked, dtype, tie=None):
    """Log-probabilities (B,T,V) f32 of N(0,1) logits times `scale`.  tie = (frame, columns, at_max): those logits of that
    frame are made equal (above all the others if at_max) before the soft-max, so the log-probabilities are bit-equal.
    masked: MASK_SHARE of the emissions are -inf, in every utterance but one when there are several."""
    x = (rng.standard_normal((B, T, V)) * scale).astype(np.float32)
    if tie is not None:
        t, cols, at_max = tie
        x[:, t, cols] = (x[:, t].max(axis=1, keepdims=True) + np.float32(1.0)) if at_max else x[:, t, cols[:1]]
    lp = rounded(GF.log_softmax32(x), dtype)
    if masked:
        mask = rng.random((B, T, V)) < MASK_SHARE
        if B > 1:
            mask[int(rng.integers(B))] = False
        lp[mask] = -np.inf
    return lp


def draw_nbest(rng, W):
    return (None, 1, int(rng.integers(1, W + 1)))[int(rng.integers(3))]


def finish(c, rng, B, T, tie=None):
    """What every search case ends with: lengths, emissions, call shape, nbest, the C call and its max_out."""
    c.lens = GF.lengths(rng, B, T)
    c.x = emissions(rng, B, T, c.V, c.scale, c.masked, c.dtype, tie)
    c.shape = GF.call_shape(rng)
    c.nbest = draw_nbest(rng, c.W)
    c.raw = c.seed % 4 == 1                     # through the C call, into buffers of garbage
    c.short_out = bool(c.raw and rng.integers(3) == 0)       # ... with max_out below the longest hypothesis
    return c


def blank_case(family, seed, **kw):
    c = SimpleNamespace(family=family, seed=seed, model=None, pruned=False, case_sensitive=True, lmwt=0.0, oov=0.0, wip=0.0,
                        restricted=False, words=None, entries=None, masked=False, tie=None, overflow=False, timesteps=False,
                        pad=0, upper=False)
    vars(c).update(kw)
    return c


def draw_plain(seed):
    rng = np.random.default_rng(SEED0["plain"] + seed)
    V = PLAIN_V[seed % len(PLAIN_V)]
    c = blank_case("plain", seed, V=V, W=width(PLAIN_W[(seed // len(PLAIN_V)) % len(PLAIN_W)], V, False))
    c.dtype = PLAIN_DTYPES[seed % len(PLAIN_DTYPES)]
    if c.dtype in ("f16", "bf16") and (seed // 6) % 4:                    # 16-bit sums lie on a grid and tie exactly, the more
        c.dtype = "f32"                                                   # the longer: one case in twelve, of at most 3 frames
    c.blank = (0, V - 1, int(rng.integers(V)))[int(rng.integers(3))]
    space = int(rng.integers(V)) if rng.integers(2) else -1
    c.labels = AF.plain_labels(V, -1 if space == c.blank else space)
    c.wip = PLAIN_WIP[int(rng.integers(3))]
    pairs = c.W * V
    B = int(rng.integers(1, 5 if pairs <= 40000 else 3))
    t_max = max(1, min(30, PLAIN_BUDGET // pairs + 1))
    T = int(rng.integers((t_max + 1) // 2, t_max + 1))
    if c.dtype in ("f16", "bf16"):
        T = min(T, 3)
    c.scale = PLAIN_SCALES[int(rng.integers(3))]
    c.masked = seed % 4 == 3
    c.timesteps = bool(rng.integers(2))
    tie = None
    if seed % 4 == 2:
        general = takes_general(V, c.W, False)
        if general and V - 1 > 4 * c.W + 64:    # more columns at the maximum than the pre-selection's list holds: the last frame
            k = int(rng.integers(4 * c.W + 65, V))
            cols = [i for i in rng.permutation(V) if i != c.blank][:k]
            tie, c.overflow = (T - 1, [int(i) for i in cols], True), True
            c.scale = 1.0                       # (sharp frames leave a member's blank share below f64's grain: its repeat ties its children)
        else:
            k = int(rng.integers(2, min(5, V) + 1))
            last = bool(rng.integers(2))
            tie = (T - 1 if last else int(rng.integers(T)), [int(i) for i in rng.permutation(V)[:k]], False)
    c.tie = tie
    return finish(c, rng, B, T, tie)


def draw_long(seed):
    rng = np.random.default_rng(SEED0["long"] + seed)
    V = (5, 29)[seed % 2]
    c = blank_case("long", seed, V=V, W=int(rng.integers(2, 9)), timesteps=True)
    c.dtype = ("f32", "f64")[(seed // 3) % 2]
    c.blank = (0, V - 1)[(seed // 2) % 2]
    space = int(rng.integers(V)) if rng.integers(2) else -1
    c.labels = AF.plain_labels(V, -1 if space == c.blank else space)
    c.wip = PLAIN_WIP[seed % 3]
    c.scale = PLAIN_SCALES[seed % 3]
    T = int(rng.integers(300, 701))
    finish(c, rng, 2, T)
    c.lens = [T, 1] if rng.integers(2) else [1, T]
    return c


def _scored(family, seed):
    """What lm and lex share: the model, the labels, the knobs, the inputs."""
    rng = np.random.default_rng(SEED0[family] + seed)
    c = blank_case(family, seed, blank=0)
    c.model = LM_FILES[seed % len(LM_FILES)]
    c.pruned = bool((seed // 3) % 2)
    c.dtype = ("f32", "f64")[(seed // 2) % 2]
    chars = list(AF.model_chars(c.model))
    c.upper = bool(rng.integers(2))
    if c.upper:
        chars = [s.upper() for s in chars]
    c.case_sensitive = bool(rng.integers(2))
    c.pad = LM_PADS[int(rng.integers(3))] if seed % 9 != 5 else 300       # (fastcap + 1 is wide at a small alphabet)
    chars += [chr(0x100 + 2 * i) for i in range(c.pad)]                   # capital letters with a diacritic: they spell no word
    no_space = family == "lex" and seed % 4 == 2
    if not no_space:
        chars.insert(int(rng.integers(len(chars) + 1)), " ")
    c.labels = ["_"] + chars
    c.V = len(c.labels)
    if family == "lm" and seed % 5 == 3:        # no model: wip alone
        c.model, c.pruned = None, False
    c.W = width(LM_W[seed % len(LM_W)], c.V, True)
    pairs = c.W * c.V
    B = int(rng.integers(1, 4 if pairs < 20000 else 3))
    t_max = max(3 if pairs <= LM_BUDGET else 2, min(24, LM_BUDGET // pairs + 1))
    T = int(rng.integers((t_max + 1) // 2 + 1, t_max + 1))
    c.scale = (1.0, 2.0, 8.0)[int(rng.integers(3))]
    c.lmwt, c.wip, c.oov = LMWT[int(rng.integers(3))], WIP[int(rng.integers(2))], OOV[int(rng.integers(2))]
    if c.model is None:
        c.lmwt = 0.0
    c.masked = bool(rng.integers(4) == 0)
    return c, rng, B, T


def favour(c, rng, cols, by=3.0):
    """Raise the log-probabilities of the labels the words are made of (and the space), so that words form: the emissions stay
    what every call sees, they only stop being normalised."""
    c.x[:, :, cols] += np.float32(by)
    c.x = rounded(c.x, c.dtype)


def draw_lm(seed):
    c, rng, B, T = _scored("lm", seed)
    c.timesteps = bool(rng.integers(2))
    finish(c, rng, B, T)
    if c.pad:
        favour(c, rng, [i for i, s in enumerate(c.labels) if i and ord(s[0]) < 0x100])
    return c


def draw_lex(seed):
    c, rng, B, T = _scored("lex", seed)
    c.timesteps, c.restricted = True, True
    if c.upper:                                 # (upper-case labels spell no word of a case-sensitive vocabulary)
        c.case_sensitive = False
    if seed % 2:                                # a word list drawn from the model's words: lmwt and oov_penalty count as 0
        words = list(model_words(c.model))
        n = int(rng.integers(min(3, len(words)), len(words) + 1))
        c.words = sorted(str(w) for w in rng.choice(words, size=n, replace=False))
        c.lmwt, c.oov, c.pruned = 0.0, 0.0, False
    return finish(c, rng, B, T)


def draw_trans(seed):
    rng = np.random.default_rng(SEED0["trans"] + seed)
    c = blank_case("trans", seed, blank=0, timesteps=bool(rng.integers(2)))
    c.model = LM_FILES[seed % len(LM_FILES)]
    kind = (seed // 3) % 3                      # the model, its pruned variant, no model
    c.pruned = kind == 1
    c.restricted = bool((seed // 9) % 2)
    c.dtype = ("f32", "f64")[(seed // 2) % 2]
    n_tok = int(rng.integers(4, len(TOKENS) + 1))
    toks = list(TOKENS[:n_tok])
    c.pad = 300 if seed % 6 >= 4 else 0         # padding labels that no transcription uses: the general kernel
    toks += ["P%d" % i for i in range(c.pad)]
    toks.insert(int(rng.integers(len(toks) + 1)), " ")
    c.labels = ["_"] + toks
    c.V = len(c.labels)
    letters = [t for t in toks if t in TOKENS]
    words = list(model_words(c.model))
    order = [str(w) for w in rng.permutation(words)]

    def key():
        return tuple(letters[int(i)] for i in rng.integers(len(letters), size=int(rng.integers(1, 4))))
    entries, used = [], set()
    big = key()                                 # one key with as many words as the model allows, up to 16
    used.add(big)
    n_big = min(16, len(words))
    entries += [(w, big) for w in order[:n_big]]
    rest = order[n_big:] + order[:n_big]
    i = 0
    while i < len(rest) and len(entries) < 60:
        k = key()
        if k in used:
            continue
        used.add(k)
        n = int(rng.integers(1, 5))             # a key of its own, or homophones of 2..4 words
        entries += [(w, k) for w in rest[i:i + n]]
        i += n
    for w in order[:4]:                         # variants: a second transcription of words listed already
        k = key()
        if k not in used:
            used.add(k)
            entries.append((w, k))
    for j in range(int(rng.integers(1, 4))):    # words the model does not list: dropped
        entries.insert(int(rng.integers(len(entries) + 1)), ("zz%d" % j, key()))
    c.entries = [(w, list(k)) for w, k in entries]
    if kind == 2:                               # no model: nothing is scored, the first listed word wins
        c.model, c.lmwt, c.oov = None, 0.0, 0.0
        c.entries = [e for e in c.entries if not e[0].startswith("zz")]
    c.W = (3, 10, 33, 100)[seed % 4]
    B = int(rng.integers(1, 4))
    T = int(rng.integers(6, 25)) if not c.pad else int(rng.integers(4, 9))
    c.scale = (1.0, 2.0, 4.0)[int(rng.integers(3))]
    c.wip = WIP[int(rng.integers(2))]
    if kind != 2:
        c.lmwt, c.oov = LMWT[int(rng.integers(3))], OOV[int(rng.integers(2))]
    c.masked = bool(rng.integers(6) == 0)
    finish(c, rng, B, T)
    if c.pad:
        favour(c, rng, [i for i, s in enumerate(c.labels) if s in TOKENS or s == " "], 4.0)
    return c


def draw_greedy(seed):
    rng = np.random.default_rng(SEED0["greedy"] + seed)
    V, T = GREEDY_V[seed % len(GREEDY_V)], GREEDY_T[seed % len(GREEDY_T)]
    if V == 8000:
        T = (1, 63, 64, 65)[(seed // 6) % 4]
    c = SimpleNamespace(family="greedy", seed=seed, V=V, dtype=GREEDY_DTYPES[(seed // 3) % 4])
    c.blank = (0, V - 1, int(rng.integers(V)))[seed % 3]
    B = int(rng.integers(1, 4))
    c.x = (rng.standard_normal((B, T, V)) * 2.0).astype(np.float32)
    # exactly tied maxima, in a third of the frames: two columns share a value above all the others.  (16-bit inputs tie on
    # their own as well; a multiple of 1/8 below 16 is exact in f16 and bf16, so these survive the conversion)
    c.tied = rng.random((B, T)) < 1.0 / 3
    for b, t in zip(*np.nonzero(c.tied)):
        top = math.ceil(float(c.x[b, t].max())) + 1.0 + float(rng.integers(0, 8)) / 8.0
        assert top < 16.0
        c.x[b, t, rng.choice(V, size=2, replace=False)] = top
    c.x = rounded(c.x, c.dtype)
    c.lens = [int(n) for n in rng.integers(1, T + 1, size=B)]
    c.lens[int(rng.integers(B))] = T
    c.shape = {"time_major": bool(rng.integers(2)), "strided": bool(seed % 2)}
    return c


@functools.lru_cache(maxsize=None)
def draw(family, seed):
    return {"plain": draw_plain, "long": draw_long, "lm": draw_lm, "lex": draw_lex, "trans": draw_trans,
            "greedy": draw_greedy}[family](seed)


def greedy_definition(c, b):
    """arg-max per frame (the first of equal maxima), repeats merged, blanks dropped."""
    am = c.x[b, :c.lens[b]].argmax(axis=1)
    keep = np.concatenate(([True], am[1:] != am[:-1])) & (am != c.blank)
    return am[keep].tolist()


# ---- the restatements -------------------------------------------------------------------------------------------------------
def recording(cls):
    """The restatement's class, noting per frame what the coverage test asks for (nothing it computes changes)."""
    class Recording(cls):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.sizes, self.q7, self.ninf_in_full = [], 0, 0

        def next_prefix(self, p, ch):
            q, new = super().next_prefix(p, ch)
            if q is not None and not new and id(q) not in self._beam_ids:
                self.q7 += 1                    # a pruned child that a descendant keeps alive, found again (Q7)
            return q, new

        def step(self, beam, row, t=-1):
            self._beam_ids = {id(p) for p in beam}
            out = super().step(beam, row, t)
            self.sizes.append(len(out))
            if len(out) == self.W and any(self.score(p) == LR.NEG_INF for p in out):
                self.ninf_in_full += 1
            return out
    return Recording


def ref_lm(c):
    """The language model's side of a case as the restatement takes it (None: no model)."""
    if c.family == "trans":
        return oracle_lm(c.model, c.pruned) if c.model else LR.WordListLM(list(dict.fromkeys(w for w, _ in c.entries)))
    if c.words is not None:
        return LR.WordListLM(c.words, c.case_sensitive)
    return oracle_lm(c.model, c.pruned) if c.model else None


def table_of(c):
    return TR.Table(c.entries, c.labels, ref_lm(c))


def make_search(c, restricted=None):
    restricted = c.restricted if restricted is None else restricted
    if c.family == "trans":
        return recording(TR.Search)(c.labels, c.blank, c.W, ref_lm(c), table_of(c), restricted, c.lmwt, c.wip, c.oov)
    lexicon = None
    if restricted:
        lexicon = LR.Lexicon(c.words if c.words is not None else model_words(c.model), c.case_sensitive)
    return recording(LR.Search)(c.labels, c.blank, c.W, ref_lm(c), c.case_sensitive, c.lmwt, c.wip, c.oov, lexicon=lexicon)


def frames_of(c, b):
    return max(0, min(c.lens[b], c.x.shape[1]))


def search(c, b, n_frames=None, restricted=None):
    """The restatement on utterance b (its first n_frames frames) -> (ranking, margin, the search with what it recorded)."""
    n = frames_of(c, b) if n_frames is None else n_frames
    s = make_search(c, restricted)
    t0 = time.perf_counter()
    ranking = s.run(c.x[b, :n].astype(np.float64), n)
    s.seconds = time.perf_counter() - t0
    return ranking, s.margin(), s


@functools.lru_cache(maxsize=None)
def reference(family, seed):
    """[(ranking, margin, search) per utterance] of a case of SEARCHES, once per process."""
    c = draw(family, seed)
    return [search(c, b) for b in range(len(c.lens))]


def compared(family, seed, b):
    return reference(family, seed)[b][1] >= MIN_GAP


def utterances(family):
    return [(s, b) for s in range(FAMILIES[family]) for b in range(len(draw(family, s).lens))]


def lm_kind(c):
    """The LM kind of DESIGN 4.4 a case asks for: none, or (tables, spelled or homophones, restricted or not)."""
    if c.model is None and c.words is None and c.entries is None:
        return "none"
    return ("id tables" if c.pruned else "signatures", "homophones" if c.entries is not None else "spelled", c.restricted)


def facts(family, seed):
    """What the coverage test counts, of the compared utterances of a case."""
    c = draw(family, seed)
    f = SimpleNamespace(case=c, utts=[], general=takes_general(c.V, c.W, lm_kind(c) != "none"))
    for b, (ranking, gap, s) in enumerate(reference(family, seed)):
        if gap < MIN_GAP:
            continue
        u = SimpleNamespace(b=b, frames=frames_of(c, b), ranking=ranking, gap=gap, n=len(ranking), search=s)
        run, u.full_run = 0, 0                  # the longest run of frames with a full beam
        for k in s.sizes:
            run = run + 1 if k == c.W else 0
            u.full_run = max(u.full_run, run)
        u.never_full = u.frames > 0 and max(s.sizes) < c.W
        u.empty_winner = u.frames > 0 and ranking[0]["ids"] == (-1,)
        f.utts.append(u)
    return f
