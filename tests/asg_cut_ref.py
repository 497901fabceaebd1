"""The pruned ASG beam search (TEST INFRASTRUCTURE ONLY): the host selection of include/e2e_ctc.h (e2e_asg_beam_nbest_cut), a
kept-loop restatement -- asg_beam_ref.Search and asg_lexicon_ref.RestrictedSearch subclassed so that a frame loops over its
kept labels alone; it is not a mask -- and the seeded cases that tests/test_asg_cut_cpu.py and tests/test_gpu_asg_cut.py share.

A label outside the frame's kept set is no candidate at frame 0 and gives no extension share; a member whose last label is not
kept has no stay share and survives the frame only as a parent.

An utterance whose search is decided by a margin below asg_beam_fuzz_util's MIN_GAP is not compared with the restatement on
the GPU (LEFT_OUT; the CPU test recomputes it and holds it to LEFT_OUT_CAP)."""
import functools
import os

import numpy as np

import asg_beam_fuzz_util as F
import asg_beam_ref as REF
import asg_beam_util as BU
import asg_lexicon_ref as LR
import asg_lexicon_util as LU

MIN_GAP, LEFT_OUT_CAP = BU.MIN_GAP, F.LEFT_OUT_CAP
NEG_INF = REF.NEG_INF
MODEL = "tiny_3gram.arpa"                        # its words are spelled with a and b
WORDS = ["a", "ab", "b", "ba", "abb", "baa", "c", "ca", "dab"]
KNOBS = BU.LM_KNOBS


# ---- the selection -------------------------------------------------------------------------------------------------------------
def kept_of(row, top_n):
    """The kept labels of a frame, ascending: the first min(top_n, V) of a stable descending sort (the lower id wins a tie),
    NaN counting as -inf; -0 and +0 compare equal."""
    v = np.asarray(row, dtype=np.float64).copy()
    v[np.isnan(v)] = -np.inf
    order = np.argsort(-v, kind="stable")
    return sorted(int(c) for c in order[: min(int(top_n), len(v))])


def masked(x, top_n):
    """x (..., V) with every label outside its frame's kept set at -inf (the kept ones as they are, a kept NaN included)."""
    x = np.asarray(x)
    out = np.full_like(x, -np.inf)
    flat_in, flat_out = x.reshape(-1, x.shape[-1]), out.reshape(-1, x.shape[-1])
    for i in range(flat_in.shape[0]):
        k = kept_of(flat_in[i], top_n)
        flat_out[i, k] = flat_in[i, k]
    return out


# ---- the kept-loop restatement ---------------------------------------------------------------------------------------------------
def _kept_run(s, x, A, n):
    """asg_lexicon_ref.RestrictedSearch.run with every loop over the labels replaced by a loop over the frame's kept labels,
    and the stay share only for a member whose last label is kept.  s.allowed / s.note are the restricted search's (absent: the
    plain search)."""
    V = s.V
    allowed = getattr(s, "allowed", lambda y, c: True)
    note = getattr(s, "note", lambda beam: None)
    root = REF.LmFields((s.lm.word_index("<s>"),) if s.lm is not None else ())
    cands = {}
    for c in kept_of(x[0], s.top_n):
        if REF.may_follow(None, c, V, s.R, s.space_id) and allowed((), c):
            cands[(c,)] = (float(x[0][c]), s.child_fields(root, None, c))
    beam = s.ranked(cands, cut=True)
    frames = {seq: (0,) for seq, _, _, _ in beam}
    note(beam)
    for t in range(1, n):
        if not beam:
            s.died = True
            return []
        kept = kept_of(x[t], s.top_n)
        here = set(kept)
        members = {seq: (ac, f) for seq, ac, f, _ in beam}
        stay, extn, fields, parent = {}, {}, {}, {}
        for seq, (sc, f) in members.items():
            a = seq[-1]
            fields[seq] = f
            if a in here:                                                 # (a member whose label is dropped does not stay)
                aa = float(A[a][a]) if A is not None else 0.0
                stay[seq] = sc + aa + float(x[t][a])
            for c in kept:
                if c == a or not REF.may_follow(a, c, V, s.R, s.space_id) or not allowed(seq, c):
                    continue
                ca = float(A[c][a]) if A is not None else 0.0
                child = seq + (c,)
                extn[child] = sc + ca + float(x[t][c])
                if child not in members:
                    fields[child] = s.child_fields(f, a, c)
                    parent[child] = seq
        cands = {seq: (REF.lse(stay.get(seq, NEG_INF), extn.get(seq, NEG_INF)), fields[seq]) for seq in set(stay) | set(extn)}
        beam = s.ranked(cands, cut=True)
        frames = {seq: frames[seq] if seq in members else frames[parent[seq]] + (t,) for seq, _, _, _ in beam}
        note(beam)
    if not beam:
        s.died = True
    for hi, lo in zip(beam, beam[1:]):
        if hi[3] != lo[3]:
            s.min_gap = min(s.min_gap, hi[3] - lo[3])
    return [dict(ids=seq, total=tot, ac=ac, lm=f.lm, words=f.words, oov=f.oov, frames=frames[seq]) for seq, ac, f, tot in beam]


class CutSearch(REF.Search):
    """asg_beam_ref.Search whose frames loop over their top_n kept labels."""

    def __init__(self, top_n, *a, **kw):
        super().__init__(*a, **kw)
        self.top_n, self.died = top_n, False

    def run(self, x, A, n):
        return _kept_run(self, x, A, n)


class CutRestrictedSearch(LR.RestrictedSearch):
    """asg_lexicon_ref.RestrictedSearch whose frames loop over their top_n kept labels."""

    def __init__(self, top_n, *a, **kw):
        super().__init__(*a, **kw)
        self.top_n = top_n

    def run(self, x, A, n):
        return _kept_run(self, x, A, n)


def run_all(s, x, A, x_len):
    """[ranking per utterance] of search s (any of the four classes): empty for a length outside [1, T]; and [margin per
    utterance] (inf for such an utterance)."""
    out, gaps = [], []
    for b in range(len(x)):
        s.min_gap = float("inf")
        n = int(x_len[b])
        out.append(s.run(x[b], A, n) if 1 <= n <= len(x[b]) else [])
        gaps.append(s.min_gap)
    return out, gaps


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
# (B, T, V, R, W, K): a small one; the README's alphabet; the largest pair space (W * K above the thread count); K = 1; K = V - 1
SHAPES = ((4, 24, 7, 2, 4, 3), (3, 40, 29, 2, 16, 10), (2, 12, 128, 0, 128, 40), (3, 16, 5, 1, 8, 1), (3, 16, 5, 1, 8, 4))
LENS = ([24, 1, 0, 25], [40, 23, 31], [12, 7], [16, 0, 9], [1, 16, 17])          # ragged; 1, 0 and T + 1 among them
KINDS = ("randn", "half", "nan")
INSTANCES = ("plain", "wip", "lm", "lex_lm", "lex_words", "timesteps")


def chars_of(shape):
    """The V - R characters of a shape: a and b (the model's letters) and the space among them."""
    V, R = SHAPES[shape][2], SHAPES[shape][3]
    if V == 29:
        return list(LU.LETTERS)
    if V == 128:
        return LU.alphabet(V - R, space=5)
    return ["a", "b", " ", "c", "d"][: V - R]


def labels_of(shape):
    """The strings of all V columns, as the device model is loaded with them."""
    return chars_of(shape) + ["<%d>" % (r + 1) for r in range(SHAPES[shape][3])]


@functools.lru_cache(maxsize=None)
def case(shape, kind):
    """(x (B,T,V) f32 -- the f32 and the f64 call see the same numbers --, A (V,V) f32 or None, lengths).
    randn: N(0,1) times 3, random transitions.  half: quantised to multiples of 0.5, so that a frame's K-th place is tied and
    the lower id must win; no transitions.  nan: randn with label 1 NaN in every frame and a tenth of the rest -inf."""
    B, T, V, R, W, K = SHAPES[shape]
    rng = np.random.default_rng(91000 + 10 * shape + KINDS.index(kind))
    x = (rng.standard_normal((B, T, V)) * 3.0).astype(np.float32)
    A = rng.standard_normal((V, V)).astype(np.float32)
    if kind == "half":
        x = (np.round(x) * 0.5).astype(np.float32)
        x[x == 0] = np.where(rng.random(int((x == 0).sum())) < 0.5, np.float32(-0.0), np.float32(0.0))
        A = None
    if kind == "nan":
        x[rng.random((B, T, V)) < 0.1] = -np.inf
        x[:, :, 1] = np.nan
    return x, A, list(LENS[shape])


def search_of(shape, inst, top_n=None):
    """The restatement's search of an instance: kept-loop with top_n, else the plain one."""
    import oracle_lib as O
    B, T, V, R, W, K = SHAPES[shape]
    chars = chars_of(shape)
    kw = dict(V=V, R=R, space_id=chars.index(" "), W=W, chars=chars)
    lex = None
    if inst in ("wip", "lex_words"):
        kw.update(wip=0.4)
    if inst in ("lm", "lex_lm", "timesteps"):
        kw.update(lm=O.OracleLM(os.path.join(BU.GOLDEN, MODEL)), lmwt=KNOBS["lmwt"], wip=KNOBS["wip"], oov=KNOBS["oov_penalty"])
    if inst == "lex_lm":
        lex = LR.Lexicon(LR.arpa_words(os.path.join(BU.GOLDEN, MODEL)), True)
    if inst == "lex_words":
        kw.update(lm=LR.WordListLM(WORDS, True))
        lex = LR.Lexicon(WORDS, True)
    if lex is not None:
        return CutRestrictedSearch(top_n, lexicon=lex, **kw) if top_n is not None else LR.RestrictedSearch(lexicon=lex, **kw)
    return CutSearch(top_n, **kw) if top_n is not None else REF.Search(**kw)


# ---- what the GPU file holds to the restatement (test 7): two shapes, plain and with the model, the randn emissions -----------------
ORACLE = tuple((shape, inst) for shape in (1, 0) for inst in ("plain", "lm"))


@functools.lru_cache(maxsize=None)
def oracle_reference(shape, inst):
    """([ranking per utterance], [margin per utterance]) of the kept-loop restatement, once per process."""
    x, A, lens = case(shape, "randn")
    return run_all(search_of(shape, inst, SHAPES[shape][5]), x.astype(np.float64).tolist(), A.tolist(), lens)


def oracle_left_out():
    """[(shape, inst, utterance)] decided by less than MIN_GAP, and the number of utterances that have a ranking at all."""
    out, total = [], 0
    for shape, inst in ORACLE:
        ranking, gaps = oracle_reference(shape, inst)
        for b, n in enumerate(LENS[shape]):
            if 1 <= n <= SHAPES[shape][1]:
                total += 1
                if not gaps[b] >= MIN_GAP:
                    out.append((shape, inst, b))
    return out, total


LEFT_OUT = ()                                    # (shape, inst, utterance) not compared (the CPU test recomputes them: equal)
