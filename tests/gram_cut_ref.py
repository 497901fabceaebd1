"""The pruned Gram-CTC beam search (TEST INFRASTRUCTURE ONLY): a plain-Python restatement whose step loops over the
frame's kept columns (label_cut_ref.cut_frame with blank 0), for the masses as gram_decode_ref.beam_search states them and
for the totals as gram_decode_lm_ref.beam_search does -- their ranking, keys and Fields are imported, not restated -- and
the seeded cases that tests/test_gram_cut_cpu.py and tests/test_gpu_gram_cut.py share.  A column outside the frame's set
gives no extension share and no "run continues" stay share; the blank's stay share is always there.

The kept set's P_j is a sequential f64 sum here and a scan of fixed shape on the GPU: an utterance one of whose frames has a
P_j within label_cut_ref.BOUNDARY of cutoff_prob, or whose search is decided by a margin below gram_beam_fuzz_util.MIN_GAP
(relative for the masses, absolute for the log totals), is not compared on the GPU (LEFT_OUT; the CPU test recomputes it and
holds it to LEFT_OUT_CAP)."""
import functools
import math

import numpy as np

import gram_beam_fuzz_util as GF
import gram_decode_lm_ref as LR
import gram_decode_ref as DR
import gram_ref as GR
import label_cut_ref as LC

LN2 = math.log(2.0)
MIN_GAP, BOUNDARY, LEFT_OUT_CAP = GF.MIN_GAP, LC.BOUNDARY, GF.LEFT_OUT_CAP
LABELS = LR.TINY_LABELS + ["c", "d"]             # R = 6: the alphabet of tiny_3gram.arpa and two letters it does not have
MODEL = LR.TINY_MODEL
WORDS = ["a", "ab", "b", "ba"]


def beam_search(lp, grams, cutoff_top_n, cutoff_prob, beam_width=None, F=None):
    """lp (T, V) f64 log-probabilities, grams {column: base-id tuple} -> (ranking, margin, smallest boundary margin).
    F None: the search on the masses, ranking [(sequence, log tot)] and relative gaps as gram_decode_ref.beam_search;
    F a gram_decode_lm_ref.Fields: the search on the totals, ranking of dicts and absolute gaps as gram_decode_lm_ref's.
    margin: the smallest gap at any cut and between neighbours of the final ranking whose scores differ."""
    T, V = lp.shape
    order = max((len(g) for g in grams.values()), default=1)
    slots = range(order + 1)
    top_n = V if cutoff_top_n is None else cutoff_top_n
    beam = {(): ([1.0] + [0.0] * order, [0] * (order + 1))}
    esum, gap, boundary = 0, math.inf, math.inf

    def total(p):
        tot = 0.0
        for k in slots:
            tot += p[k]
        return tot

    for t in range(T):
        kept = LC.cut_frame(lp[t], 0, top_n, cutoff_prob)            # ascending, the blank among them
        boundary = min(boundary, LC.boundary_margin(lp[t], top_n, cutoff_prob))
        here = set(kept)
        y = np.exp(lp[t]).tolist()
        new, parent = {}, {}
        for seq, (p, col) in beam.items():
            sp, sc = [0.0] * (order + 1), [0] * (order + 1)
            sp[0] = total(p) * y[0]
            for k in range(1, order + 1):
                if p[k] > 0.0 and col[k] in here:                    # (a slot whose column is not kept: no stay share)
                    sp[k] = p[k] * y[col[k]]
                    sc[k] = col[k]
            new[seq] = (sp, sc)
        for seq, (p, col) in beam.items():
            tot = total(p)
            for c in kept:                                           # the frame's kept columns alone
                if c == 0:
                    continue
                g = tuple(grams[c])
                k = len(g)
                src = tot
                if col[k] == c and p[k] > 0.0:
                    src = 0.0
                    for kk in slots:
                        if kk != k:
                            src += p[kk]
                v = src * y[c]
                if v > 0.0:
                    child = seq + g
                    if child not in new:
                        new[child] = ([0.0] * (order + 1), [0] * (order + 1))
                        parent[child] = seq
                    new[child][0][k] += v
                    new[child][1][k] = c
        rows = []
        for seq, (p, col) in new.items():
            tot = total(p)
            if tot > 0.0:
                if F is None:
                    rows.append((tot, seq, tot))
                else:
                    tt = F.total(math.log(tot), F.of(seq, parent.get(seq)))
                    if tt > LR.NEG_INF:
                        rows.append((tt, seq, tot))
        rows = (DR._ranked if F is None else LR._ranked)(rows)
        if beam_width is not None and len(rows) > beam_width:
            hi, lo = rows[beam_width - 1][0], rows[beam_width][0]
            gap = min(gap, (hi - lo) / hi if F is None else hi - lo)
            rows = rows[:beam_width]
        if not rows:
            return [], gap, boundary
        _, ex = math.frexp(rows[0][2])
        esum += ex
        beam = {}
        for _, seq, _ in rows:
            p, col = new[seq]
            p = [math.ldexp(v, -ex) for v in p]
            beam[seq] = (p, [c if v > 0.0 else 0 for v, c in zip(p, col)])
    if F is None:
        final = DR._ranked([(total(p), seq) for seq, (p, _) in beam.items()])
        for hi, lo in zip(final, final[1:]):
            if hi[0] != lo[0]:
                gap = min(gap, (hi[0] - lo[0]) / hi[0])
        return [(seq, math.log(tot) + esum * LN2) for tot, seq in final], gap, boundary
    rows = []
    for seq, (p, _) in beam.items():
        f = F.of(seq)
        tot = total(p)
        rows.append((F.total(math.log(tot), f), seq, math.log(tot) + esum * LN2, f))
    rows = LR._ranked(rows)
    for hi, lo in zip(rows, rows[1:]):
        if hi[0] != lo[0]:
            gap = min(gap, hi[0] - lo[0])
    return [dict(ids=seq, total=F.total(ac, f), ac=ac, lm=f.lm, words=f.words, oov=f.oov) for _, seq, ac, f in rows], gap, boundary


def masked(lp, cutoff_top_n, cutoff_prob):
    """lp (T, V) with every column outside its frame's kept set at -inf."""
    out = np.full_like(lp, -np.inf)
    for t in range(lp.shape[0]):
        kept = LC.cut_frame(lp[t], 0, lp.shape[1] if cutoff_top_n is None else cutoff_top_n, cutoff_prob)
        out[t, kept] = lp[t, kept]
    return out


# ---- the tables of the bit-for-bit cases (tests/test_gpu_gram_cut.py 1, 2, 4, 5) -----------------------------------------------
EQ_V = (6, 40, 300)
EQ_SHAPE = (4, 24, [24, 0, 1, 17])               # B, T, lengths: 0, 1 and T among them
EQ_TOP_N = (1, 3, 12)
EQ_PROB = (1.0, 0.9, 0.5)


def eq_widths(V):
    """2, 8 and the unpruned limit for V, capped at 128."""
    return (2, 8, min(128, GF.max_width(V)))


@functools.lru_cache(maxsize=None)
def eq_table(V):
    """R = 6 and random_table's grams: none (V = 6); orders 2, 3 and one of order 8 (V = 40); orders 2, 3, 4 (V = 300)."""
    rng = np.random.default_rng(81000 + V)
    R = 6
    counts = {6: ((), ()), 40: ((14, 19), (8,)), 300: ((20, 100, 174), ())}[V]
    l2i, total = DR.random_table(rng, R, *counts[0], extra=counts[1])
    assert total == V
    return R, l2i


@functools.lru_cache(maxsize=None)
def eq_input(V):
    """Log-probabilities (B,T,V) f32 (the f32 and the f64 call see the same numbers): N(0,1) logits times 2, the blank's logit
    raised by 6 in every third frame so that cutoff_top_n = 1 has frames that keep the blank alone."""
    B, T, lens = EQ_SHAPE
    rng = np.random.default_rng(82000 + V)
    x = (rng.standard_normal((B, T, V)) * 2.0).astype(np.float32)
    x[:, ::3, 0] += 6.0
    return GF.log_softmax32(x), list(lens)


# ---- beyond the unpruned width limit (tests/test_gpu_gram_cut.py 3) --------------------------------------------------------------
WIDE = dict(V=2048, R=6, W=100, top_n=20, B=2, T=16)
WIDE_PROBS = (1.0, 0.9)
WIDE_SEED = {1.0: 83000, 0.9: 83001}             # seeds for which the restatement alone stays within the cap (CPU test)
KNOBS = LR.KNOBS


@functools.lru_cache(maxsize=None)
def wide_table():
    """V = 2048 over R = 6: 25 bigrams, 125 trigrams, 625 and 1267 grams of orders 4 and 5."""
    rng = np.random.default_rng(83100)
    l2i, total = DR.random_table(rng, WIDE["R"], 25 - 6, 125 - 50, 625 - 250, 2042 - 19 - 75 - 375)
    assert total == WIDE["V"]
    return l2i


@functools.lru_cache(maxsize=None)
def wide_input(prob):
    rng = np.random.default_rng(WIDE_SEED[prob])
    x = (rng.standard_normal((WIDE["B"], WIDE["T"], WIDE["V"])) * 3.0).astype(np.float32)
    x[:, :, :WIDE["R"]] += 2.0                                       # (the unigrams and the blank stay in sight of the grams)
    return GF.log_softmax32(x), [WIDE["T"], WIDE["T"] - 3]


def wide_fields(with_lm):
    if not with_lm:
        return None
    return LR.Fields(LABELS, LR.oracle_lm(MODEL), True, **KNOBS)


@functools.lru_cache(maxsize=None)
def wide_reference(prob, with_lm):
    """[(ranking, margin, boundary margin) per utterance] of the kept-loop restatement, once per process."""
    lp, lens = wide_input(prob)
    grams = GR.grams_of(WIDE["R"], WIDE["V"], wide_table())
    return [beam_search(lp[b, :n].astype(np.float64), grams, WIDE["top_n"], prob, WIDE["W"], wide_fields(with_lm))
            for b, n in enumerate(lens)]


def wide_compared(prob, with_lm, b):
    _, gap, boundary = wide_reference(prob, with_lm)[b]
    return gap >= MIN_GAP and boundary >= BOUNDARY


def wide_left_out():
    """[(prob, with_lm, b)] of the utterances that are not compared, and the number of utterances."""
    out, total = [], 0
    for prob in WIDE_PROBS:
        for with_lm in (False, True):
            for b in range(WIDE["B"]):
                total += 1
                if not wide_compared(prob, with_lm, b):
                    out.append((prob, with_lm, b))
    return out, total


LEFT_OUT = ()                                    # (prob, with_lm, utterance) not compared (the CPU test recomputes them)
