"""Test-side restatement of the Gram-CTC beam search restricted to a vocabulary, with label timestamps
(e2e_gram_ctc_beam_nbest_opt, the definition in include/e2e_ctc.h), in plain Python: gram_decode_lm_ref.beam_search's masses,
fields, totals, cut and ranking, with two additions -- a (member, column) pair whose extension is not admissible is skipped,
and every sequence carries the frames at which the nodes of its ids were created.  admissible() is the same rule as a
stand-alone predicate of a base-id sequence, for the enumerator.  As the restatement it builds on, it reports the smallest
gap between the W-th and the (W+1)-th total at any cut and between neighbours of the final ranking (totals are logs: an
absolute gap there is a relative gap of the masses).  Also the fixed-seed inputs that the CPU and the GPU tests share.

L and Pref(L) come from lexicon_ref.Lexicon, a word list's model from lexicon_ref.WordListLM, everything else from
gram_decode_lm_ref; none of them is edited.  It shares no code with the product; only tests import it."""
import functools
import math
import os

import numpy as np

import gram_decode_lm_ref as LR
import gram_decode_ref as DR
import gram_ref as GR
from lexicon_ref import Lexicon, WordListLM, arpa_words

NEG_INF = LR.NEG_INF
MIN_GAP = LR.MIN_GAP


class Rule:
    """The vocabulary's side of a restricted search: the base labels' strings, the space's base id, a Lexicon."""

    def __init__(self, labels, lexicon):
        self.labels = list(labels)
        self.space_id = self.labels.index(" ") if " " in self.labels else -1
        self.lexicon = lexicon

    def last_word(self, seq):
        """The folded spelling of the run of ids after the last space."""
        k = len(seq)
        while k > 0 and seq[k - 1] != self.space_id:
            k -= 1
        return self.lexicon.fold("".join(self.labels[i] for i in seq[k:]).encode())

    def step_allowed(self, y, i):
        """The rule for y + (i), y admissible."""
        if i != self.space_id:
            return self.last_word(tuple(y) + (i,)) in self.lexicon.prefixes
        return len(y) == 0 or y[-1] == self.space_id or self.last_word(tuple(y)) in self.lexicon.words

    def gram_allowed(self, y, gram):
        """An extension by a gram of k ids applies the rule k times."""
        y = tuple(y)
        for i in gram:
            if not self.step_allowed(y, i):
                return False
            y += (i,)
        return True


def admissible(seq, rule):
    """Does every base-id prefix of the sequence obey the rule?  (The empty sequence does.)"""
    seq = tuple(seq)
    return all(rule.step_allowed(seq[:n], seq[n]) for n in range(len(seq)))


def beam_search(lp, grams, F, rule, beam_width=None):
    """gram_decode_lm_ref.beam_search restricted to rule (None: unrestricted, only the frames are new): the final ranking's
    dicts also have `frames`, one per id -- the frame at which the node that carries the id was created.  A survivor that was a
    member keeps its frames; a new one takes those of the parent of its least m * V + c pair (m the parent's position in the
    beam; the loops below run in that order, so it is the pair that creates the entry) plus (t,) once per id of the column."""
    T, V = lp.shape
    order = max((len(g) for g in grams.values()), default=1)
    slots = range(order + 1)
    cols = [(c, len(grams[c]), tuple(grams[c])) for c in range(1, V)]
    beam = {(): ([1.0] + [0.0] * order, [0] * (order + 1))}
    frames = {(): ()}
    ranking = [(0.0, ())]
    esum, gap = 0, math.inf

    def total(p):
        tot = 0.0
        for k in slots:
            tot += p[k]
        return tot

    for t in range(T):
        y = np.exp(lp[t]).tolist()
        new, parent = {}, {}
        for seq, (p, col) in beam.items():
            tot = total(p)
            sp, sc = [0.0] * (order + 1), [0] * (order + 1)
            sp[0] = tot * y[0]
            for k in range(1, order + 1):
                if p[k] > 0.0:
                    sp[k] = p[k] * y[col[k]]
                    sc[k] = col[k]
            new[seq] = (sp, sc)
        for seq, (p, col) in beam.items():                             # in the order of the ranks: m ascending, then c
            tot = total(p)
            for c, k, g in cols:
                src = tot
                if col[k] == c and p[k] > 0.0:
                    src = 0.0
                    for kk in slots:
                        if kk != k:
                            src += p[kk]
                v = src * y[c]
                if v > 0.0 and (rule is None or rule.gram_allowed(seq, g)):
                    child = seq + g
                    if child not in new:
                        new[child] = ([0.0] * (order + 1), [0] * (order + 1))
                        parent[child] = (seq, len(g))
                    new[child][0][k] += v
                    new[child][1][k] = c
        rows = []
        for seq, (p, col) in new.items():
            tot = total(p)
            if tot > 0.0:
                tt = F.total(math.log(tot), F.of(seq, parent[seq][0] if seq in parent else None))
                if tt > NEG_INF:
                    rows.append((tt, seq, tot))
        rows = LR._ranked(rows)
        if beam_width is not None and len(rows) > beam_width:
            gap = min(gap, rows[beam_width - 1][0] - rows[beam_width][0])
            rows = rows[:beam_width]
        if not rows:
            return [], gap
        _, ex = math.frexp(rows[0][2])
        esum += ex
        beam, was = {}, frames
        frames = {}
        for _, seq, _ in rows:
            p, col = new[seq]
            p = [math.ldexp(v, -ex) for v in p]
            beam[seq] = (p, [c if v > 0.0 else 0 for v, c in zip(p, col)])
            frames[seq] = was[parent[seq][0]] + (t,) * parent[seq][1] if seq in parent else was[seq]
        ranking = [(tt, seq) for tt, seq, _ in rows]
    for hi, lo in zip(ranking, ranking[1:]):
        gap = min(gap, hi[0] - lo[0])
    out = []
    for _, seq in ranking:
        f = F.of(seq)
        ac = math.log(total(beam[seq][0])) + esum * LR.LN2
        out.append(dict(ids=seq, total=F.total(ac, f), ac=ac, lm=f.lm, words=f.words, oov=f.oov, frames=frames[seq]))
    return out, gap


def enumerate_ranked(lp, grams, F, rule):
    """gram_decode_lm_ref.enumerate_ranked over the admissible labellings only."""
    return [r for r in LR.enumerate_ranked(lp, grams, F) if admissible(r["ids"], rule)]


def timestep_properties(row, n_frames):
    """The properties the header states of one result's frames (a list of problems; empty: none)."""
    fr, bad = row["frames"], []
    if len(fr) != len(row["ids"]):
        bad.append("one frame per id")
    if any(not 0 <= v < n_frames for v in fr):
        bad.append("values in [0, x_len)")
    if any(a > b for a, b in zip(fr, fr[1:])):
        bad.append("never decrease")
    return bad


# ---- vocabularies ---------------------------------------------------------------------------------------------------
KNOBS = LR.KNOBS
LIST_KNOBS = dict(lmwt=0.0, wip=KNOBS["wip"], oov_penalty=0.0)        # what a word list leaves of the knobs
TINY_WORDS = ["ab", "b"]                                               # the tiny grid's word list (`a` is a prefix, no word)


@functools.lru_cache(maxsize=None)
def vocabulary(source, labels, case_sensitive=True):
    """source: the name of a model under tests/golden or a tuple of words; labels a tuple -> (Fields, Rule).  With
    case_sensitive False the labels are given in upper case and folded by the lookup."""
    labels = list(labels)
    if isinstance(source, str):
        words = arpa_words(os.path.join(LR.GOLDEN, source))
        F = LR.Fields(labels, LR.oracle_lm(source), case_sensitive, **KNOBS)
    else:
        words = list(source)
        F = LR.Fields(labels, WordListLM(words, case_sensitive), case_sensitive, **LIST_KNOBS)
    return F, Rule(labels, Lexicon(words, case_sensitive))


def tiny_labels(case_sensitive):
    return tuple(LR.TINY_LABELS if case_sensitive else LR.upper(LR.TINY_LABELS))


TINY_SOURCES = (LR.TINY_MODEL, tuple(TINY_WORDS))


@functools.lru_cache(maxsize=None)
def tiny_enumeration(i, source, case_sensitive, f32=False):
    """The filtered enumeration of tiny case i of gram_decode_lm_ref's grid (f32: of the f32 log-softmax)."""
    import torch
    R, V, l2i, x = LR.tiny_case(i)
    t = torch.from_numpy(x)
    lp = torch.log_softmax(t if f32 else t.double(), -1).double().numpy()
    F, rule = vocabulary(source, tiny_labels(case_sensitive), case_sensitive)
    return enumerate_ranked(lp, GR.grams_of(R, V, l2i), F, rule)


# ---- the pruned cases: V = 21 with a gram of order 8, T = 14, four utterances of lengths 14, 9, 1, 0 ------------------
PRUNED_WIDTHS = (2, 7, 32)
PRUNED_T, PRUNED_LENS = 14, [14, 9, 1, 0]
_T = dict(a=1, b=2, s=3)                                               # _ a b ` `
_O = {" ": 1, "a": 2, "b": 3, "c": 4, "d": 5, "e": 6, "'": 7}          # _ ` ` a b c d e '


def _ids(index, spelled):
    return [index[ch] for ch in spelled]


PRUNED = {
    "tiny_3gram.arpa": dict(
        source="tiny_3gram.arpa", labels=LR.TINY_LABELS, seed=71,
        grams=[_ids(_T, g) for g in ("ab", "as", "sb", "ba", "asb", "bsa", "aa", "bb", "ss", "abs", "bas", "sa", "bs", "sab",
                                     "asba", "aba", "absbasab")]),
    "lm_order4.arpa": dict(
        source="lm_order4.arpa", labels=["_", " ", "a", "b", "c", "d", "e", "'"], seed=72,
        grams=[_ids(_O, g) for g in ("be", "ad", "ca", "bea", "d b", "dead", "de", "ed", "ab ", " a", "e'", "cc", "bead dad")]),
    "word list": dict(
        source=("bead", "dad", "be", "ad", "cab", "a", "deed", "e'", "d"), labels=["_", " ", "a", "b", "c", "d", "e", "'"], seed=73,
        grams=[_ids(_O, g) for g in ("be", "ad", "ca", "bea", "d b", "dead", "de", "ed", "ab ", " a", "e'", "cc", "bead dad")]),
}
PRUNED_CASES = [(name, W) for name in PRUNED for W in PRUNED_WIDTHS]
LEFT_OUT = ()      # cases whose restatement is decided by less than MIN_GAP: at most one in ten (test_gram_lexicon_cpu.py)


@functools.lru_cache(maxsize=None)
def pruned_case(name):
    """-> (R, V, label2ids, logits (4, 14, V) f32)."""
    m = PRUNED[name]
    R = len(m["labels"])
    l2i = {R + j: list(g) for j, g in enumerate(m["grams"])}
    V = R + len(l2i)
    x = (np.random.default_rng(m["seed"]).standard_normal((len(PRUNED_LENS), PRUNED_T, V)) * 2.0).astype(np.float32)
    x[1, 0, 0] = 9.0                           # utterance 1 begins with a frame of blank: the empty prefix stays, the first id
    return R, V, l2i, x                        # of most of its results is created later than frame 0


@functools.lru_cache(maxsize=None)
def pruned_ref(name, W, restricted=True):
    """beam_search on the f64 log-softmax of every utterance of pruned_case(name): ([ranking per utterance], smallest gap)."""
    m = PRUNED[name]
    R, V, l2i, x = pruned_case(name)
    grams = GR.grams_of(R, V, l2i)
    lp = DR.log_softmax(x.astype(np.float64))
    F, rule = vocabulary(m["source"], tuple(m["labels"]))
    out, gap = [], math.inf
    for b, n in enumerate(PRUNED_LENS):
        r, g = beam_search(lp[b, :n], grams, F, rule if restricted else None, W)
        out.append(r)
        gap = min(gap, g)
    return out, gap
