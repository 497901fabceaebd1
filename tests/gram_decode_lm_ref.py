"""Test-side restatement of the Gram-CTC beam search with a word language model (e2e_gram_ctc_beam_nbest_lm, the
definition in include/e2e_ctc.h) in plain Python: gram_decode_ref.beam_search's rules for the masses, asg_beam_ref's
LmFields / child_fields applied per base id for the language model's fields, and the cut and the ranking on the totals.
It reports the smallest absolute gap between the W-th and the (W+1)-th total at any cut and between neighbours of the
final ranking.  Also: an enumerator that groups all V**T paths by base sequence, computes each sequence's fields from the
sequence alone and ranks by total, and the fixed-seed inputs that the CPU and the GPU tests share.  LM numbers come from
oracle_lib.OracleLM.  It shares no code with the product; only tests import it."""
import functools
import math
import os

import numpy as np

import asg_beam_ref as AR
import gram_decode_ref as DR
import gram_ref as GR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NEG_INF = float("-inf")
LN2 = math.log(2.0)
KNOBS = dict(lmwt=0.7, wip=0.4, oov_penalty=-1.3)
MIN_GAP = 1e-6         # a cut decided by less is decided by f64 rounding (sums of a few dozen terms <= 1e3: about 1e-12)


@functools.lru_cache(maxsize=None)
def oracle_lm(model):
    import oracle_lib as O
    return O.OracleLM(os.path.join(GOLDEN, model))


class Fields:
    """The language model's side of a search: labels (the base labels' strings, index 0 the blank's), the space's base id
    (-1: none), an OracleLM or None, the knobs.  The rules are asg_beam_ref.Search.child_fields', one base id at a time."""

    def __init__(self, labels, lm=None, case_sensitive=True, lmwt=1.0, wip=0.0, oov_penalty=0.0):
        self.labels = list(labels)
        self.space_id = self.labels.index(" ") if " " in self.labels else -1
        self.rules = AR.Search(len(self.labels), 0, self.space_id, None, self.labels, lm, case_sensitive, lmwt, wip, oov_penalty)
        self.lm, self.lmwt, self.wip, self.oov = lm, self.rules.lmwt, wip, oov_penalty
        self.root = AR.LmFields((lm.word_index("<s>"),) if lm is not None else ())
        self._of = {(): self.root}

    def step(self, f, last, c):
        return self.rules.child_fields(f, last, c)

    def sequence_fields(self, seq):
        """From the sequence alone, id by id."""
        f, last = self.root, None
        for c in seq:
            f, last = self.step(f, last, c), c
        return f

    def _skip(self, p, last, c):
        """child_fields without its query: what a non-final id of a word leaves when the model is not asked (lm, oov and the
        state keep the parent's values; they are overwritten at the word's next id)."""
        n = AR.LmFields()
        new_word = last is None or last == self.space_id
        n.words = p.words + (1 if new_word else 0)
        if self.lm is None:
            return n
        n.word = self.labels[c] if new_word else p.word + self.labels[c]
        if new_word:
            n.st_before, n.lm_before, n.oov_before = p.st, p.lm, p.oov
        else:
            n.st_before, n.lm_before, n.oov_before = p.st_before, p.lm_before, p.oov_before
        n.lm, n.oov, n.st = p.lm, p.oov, p.st
        return n

    def gram_fields(self, f, last, gram):
        """The fields of a sequence (fields f, last id `last` or None) extended by a gram: the model is asked only at a
        word's last id inside the gram and at the gram's last id."""
        for j, c in enumerate(gram):
            ask = j + 1 == len(gram) or gram[j + 1] == self.space_id
            f = self.step(f, last, c) if (c == self.space_id or ask) else self._skip(f, last, c)
            last = c
        return f

    def of(self, seq, parent=None):
        """Memo: the fields of seq, through a parent whose fields are known when one is given."""
        f = self._of.get(seq)
        if f is None:
            if parent is not None and parent in self._of:
                f = self.gram_fields(self._of[parent], parent[-1] if parent else None, seq[len(parent):])
            else:
                f = self.sequence_fields(seq)
            self._of[seq] = f
        return f

    def total(self, ac, f):
        return ac + self.lmwt * f.lm - self.wip * f.words + self.oov * f.oov


def _ranked(rows):
    """[(total, seq, ...)] -> by total descending; exactly equal totals by ascending key."""
    rows.sort(key=lambda r: -r[0])
    i = 0
    while i < len(rows):
        j = i + 1
        while j < len(rows) and rows[j][0] == rows[i][0]:
            j += 1
        if j - i > 1:
            rows[i:j] = sorted(rows[i:j], key=lambda r: DR.key_of(r[1]))
        i = j
    return rows


def beam_search(lp, grams, F, beam_width=None):
    """lp (T, V) f64 log-probabilities, grams {column: base-id tuple}, F a Fields -> (the final ranking: dicts of ids,
    total, ac, lm, words, oov; the smallest gap).  The masses follow gram_decode_ref.beam_search; a candidate's total is
    log(tot) + lmwt * lm - wip * words + oov_penalty * oov with tot in the frame's scaling."""
    T, V = lp.shape
    order = max((len(g) for g in grams.values()), default=1)
    slots = range(order + 1)
    cols = [(c, len(grams[c]), tuple(grams[c])) for c in range(1, V)]
    beam = {(): ([1.0] + [0.0] * order, [0] * (order + 1))}
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
        for seq, (p, col) in beam.items():
            tot = total(p)
            for c, k, g in cols:
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
                tt = F.total(math.log(tot), F.of(seq, parent.get(seq)))
                if tt > NEG_INF:                                       # (false for NaN as well)
                    rows.append((tt, seq, tot))
        rows = _ranked(rows)
        if beam_width is not None and len(rows) > beam_width:
            gap = min(gap, rows[beam_width - 1][0] - rows[beam_width][0])
            rows = rows[:beam_width]
        if not rows:
            return [], gap
        _, ex = math.frexp(rows[0][2])
        esum += ex
        beam = {}
        for _, seq, _ in rows:
            p, col = new[seq]
            p = [math.ldexp(v, -ex) for v in p]
            beam[seq] = (p, [c if v > 0.0 else 0 for v, c in zip(p, col)])
        ranking = [(tt, seq) for tt, seq, _ in rows]
    for hi, lo in zip(ranking, ranking[1:]):
        gap = min(gap, hi[0] - lo[0])
    out = []
    for _, seq in ranking:
        f = F.of(seq)
        ac = math.log(total(beam[seq][0])) + esum * LN2
        out.append(dict(ids=seq, total=F.total(ac, f), ac=ac, lm=f.lm, words=f.words, oov=f.oov))
    return out, gap


def enumerate_ranked(lp, grams, F):
    """All V**T paths grouped by base sequence; each sequence's fields from the sequence alone; ranked by total."""
    rows = []
    for seq, prob in DR.enumerate_labellings(lp, grams).items():
        if prob > 0.0:
            f = F.sequence_fields(seq)
            ac = math.log(prob)
            rows.append((F.total(ac, f), seq, ac, f))
    return [dict(ids=seq, total=tt, ac=ac, lm=f.lm, words=f.words, oov=f.oov) for tt, seq, ac, f in _ranked(rows)]


# ---- inputs shared by tests/test_gram_decode_lm_cpu.py and tests/test_gpu_gram_decode_lm.py ---------------------------
TINY_LABELS = ["_", "a", "b", " "]                                     # the alphabet of tests/golden/tiny_3gram.arpa
TINY_MODEL = "tiny_3gram.arpa"
AB, A_SP, SP_B, BA, A_SP_B = [1, 2], [1, 3], [3, 2], [2, 1], [1, 3, 2]  # `ab`, `a `, ` b`, `ba`, and `a b` (an inner space)
TINY_TABLES = [[], [AB], [A_SP, SP_B], [BA, AB, A_SP_B], [AB, A_SP, SP_B, BA], [BA, A_SP], [A_SP_B]]
# (table, T): every table at T = 2 (at most 64 paths); the deeper ones while V**T stays enumerable.  Three of the sixteen
# have more labellings than the widest beam holds (153, 214 and 155)
TINY_GRID = [(i, 2) for i in range(7)] + [(0, 3), (0, 4), (1, 3), (2, 3), (3, 3), (4, 3), (1, 4), (5, 3), (6, 3)]
PATH_CAP = 128                                                         # the widest beam: what an unpruned search can hold


def upper(labels):
    return [s.upper() for s in labels]


@functools.lru_cache(maxsize=None)
def tiny_case(i):
    """-> (R, V, label2ids, logits (T, V) f32 drawn once: the f32 and the f64 calls see the same numbers)."""
    table, T = TINY_GRID[i]
    R = len(TINY_LABELS)
    l2i = {R + j: list(g) for j, g in enumerate(TINY_TABLES[table])}
    V = R + len(l2i)
    x = (np.random.default_rng(500 + i).standard_normal((T, V)) * 2.0).astype(np.float32)
    return R, V, l2i, x


def tiny_fields(with_lm, case_sensitive):
    labels = TINY_LABELS if case_sensitive else upper(TINY_LABELS)
    if not with_lm:
        return Fields(labels, None, case_sensitive, wip=KNOBS["wip"])
    return Fields(labels, oracle_lm(TINY_MODEL), case_sensitive, **KNOBS)


@functools.lru_cache(maxsize=None)
def tiny_enumeration(i, with_lm, case_sensitive, f32=False):
    """The enumeration of tiny case i, of torch's f64 log-softmax of the logits (f32: of the f32 log-softmax)."""
    import torch
    R, V, l2i, x = tiny_case(i)
    t = torch.from_numpy(x)
    lp = torch.log_softmax(t if f32 else t.double(), -1).double().numpy()
    return enumerate_ranked(lp, GR.grams_of(R, V, l2i), tiny_fields(with_lm, case_sensitive))


PRUNED_WIDTHS = (2, 7, 32)
PRUNED_T, PRUNED_LENS = 14, [14, 9, 1, 0]
PRUNED = {
    "tiny_3gram.arpa": dict(labels=TINY_LABELS, grams=[AB, A_SP, SP_B, BA], seed=31),
    # ` `=1 a=2 b=3 c=4 d=5 e=6 '=7: be, ad, ca, bea, `d b` (an inner space), dead
    "lm_order4.arpa": dict(labels=["_", " ", "a", "b", "c", "d", "e", "'"],
                           grams=[[3, 6], [2, 5], [4, 2], [3, 6, 2], [5, 1, 3], [5, 6, 2, 5]], seed=32),
}


@functools.lru_cache(maxsize=None)
def pruned_case(model):
    """-> (R, V, label2ids, logits (4, 14, V) f32)."""
    m = PRUNED[model]
    R = len(m["labels"])
    l2i = {R + j: list(g) for j, g in enumerate(m["grams"])}
    V = R + len(l2i)
    x = (np.random.default_rng(m["seed"]).standard_normal((len(PRUNED_LENS), PRUNED_T, V)) * 2.0).astype(np.float32)
    return R, V, l2i, x


def pruned_fields(model, case_sensitive=True, with_lm=True):
    labels = PRUNED[model]["labels"] if case_sensitive else upper(PRUNED[model]["labels"])
    if not with_lm:
        return Fields(labels, None, case_sensitive, wip=KNOBS["wip"])
    return Fields(labels, oracle_lm(model), case_sensitive, **KNOBS)


@functools.lru_cache(maxsize=None)
def pruned_ref(model, W, case_sensitive=True, with_lm=True):
    """beam_search on the f64 log-softmax of every utterance of pruned_case(model): ([ranking per utterance], smallest gap)."""
    R, V, l2i, x = pruned_case(model)
    grams = GR.grams_of(R, V, l2i)
    lp = DR.log_softmax(x.astype(np.float64))
    out, gap = [], math.inf
    for b, n in enumerate(PRUNED_LENS):
        r, g = beam_search(lp[b, :n], grams, pruned_fields(model, case_sensitive, with_lm), W)
        out.append(r)
        gap = min(gap, g)
    return out, gap
