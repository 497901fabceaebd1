"""Test-side restatement of Gram-CTC decoding (the definition of include/e2e_ctc.h) in plain Python: dicts keyed by
base-id tuples, the header's 64-bit key for ties, the same probability-domain scaling.  Besides the ranked hypotheses it
reports the smallest relative gap between the last kept and the first dropped hypothesis at any frame -- the margin by
which the pruned search is decided.  Also: the probabilities of every labelling by enumeration of all V**T paths, the
three-line greedy definition, and the fixed-seed inputs that the CPU and the GPU tests share.  It shares no code with the
product; only tests import it."""
import itertools
import math

import numpy as np

import gram_ref as GR

KEY0, PRIME, MASK = 0xcbf29ce484222325, 0x100000001b3, (1 << 64) - 1
LN2 = math.log(2.0)


def key_of(seq):
    k = KEY0
    for i in seq:
        k = ((k ^ int(i)) * PRIME) & MASK
    return k


def enumerate_labellings(lp, grams):
    """lp (T, V) f64 log-probabilities -> {base-id tuple: probability}, summed over every one of the V**T paths."""
    T, V = lp.shape
    parts = {}
    for path in itertools.product(range(V), repeat=T):
        s = 0.0
        for t, c in enumerate(path):
            s += lp[t, c]
        parts.setdefault(GR.labelling(path, grams), []).append(math.exp(s))
    return {seq: math.fsum(v) for seq, v in parts.items()}


def _ranked(cands):
    """[(tot, seq)] -> ordered by tot descending; exactly equal totals by ascending key."""
    cands.sort(key=lambda c: -c[0])
    i = 0
    while i < len(cands):
        j = i + 1
        while j < len(cands) and cands[j][0] == cands[i][0]:
            j += 1
        if j - i > 1:
            cands[i:j] = sorted(cands[i:j], key=lambda c: key_of(c[1]))
        i = j
    return cands


def beam_search(lp, grams, beam_width=None):
    """lp (T, V) f64 log-probabilities, grams {column: base-id tuple} -> ([(sequence, log tot)] ranked, smallest gap).
    beam_width None: nothing is cut.  A hypothesis is a base-id tuple with slots p[0 .. order] (p[0]: paths ending in the
    blank; p[k]: paths whose last column is the order-k gram col[k] that spells the last k ids).  A frame's stay shares are
    kept per sequence as slot lists, its extension shares as (slot, share, column) items per sequence; a total is the sum
    over the slots 0 .. order of stay + extension."""
    T, V = lp.shape
    order = max((len(g) for g in grams.values()), default=1)
    slots = range(order + 1)
    cols = [(c, len(grams[c]), tuple(grams[c])) for c in range(1, V)]
    beam = {(): ([1.0] + [0.0] * order, [0] * (order + 1))}
    esum, gap = 0, math.inf

    def slots_of(seq, stay, ext):
        p, col = stay.get(seq) or ([0.0] * (order + 1), [0] * (order + 1))
        p, col = list(p), list(col)
        for k, v, c in ext.get(seq, ()):
            p[k] += v
            col[k] = c
        return p, col

    def total(p):
        tot = 0.0
        for k in slots:
            tot += p[k]
        return tot

    for t in range(T):
        yt = np.exp(lp[t])
        y = yt.tolist()
        stay, ext = {}, {}
        for seq, (p, col) in beam.items():
            tot = total(p)
            sp, sc = [0.0] * (order + 1), [0] * (order + 1)
            sp[0] = tot * y[0]
            for k in range(1, order + 1):
                if p[k] > 0.0:
                    sp[k] = p[k] * y[col[k]]
                    sc[k] = col[k]
            stay[seq] = (sp, sc)
            shares = (tot * yt).tolist()                       # src = tot but for a column that sits in its own slot
            for k in range(1, order + 1):
                if p[k] > 0.0:
                    src = 0.0
                    for kk in slots:
                        if kk != k:
                            src += p[kk]
                    shares[col[k]] = src * y[col[k]] if src > 0.0 else 0.0
            for c, k, g in cols:
                v = shares[c]
                if v > 0.0:
                    new = seq + g
                    items = ext.get(new)
                    if items is None:
                        ext[new] = [(k, v, c)]
                    else:
                        items.append((k, v, c))
        seqs, tots = [], []
        for seq in stay:
            seqs.append(seq)
            tots.append(total(slots_of(seq, stay, ext)[0]))
        for seq, items in ext.items():
            if seq not in stay:
                seqs.append(seq)
                tots.append(items[0][1] if len(items) == 1 else total(slots_of(seq, stay, ext)[0]))
        arr = np.array(tots)
        if beam_width is not None and len(tots) > beam_width:
            # (everything at or above the (beam_width + 1)-th largest total, then the exact order among those)
            floor = np.partition(arr, len(tots) - beam_width - 1)[len(tots) - beam_width - 1]
            pick = np.nonzero(arr >= floor)[0].tolist()
        else:
            pick = range(len(tots))
        cands = _ranked([(tots[i], seqs[i]) for i in pick if tots[i] > 0.0])
        if beam_width is not None and len(cands) > beam_width:
            kept, dropped = cands[beam_width - 1][0], cands[beam_width][0]
            gap = min(gap, (kept - dropped) / kept)
            cands = cands[:beam_width]
        if not cands:
            return [], gap
        _, ex = math.frexp(cands[0][0])
        esum += ex
        beam = {}
        for _, seq in cands:
            p, col = slots_of(seq, stay, ext)
            p = [math.ldexp(v, -ex) for v in p]
            beam[seq] = (p, [c if v > 0.0 else 0 for v, c in zip(p, col)])
    out = [(total(p), seq) for seq, (p, _) in beam.items()]
    return [(seq, math.log(tot) + esum * LN2) for tot, seq in _ranked(out)], gap


def greedy(x, n, grams):
    """x (T, V), the first n frames -> (base ids, collapsed columns): the definition in three lines."""
    am = np.argmax(x[:n], axis=1).tolist()
    cols = [c for i, c in enumerate(am) if c != 0 and (i == 0 or c != am[i - 1])]
    return [i for c in cols for i in grams[c]], cols


# ---- inputs shared by tests/test_gram_decode_cpu.py and tests/test_gpu_gram_decode.py ---------------------------------
def tiny_cases():
    """The 300 cases of gram_ref.random_tiny_case(default_rng(7)): [(R, V, label2ids, logits (T, V) f64)]."""
    rng = np.random.default_rng(7)
    out = []
    for _ in range(300):
        R, V, l2i, x, _ = GR.random_tiny_case(rng)
        out.append((R, V, l2i, x))
    return out


def log_softmax(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max(axis=-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


def random_table(rng, R, *counts, extra=()):
    """counts[i] random grams of order i + 2 over the base labels 1 .. R-1, then one of every order in `extra`
    -> (label2ids, V)."""
    l2i, seen, c = {}, set(), R
    for k, n in list(enumerate(counts, start=2)) + [(k, 1) for k in extra]:
        have = 0
        while have < n:
            s = tuple(int(v) for v in rng.integers(1, R, size=k))
            if s not in seen:
                seen.add(s)
                l2i[c] = list(s)
                c += 1
                have += 1
    return l2i, c


PRUNED_WIDTHS = (1, 2, 7, 32, 100)
PRUNED_SCALES = (1.0, 3.0)


def pruned_cases(seed=3):
    """The pruned GPU test's inputs: R = 6, 14 random grams of orders 2-3 and one of order 8 (V = 21); for every width of
    PRUNED_WIDTHS and scale of PRUNED_SCALES three ragged utterances of 30..60 frames.
    -> (R, V, label2ids, {(width, scale): (logits (3, 60, V) f64, lengths (3,))})."""
    rng = np.random.default_rng(seed)
    R = 6
    l2i, V = random_table(rng, R, 8, 6, extra=(8,))
    assert V == 21
    batches = {}
    for w in PRUNED_WIDTHS:
        for s in PRUNED_SCALES:
            xl = rng.integers(30, 61, size=3)
            xl[0] = 60
            batches[(w, s)] = (rng.normal(size=(3, 60, V)) * s, xl.astype(np.int64))
    return R, V, l2i, batches


def headline_case(seed=4):
    """One case at the loss's headline table: R = 29, 300 bigrams and 50 trigrams (V = 379), B = 2, T = 30, width 100."""
    rng = np.random.default_rng(seed)
    R = 29
    l2i, V = random_table(rng, R, 300, 50)
    assert V == 379
    return R, V, l2i, rng.normal(size=(2, 30, V)), np.array([30, 26], dtype=np.int64), 100


_cache = {}


def pruned_reference():
    """beam_search on every utterance of pruned_cases() and headline_case(), once per process:
    {(width, scale) or "headline": [([(sequence, score)], gap) per utterance]}."""
    if "pruned" not in _cache:
        R, V, l2i, batches = pruned_cases()
        grams = GR.grams_of(R, V, l2i)
        ref = {}
        for (w, s), (x, xl) in batches.items():
            lp = log_softmax(x)
            ref[(w, s)] = [beam_search(lp[b, :int(xl[b])], grams, w) for b in range(len(xl))]
        R, V, l2i, x, xl, w = headline_case()
        grams = GR.grams_of(R, V, l2i)
        lp = log_softmax(x)
        ref["headline"] = [beam_search(lp[b, :int(xl[b])], grams, w) for b in range(len(xl))]
        _cache["pruned"] = ref
    return _cache["pruned"]


def tiny_reference():
    """Enumeration on every tiny case, once per process: [{sequence: probability}] for the f64 log-softmax of the logits."""
    if "tiny" not in _cache:
        _cache["tiny"] = [enumerate_labellings(log_softmax(x), GR.grams_of(R, V, l2i)) for R, V, l2i, x in tiny_cases()]
    return _cache["tiny"]
