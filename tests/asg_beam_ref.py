"""The checker of the ASG beam search (TEST INFRASTRUCTURE ONLY): a plain-Python restatement of the definition in
include/e2e_ctc.h (e2e_asg_beam_nbest) -- dicts keyed by label tuples, math log-sum --, and an enumerator over all V**T
paths that groups them by labelling.

LM numbers come from an object with oracle_lib.OracleLM's interface (word_index / base_score), as in lexicon_ref.py.
"""
import itertools
import math

NEG_INF = float("-inf")
LN10 = math.log(10.0)
KEY_BASIS, KEY_PRIME, MASK64 = 0xcbf29ce484222325, 0x100000001b3, (1 << 64) - 1


def lse(a, b):
    """log(exp(a) + exp(b)), symmetric in its arguments; -inf is "no share"."""
    hi, lo = (a, b) if a > b else (b, a)
    if lo == NEG_INF:
        return hi
    return hi + math.log1p(math.exp(lo - hi))


def key_of(seq):
    """The sequence's 64-bit key: the kernel's, and the Gram-CTC search's."""
    k = KEY_BASIS
    for c in seq:
        k = ((k ^ c) * KEY_PRIME) & MASK64
        if k == 0:
            k = 1
    return k


def may_follow(last, c, V, R, space_id):
    """May label c != last follow a sequence that ends in `last` (None: nothing yet)?"""
    nch = V - R
    return c < nch or (last is not None and last < nch and last != space_id)


def spellable(seq, V, R, space_id):
    return len(seq) > 0 and all(a != b for a, b in zip(seq, seq[1:])) and \
        all(may_follow(seq[i - 1] if i else None, c, V, R, space_id) for i, c in enumerate(seq))


def expand(seq, chars):
    """The sentence: repeat label r (id len(chars) + r - 1) is the character before it, r more times."""
    out = []
    for i in seq:
        if i < len(chars):
            out.append(chars[i])
        elif out:
            out.extend([out[-1]] * (i - len(chars) + 1))
    return "".join(out)


class LmFields:
    """lm_score, num_words, num_oov and the LM state: functions of the sequence alone (get_next_prefix's rules)."""
    __slots__ = ("lm", "lm_before", "words", "oov", "oov_before", "word", "st", "st_before")

    def __init__(self, st=()):
        self.lm = self.lm_before = 0.0
        self.words = self.oov = self.oov_before = 0
        self.word = ""
        self.st = self.st_before = st


class Search:
    def __init__(self, V, R=0, space_id=-1, W=None, chars=None, lm=None, case_sensitive=True, lmwt=1.0, wip=0.0, oov=0.0):
        self.V, self.R, self.space_id, self.W = V, R, space_id, W
        self.chars, self.lm, self.case_sensitive = chars, lm, case_sensitive
        self.lmwt = lmwt if lm is not None else 0.0
        self.wip, self.oov = wip, oov
        # the smallest gap between the W-th and the (W+1)-th total over all cuts (0: an exact tie, cut by key) and between
        # neighbours of a final ranking whose totals differ
        self.min_gap = math.inf

    def child_fields(self, p, last, c):
        n = LmFields()
        new_word = c != self.space_id and (last is None or last == self.space_id)
        n.words = p.words + (1 if new_word else 0)
        if self.lm is None:
            return n
        if c == self.space_id:                                            # a space copies the fields
            n.lm, n.lm_before, n.oov, n.oov_before = p.lm, p.lm_before, p.oov, p.oov_before
            n.word, n.st, n.st_before = p.word, p.st, p.st_before
            return n
        nch = self.V - self.R
        piece = self.chars[c] if c < nch else self.chars[last] * (c - nch + 1)
        n.word = piece if new_word else p.word + piece
        if new_word:
            n.st_before, n.lm_before, n.oov_before = p.st, p.lm, p.oov
        else:
            n.st_before, n.lm_before, n.oov_before = p.st_before, p.lm_before, p.oov_before
        w = n.word if self.case_sensitive else "".join(ch.lower() if "A" <= ch <= "Z" else ch for ch in n.word)
        wi = self.lm.word_index(w)
        s, st = self.lm.base_score(list(n.st_before), wi)
        n.st = tuple(st)
        n.lm = n.lm_before + s / LN10                                      # quirk Q8: divides by ln 10
        n.oov = n.oov_before + (1 if wi == 0 else 0)
        return n

    def total(self, ac, f):
        return ac + f.lm * self.lmwt - f.words * self.wip + f.oov * self.oov

    def ranked(self, cands, cut):
        """cands: {seq: (ac, fields)} -> [(seq, ac, fields, total)] by total descending, key ascending.  A candidate whose
        total is -inf or NaN is no candidate: it is dropped before the sort and before the cut."""
        rows = [(seq, ac, f, self.total(ac, f)) for seq, (ac, f) in cands.items()]
        rows = [r for r in rows if r[3] > NEG_INF]
        rows.sort(key=lambda r: -r[3])
        i = 0
        while i < len(rows):                                              # (a key costs its sequence's length: only ties ask)
            j = i + 1
            while j < len(rows) and rows[j][3] == rows[i][3]:
                j += 1
            if j - i > 1:
                rows[i:j] = sorted(rows[i:j], key=lambda r: key_of(r[0]))
            i = j
        if cut and self.W is not None and len(rows) > self.W:
            self.min_gap = min(self.min_gap, rows[self.W - 1][3] - rows[self.W][3])
            rows = rows[: self.W]
        return rows

    def run(self, x, A, n):
        """x: (T,V) rows of floats, A: (V,V) rows A[to][from] or None, n frames -> the final ranking: dicts of ids, total,
        ac, lm, words, oov."""
        V = self.V
        root = LmFields((self.lm.word_index("<s>"),) if self.lm is not None else ())
        cands = {}
        for c in range(V):
            if may_follow(None, c, V, self.R, self.space_id):
                cands[(c,)] = (float(x[0][c]), self.child_fields(root, None, c))
        beam = self.ranked(cands, cut=True)
        for t in range(1, n):
            if not beam:                                                  # nothing has a number for a total: no hypotheses
                return []
            members = {seq: (ac, f) for seq, ac, f, _ in beam}
            stay, extn, fields = {}, {}, {}
            for seq, (s, f) in members.items():
                a = seq[-1]
                aa = float(A[a][a]) if A is not None else 0.0
                stay[seq] = s + aa + float(x[t][a])
                fields[seq] = f
                for c in range(V):
                    if c == a or not may_follow(a, c, V, self.R, self.space_id):
                        continue
                    ca = float(A[c][a]) if A is not None else 0.0
                    child = seq + (c,)
                    extn[child] = s + ca + float(x[t][c])
                    if child not in members:
                        fields[child] = self.child_fields(f, a, c)
            cands = {seq: (lse(stay.get(seq, NEG_INF), extn.get(seq, NEG_INF)), fields[seq]) for seq in set(stay) | set(extn)}
            beam = self.ranked(cands, cut=True)
        for hi, lo in zip(beam, beam[1:]):                                # (the final order is compared exactly)
            if hi[3] != lo[3]:
                self.min_gap = min(self.min_gap, hi[3] - lo[3])
        return [dict(ids=seq, total=tot, ac=ac, lm=f.lm, words=f.words, oov=f.oov) for seq, ac, f, tot in beam]


def beam(x, A, x_len, V, R=0, space_id=-1, W=None, chars=None, lm=None, case_sensitive=True, lmwt=1.0, wip=0.0,
         oov_penalty=0.0):
    """The whole final ranking of every utterance of x (B,T,V) and the smallest margin met (Search.min_gap):
    ([ranking per utterance], gap).  W None: unbounded.  An utterance with x_len outside [1,T] has an empty ranking."""
    s = Search(V, R, space_id, W, chars, lm, case_sensitive, lmwt, wip, oov_penalty)
    out = [s.run(x[b], A, int(x_len[b])) if 1 <= int(x_len[b]) <= len(x[b]) else [] for b in range(len(x))]
    return out, s.min_gap


def enumerate_paths(x, A, n, V, R=0, space_id=-1):
    """{labelling: ac} over all V**n paths of the first n frames of x (T,V), unspellable labellings dropped.  A path whose
    score is -inf contributes nothing, and a labelling without any other path is absent."""
    groups = {}
    for path in itertools.product(range(V), repeat=n):
        sc = float(x[0][path[0]])
        for t in range(1, n):
            sc += (float(A[path[t]][path[t - 1]]) if A is not None else 0.0) + float(x[t][path[t]])
        seq = tuple(c for i, c in enumerate(path) if i == 0 or c != path[i - 1])
        groups.setdefault(seq, []).append(sc)
    out = {}
    for seq, scores in groups.items():
        scores = [s for s in scores if s > NEG_INF]
        if scores and spellable(seq, V, R, space_id):
            m = max(scores)
            out[seq] = m + math.log(math.fsum(math.exp(s - m) for s in scores))
    return out
