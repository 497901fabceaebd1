"""The checker of the vocabulary-restricted beam search (TEST INFRASTRUCTURE ONLY): a Python restatement of
oracle/ctc_oracle.c beam_one / next_prefix with the lexicon rule of DESIGN.md 4.4, returning the whole final ranking.

Ownership is the oracle's, through CPython's reference counts instead of explicit ones: a prefix is owned by the beam list
and by each living child's strong `parent`; a parent's `children[c]` is a weakref that expires when the child dies, so a
pruned child that a descendant keeps alive is still found and not re-created (quirk Q7).  The functions below therefore keep
no stray strong reference to a prefix beyond the beam: no prefix survives in a local variable across a pruning.

A prefix records the frame at which it was created (run() returns them per label as `frames`), and margin() says by how
little the search was decided (tests/ctc_beam_fuzz_util.py leaves out what f64 round-off could decide otherwise).

LM numbers come from oracle_lib.OracleLM (base_score / word_index): the arithmetic is the oracle's, bit for bit.
"""
import math
import weakref

NEG_INF = float("-inf")
LN10 = math.log(10.0)


def lse(a, b):
    """oracle_log_sum_exp: log(1.0 + x), not log1p (src/utils/math_utils.h:8-16)."""
    if a == NEG_INF:
        return b
    if b == NEG_INF:
        return a
    if a > b:
        return a + math.log(1.0 + math.exp(b - a))
    return b + math.log(1.0 + math.exp(a - b))


class Lexicon:
    """L and Pref(L) of a word list, spelled as the LM lookup spells a beam's words: UTF-8 bytes, A-Z folded unless case
    sensitive."""

    def __init__(self, words, case_sensitive=True):
        self.case_sensitive = case_sensitive
        self.words = {self.fold(w.encode()) for w in words}
        self.prefixes = {w[:n] for w in self.words for n in range(1, len(w) + 1)}

    def fold(self, b):
        return b if self.case_sensitive else bytes(c + 32 if 65 <= c <= 90 else c for c in b)

    def spelling_class(self, s):
        b = self.fold(s.encode())
        return (1 if b in self.words else 0) | (2 if any(w != b and w.startswith(b) for w in self.words) and b else 0)


def arpa_words(path):
    """The words of an ARPA file's \\1-grams: section without <unk>, <s>, </s>."""
    words, on = [], False
    for line in open(path, encoding="utf-8"):
        line = line.strip()
        if line.startswith("\\"):
            on = line == "\\1-grams:"
            continue
        f = line.split()
        if on and len(f) >= 2 and f[1] not in ("<unk>", "<s>", "</s>"):
            words.append(f[1])
    return words


class WordListLM:
    """What e2e_lm_load_words builds, with OracleLM's interface: order 1, every word and <unk> at log10 p = 0."""

    def __init__(self, words, case_sensitive=True):
        self.case_sensitive = case_sensitive
        self.ids = {}
        for w in ["<unk>", "<s>", "</s>"] + list(words):
            self.ids.setdefault(w if case_sensitive else w.lower(), len(self.ids))

    def word_index(self, w):
        return self.ids.get(w, 0)

    def base_score(self, ctx, word):
        return 0.0, []


class Prefix:
    __slots__ = ("pb", "pnb", "prev_pb", "prev_pnb", "last_char", "lm_score", "lm_before", "num_words", "num_oov",
                 "num_oov_before", "last_word", "st", "st_before", "parent", "children", "frame", "__weakref__")

    def __init__(self):
        self.pb = self.pnb = self.prev_pb = self.prev_pnb = NEG_INF
        self.last_char = -1
        self.lm_score = self.lm_before = 0.0
        self.num_words = self.num_oov = self.num_oov_before = 0
        self.last_word = ()
        self.st = self.st_before = ()
        self.parent = None
        self.children = {}
        self.frame = -1                          # the frame at which it was created (the root: none)


class Search:
    def __init__(self, labels, blank, W, lm=None, case_sensitive=True, lmwt=1.0, wip=0.0, oov=-1000.0, lexicon=None):
        self.labels, self.blank, self.W, self.lm = list(labels), blank, W, lm
        self.space_id = self.labels.index(" ") if " " in self.labels else -1
        self.case_sensitive = case_sensitive
        self.lmwt = lmwt if lm is not None else 0.0                     # .cpp:72-74
        self.wip, self.oov, self.lexicon = wip, oov, lexicon
        self.min_gap = math.inf                  # smallest positive gap between the W-th and (W+1)-th score over all cuts
        self.t, self.row = -1, None              # the frame being searched and its row
        self.final_gap = math.inf                # smallest gap between neighbours of the final rankings whose totals differ
        self.odd_tie = False                     # a zero gap, at a cut or in a final ranking, that is not the same arithmetic

    def spell(self, chars):
        return "".join(self.labels[c] for c in chars)

    def word_idx(self, chars):
        s = self.spell(chars)
        return self.lm.word_index(s if self.case_sensitive else s.lower())

    def score(self, p):
        return lse(p.prev_pnb, p.prev_pb) + p.lm_score * self.lmwt - p.num_words * self.wip + p.num_oov * self.oov

    def allowed(self, p, ch):
        """The rule: may the child (p, ch) be created?"""
        lx = self.lexicon
        if lx is None:
            return True
        if ch != self.space_id:
            new_word = p.num_words == 0 or p.last_char == self.space_id
            w = (ch,) if new_word else p.last_word + (ch,)
            return lx.fold(self.spell(w).encode()) in lx.prefixes
        if p.parent is not None and p.last_char != self.space_id:
            return lx.fold(self.spell(p.last_word).encode()) in lx.words
        return True

    def next_prefix(self, p, ch):
        """get_next_prefix, .cpp:247-312 -> (child or None, is_new)."""
        ref = p.children.get(ch)
        q = ref() if ref is not None else None
        if q is not None:
            return q, False                                              # :250-252, Q7 included
        if not self.allowed(p, ch):
            return None, False
        n = Prefix()
        p.children[ch] = weakref.ref(n)
        n.last_char = ch
        n.num_words = p.num_words
        new_word = ch != self.space_id and (p.num_words == 0 or p.last_char == self.space_id)
        if new_word:
            n.num_words += 1
        if self.lm is not None or self.lexicon is not None:
            if ch != self.space_id:
                n.last_word = (ch,) if new_word else p.last_word + (ch,)
            else:
                n.last_word = p.last_word
        if self.lm is not None:
            if ch != self.space_id:
                wi = self.word_idx(n.last_word)
                if new_word:
                    n.st_before, n.lm_before, n.num_oov_before = p.st, p.lm_score, p.num_oov
                else:
                    n.st_before, n.lm_before, n.num_oov_before = p.st_before, p.lm_before, p.num_oov_before
                s, st = self.lm.base_score(list(n.st_before), wi)
                n.st = tuple(st)
                n.lm_score = 0.0 + (n.lm_before + s / LN10)              # Q8: divides by ln 10
                n.num_oov = n.num_oov_before + (wi == 0)
            else:
                n.lm_score, n.lm_before = p.lm_score, p.lm_before
                n.num_oov, n.num_oov_before = p.num_oov, p.num_oov_before
                n.st, n.st_before = p.st, p.st_before
        n.parent = p
        n.frame = self.t
        return n, True

    def same_arithmetic(self, a, b):
        """An exact tie of two scores is decided by position (Q9).  It is the same on any machine only where both numbers come
        out of the same operations on the same operands: both -inf, or two children of one parent created in this frame by
        bit-equal emissions (neither repeats the parent's label), with the same words behind them."""
        if self.score(a) == NEG_INF and self.score(b) == NEG_INF:
            return True
        p = a.parent
        if p is None or p is not b.parent or a.frame != self.t or b.frame != self.t or self.row is None:
            return False
        if a.last_char == p.last_char or b.last_char == p.last_char or self.row[a.last_char] != self.row[b.last_char]:
            return False
        return (a.lm_score, a.num_words, a.num_oov) == (b.lm_score, b.num_words, b.num_oov)

    def margin(self):
        """The smaller of the smallest positive gap at any cut and the smallest gap between neighbours of the final rankings
        whose totals differ; 0 where an exact tie was met that is not the same arithmetic."""
        return 0.0 if self.odd_tie else min(self.min_gap, self.final_gap)

    def step(self, beam, row, t=-1):
        self.t, self.row = t, row
        fresh = []
        for ch in range(len(row)):                                       # char outer, prefix inner, :370-395
            cur = row[ch]
            for p in beam:
                if ch == self.blank:
                    p.pb = lse(p.pb, cur + lse(p.prev_pnb, p.prev_pb))
                    continue
                q, is_new = self.next_prefix(p, ch)
                if is_new:
                    fresh.append(q)
                if ch == p.last_char:
                    if q is not None:
                        q.pnb = lse(q.pnb, cur + p.prev_pb)
                    p.pnb = lse(p.pnb, cur + p.prev_pnb)                 # the parent's share, child or no child
                elif q is not None:
                    q.pnb = lse(q.pnb, cur + lse(p.prev_pnb, p.prev_pb))
        beam = beam + fresh
        for p in beam:                                                   # next_step, :337-342
            p.prev_pb, p.prev_pnb, p.pb, p.pnb = p.pb, p.pnb, NEG_INF, NEG_INF
        if len(beam) > self.W:                                           # :405-415
            beam = self.ranked(beam, cut=True)[: self.W]
        return beam

    def ranked(self, beam, cut=False):
        sc = [self.score(p) for p in beam]
        order = sorted(range(len(beam)), key=lambda i: (-sc[i], i))      # score descending, position ascending
        if cut:
            gap = sc[order[self.W - 1]] - sc[order[self.W]]
            if gap > 0:
                self.min_gap = min(self.min_gap, gap)
            elif not self.same_arithmetic(beam[order[self.W - 1]], beam[order[self.W]]):
                self.odd_tie = True
        return [beam[i] for i in order]

    def run(self, lp, x_len):
        """lp: (T,V) rows of floats -> the final ranking: dicts of ids, total, ctc, lm, words, oov."""
        root = Prefix()
        root.prev_pb = 0.0
        if self.lm is not None:
            root.st = root.st_before = (self.lm.word_index("<s>"),)
        beam = [root]
        for t in range(int(x_len)):
            beam = self.step(beam, [float(v) for v in lp[t]], t)
        out = []
        final = self.ranked(beam)
        for hi, lo in zip(final, final[1:]):
            gap = self.score(hi) - self.score(lo)
            if gap > 0:
                self.final_gap = min(self.final_gap, gap)
            elif not self.same_arithmetic(hi, lo):
                self.odd_tie = True
        for p in final:
            ids, frames, q = [], [], p
            while q is not None:                                         # get_sentence, :232-245
                if q is p or q.parent is not None:
                    ids.append(q.last_char)
                    frames.append(q.frame)
                q = q.parent
            out.append(dict(ids=tuple(reversed(ids)), total=self.score(p), ctc=lse(p.prev_pnb, p.prev_pb), lm=p.lm_score,
                            words=p.num_words, oov=p.num_oov, frames=tuple(reversed(frames))))
        return out


def beam(lp, x_len, blank, W, labels, lm=None, case_sensitive=True, lmwt=1.0, wip=0.0, oov_penalty=-1000.0, lexicon=None):
    """The ranking of every utterance of lp (B,T,V) and the smallest positive cut gap met: ([ranking per utterance], gap)."""
    s = Search(labels, blank, W, lm, case_sensitive, lmwt, wip, oov_penalty, lexicon)
    out = [s.run(lp[b], x_len[b]) for b in range(len(lp))]
    return out, s.min_gap
