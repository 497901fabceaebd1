"""The checker of the ASG beam search restricted to a vocabulary, with label timestamps (TEST INFRASTRUCTURE ONLY): the
restatement of tests/asg_beam_ref.py with the rule of include/e2e_ctc.h (e2e_asg_beam_nbest_opt) -- a Search whose run skips
inadmissible first labels and extensions and records the frame every label's sequence was created at -- and admissible(), the
same rule as a stand-alone predicate of a sequence, for the enumerator.

L and Pref(L) come from lexicon_ref.Lexicon; the model's numbers from an object with OracleLM's interface (lexicon_ref.WordListLM
for a word list).  Neither module is edited.
"""
from asg_beam_ref import NEG_INF, LmFields, Search, enumerate_paths, expand, key_of, lse, may_follow  # noqa: F401
from lexicon_ref import Lexicon, WordListLM, arpa_words  # noqa: F401


def last_word(seq, chars, space_id):
    """The spelling of the run of labels after the last space, repeat labels expanded."""
    k = len(seq)
    while k > 0 and seq[k - 1] != space_id:
        k -= 1
    return expand(seq[k:], chars)


def step_allowed(y, c, chars, space_id, lexicon):
    """The rule for y + (c), y admissible: c no space -- the last word of y + (c) is in Pref(L); c the space -- y is empty or
    its last word is a word of L."""
    if c != space_id:
        return lexicon.fold(last_word(tuple(y) + (c,), chars, space_id).encode()) in lexicon.prefixes
    return len(y) == 0 or lexicon.fold(last_word(tuple(y), chars, space_id).encode()) in lexicon.words


def admissible(seq, V, R, space_id, chars, lexicon):
    """Is the sequence spellable, and does every one of its prefixes obey the rule?"""
    seq = tuple(seq)
    if not seq or any(a == b for a, b in zip(seq, seq[1:])):
        return False
    for i, c in enumerate(seq):
        if not may_follow(seq[i - 1] if i else None, c, V, R, space_id):
            return False
        if not step_allowed(seq[:i], c, chars[: V - R], space_id, lexicon):
            return False
    return True


class RestrictedSearch(Search):
    """asg_beam_ref.Search restricted to `lexicon` (None: unrestricted, only the frames are new)."""

    def __init__(self, V, R=0, space_id=-1, W=None, chars=None, lm=None, case_sensitive=True, lmwt=1.0, wip=0.0, oov=0.0,
                 lexicon=None):
        super().__init__(V, R, space_id, W, chars, lm, case_sensitive, lmwt, wip, oov)
        self.lexicon = lexicon
        self.died = False                       # a beam was left without a candidate
        self.least_members = None               # the smallest beam after any frame

    def allowed(self, y, c):
        return self.lexicon is None or step_allowed(y, c, self.chars[: self.V - self.R], self.space_id, self.lexicon)

    def note(self, beam):
        self.least_members = len(beam) if self.least_members is None else min(self.least_members, len(beam))

    def run(self, x, A, n):
        """As Search.run; every row also has `frames`: the frame at which each label's sequence was created (entered the beam
        the last time on this path)."""
        V = self.V
        root = LmFields((self.lm.word_index("<s>"),) if self.lm is not None else ())
        cands, frames = {}, {}
        for c in range(V):
            if may_follow(None, c, V, self.R, self.space_id) and self.allowed((), c):
                cands[(c,)] = (float(x[0][c]), self.child_fields(root, None, c))
        beam = self.ranked(cands, cut=True)
        frames = {seq: (0,) for seq, _, _, _ in beam}
        self.note(beam)
        for t in range(1, n):
            if not beam:
                self.died = True
                return []
            members = {seq: (ac, f) for seq, ac, f, _ in beam}
            stay, extn, fields, parent = {}, {}, {}, {}
            for seq, (s, f) in members.items():
                a = seq[-1]
                aa = float(A[a][a]) if A is not None else 0.0
                stay[seq] = s + aa + float(x[t][a])
                fields[seq] = f
                for c in range(V):
                    if c == a or not may_follow(a, c, V, self.R, self.space_id) or not self.allowed(seq, c):
                        continue
                    ca = float(A[c][a]) if A is not None else 0.0
                    child = seq + (c,)
                    extn[child] = s + ca + float(x[t][c])
                    if child not in members:
                        fields[child] = self.child_fields(f, a, c)
                        parent[child] = seq
            cands = {seq: (lse(stay.get(seq, NEG_INF), extn.get(seq, NEG_INF)), fields[seq]) for seq in set(stay) | set(extn)}
            beam = self.ranked(cands, cut=True)
            frames = {seq: frames[seq] if seq in members else frames[parent[seq]] + (t,) for seq, _, _, _ in beam}
            self.note(beam)
        if not beam:
            self.died = True
        for hi, lo in zip(beam, beam[1:]):
            if hi[3] != lo[3]:
                self.min_gap = min(self.min_gap, hi[3] - lo[3])
        return [dict(ids=seq, total=tot, ac=ac, lm=f.lm, words=f.words, oov=f.oov, frames=frames[seq]) for seq, ac, f, tot in beam]


def beam(x, A, x_len, V, R=0, space_id=-1, W=None, chars=None, lm=None, case_sensitive=True, lmwt=1.0, wip=0.0,
         oov_penalty=0.0, lexicon=None, stats=None):
    """asg_beam_ref.beam restricted to `lexicon`: ([ranking per utterance], smallest margin).  `stats`, a dict, receives
    `died` (some utterance's beam was left empty) and `least_members` (the smallest beam after any frame)."""
    s = RestrictedSearch(V, R, space_id, W, chars, lm, case_sensitive, lmwt, wip, oov_penalty, lexicon)
    out = [s.run(x[b], A, int(x_len[b])) if 1 <= int(x_len[b]) <= len(x[b]) else [] for b in range(len(x))]
    if stats is not None:
        stats.update(died=s.died, least_members=s.least_members)
    return out, s.min_gap
