"""The checker of the beam search over a model with custom transcriptions (TEST INFRASTRUCTURE ONLY): lexicon_ref.Search with
the three things DESIGN.md 4.4 "Custom transcriptions" changes -- a prefix's last word is looked up by its tuple of label ids,
a key with several words (homophones) gives the word the model scores highest in the state before the word (exact ties: the
earliest listed), and the restriction's prefixes end on label boundaries.  LM numbers are the oracle's (OracleLM.base_score)
or WordListLM's."""
import lexicon_ref as LR


class Table:
    """Wd of a transcription lexicon over a model: key (tuple of label ids) -> word ids in the order of first appearance.
    entries: (word, tokens) with tokens label strings; lm: OracleLM or WordListLM; an entry whose word the model does not
    list (id 0) is dropped, as are none with WordListLM built from the same words."""

    def __init__(self, entries, labels, lm, case_sensitive=True):
        self.keys, self.dropped = {}, 0
        for word, toks in entries:
            toks = toks.split() if isinstance(toks, str) else list(toks)
            wi = lm.word_index(word if case_sensitive else word.lower())
            if wi == 0:
                self.dropped += 1
                continue
            ids = self.keys.setdefault(tuple(labels.index(t) for t in toks), [])
            if wi not in ids:
                ids.append(wi)
        self.prefixes = {k[:n] for k in self.keys for n in range(1, len(k) + 1)}


class _Chooser:
    """The model as Search sees it: base_score of a tuple of candidates is rule 2's choice among them."""

    def __init__(self, lm):
        self.lm = lm
        self.min_choice = float("inf")    # smallest non-zero difference (log10 p) between the best and the second word of a key
        self.choices = {}                 # key (the tuple of candidates) -> the words chosen for it, by any query

    def word_index(self, w):
        return self.lm.word_index(w)

    def base_score(self, ctx, word):
        if not isinstance(word, tuple):
            return self.lm.base_score(ctx, word)
        best, scores = None, []
        for w in word:
            s, st = self.lm.base_score(ctx, w)
            scores.append(s)
            if best is None or s > best[0]:                    # (strictly greater: a tie stays with the earliest)
                best = (s, st, w)
        top = sorted(scores, reverse=True)
        if top[0] != top[1]:
            self.min_choice = min(self.min_choice, top[0] - top[1])
        self.choices.setdefault(word, set()).add(best[2])
        return best[:2]


class Search(LR.Search):
    def __init__(self, labels, blank, W, lm, table, restrict=False, lmwt=1.0, wip=0.0, oov=-1000.0):
        super().__init__(labels, blank, W, _Chooser(lm), True, lmwt, wip, oov, lexicon=table if restrict else None)
        self.table = table

    def margin(self):
        """lexicon_ref.Search.margin, and the closest choice among homophones: less is f32 against f64 rounding."""
        return min(super().margin(), self.lm.min_choice)

    def word_idx(self, chars):
        ids = self.table.keys.get(tuple(chars), ())
        return 0 if not ids else ids[0] if len(ids) == 1 else tuple(ids)   # (a tuple is never == 0: homophones are no OOV)

    def allowed(self, p, ch):
        t = self.lexicon
        if t is None:
            return True
        if ch != self.space_id:
            new_word = p.num_words == 0 or p.last_char == self.space_id
            return ((ch,) if new_word else p.last_word + (ch,)) in t.prefixes
        if p.parent is not None and p.last_char != self.space_id:
            return tuple(p.last_word) in t.keys
        return True


def beam(lp, x_len, blank, W, labels, lm, table, restrict=False, lmwt=1.0, wip=0.0, oov_penalty=-1000.0):
    """The ranking of every utterance of lp (B,T,V) and the smallest positive cut gap met, like lexicon_ref.beam."""
    s = Search(labels, blank, W, lm, table, restrict, lmwt, wip, oov_penalty)
    out = [s.run(lp[b], x_len[b]) for b in range(len(lp))]
    return out, s.min_gap


def words_of(ids, labels, lm, table):
    """What e2e_lm_transcribe answers: the chosen word id of every piece between spaces, in the running context."""
    space = labels.index(" ") if " " in labels else -1
    ch, ctx, out, piece = _Chooser(lm), [lm.word_index("<s>")], [], []
    for k in list(ids) + [space]:
        if k != space:
            piece.append(k)
            continue
        if piece:
            cand = table.keys.get(tuple(piece), [0])
            best = max(cand, key=lambda w: (ch.base_score(ctx, w)[0], -cand.index(w)))
            ctx = ch.base_score(ctx, best)[1]
            out.append(best)
            piece = []
    return out
