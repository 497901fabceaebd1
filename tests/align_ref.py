"""A plain f64 statement of what a forced alignment has to be (TEST INFRASTRUCTURE ONLY; numpy, no kernel-shaped code,
nothing shared with oracle/ctc_oracle.c).

The oracle restates upstream's alignment function statement by statement, its tie rule and its quirks included, and the
kernel is compared with it label for label.  This module checks what neither of them is allowed to get wrong together:
that the frame labelling is a legal walk through the lattice of the extended labelling, and that no other walk scores
higher.  `path_score` adds the emissions in frame order, which is the very sequence of f64 additions the max-plus
recurrence performs along the path it chooses, so the check is `path_score == best_score` EXACTLY -- no tolerance.

The lattice: cells 0 .. L-1 carry the labels `ext`; CTC: blank, y1, blank, y2, ..., blank (L = 2S+1); ASG (no blanks):
y1 .. yS (L = S).  A walk starts in cell 0 or 1 (ASG: 0), ends in cell L-1 or L-2 (ASG: L-1) and moves by +0, +1, or
-- onto a non-blank label that differs from the one two cells back -- +2.
"""
import numpy as np


def extended(targets, is_ctc, blank):
    """The labels of the lattice's cells for one utterance's targets (already cut to t_len)."""
    tg = np.asarray(targets, dtype=np.int64).reshape(-1)
    if not is_ctc:
        return tg.copy()
    ext = np.full(2 * len(tg) + 1, blank, dtype=np.int64)
    ext[1::2] = tg
    return ext


def _skip_allowed(ext, is_ctc, blank):
    """(L) bool: cell i may be entered from cell i-2."""
    ok = np.zeros(len(ext), dtype=bool)
    if is_ctc and len(ext) > 2:
        ok[2:] = (ext[2:] != blank) & (ext[2:] != ext[:-2])
    return ok


def best_score(lp, ext, T, is_ctc, blank):
    """The largest f64 score of a walk over frames 0 .. T-1: the max-plus recurrence, one numpy step per frame."""
    lp = np.asarray(lp, dtype=np.float64)
    ext = np.asarray(ext, dtype=np.int64)
    L = len(ext)
    assert L >= 1 and 1 <= T <= lp.shape[0]
    skip = _skip_allowed(ext, is_ctc, blank)
    alpha = np.full(L, -np.inf)
    alpha[0] = lp[0, ext[0]]
    if is_ctc and L > 1:
        alpha[1] = lp[0, ext[1]]
    for t in range(1, T):
        best = alpha.copy()
        best[1:] = np.maximum(best[1:], alpha[:-1])
        if is_ctc and L > 2:
            best[2:] = np.maximum(best[2:], np.where(skip[2:], alpha[:-2], -np.inf))
        alpha = best + lp[t, ext]
    if is_ctc and L > 1:
        return max(alpha[L - 1], alpha[L - 2])
    return alpha[L - 1]


def path_cells(labels, ext, is_ctc, blank):
    """The cells of a legal walk that spells the frame labelling `labels`, or ValueError when there is none.  (A labelling
    does not name its cells -- blanks and repeated labels occur in several -- so the cells reachable under the labelling are
    carried frame by frame and one walk is read back from the end.)"""
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    ext = np.asarray(ext, dtype=np.int64)
    T, L = len(labels), len(ext)
    if T < 1 or L < 1:
        raise ValueError("nothing to walk: %d frames, %d cells" % (T, L))
    skip = _skip_allowed(ext, is_ctc, blank)
    reach = np.zeros((T, L), dtype=bool)
    reach[0, 0] = True
    if is_ctc and L > 1:
        reach[0, 1] = True
    reach[0] &= ext == labels[0]
    for t in range(1, T):
        r = reach[t - 1].copy()
        r[1:] |= reach[t - 1, :-1]
        r[2:] |= reach[t - 1, :-2] & skip[2:]
        reach[t] = r & (ext == labels[t])
        if not reach[t].any():
            raise ValueError("frame %d: label %d continues no walk" % (t, labels[t]))
    ends = [L - 1, L - 2] if (is_ctc and L > 1) else [L - 1]
    ends = [i for i in ends if reach[T - 1, i]]
    if not ends:
        raise ValueError("the labelling does not end in the lattice's last cells")
    cells = np.empty(T, dtype=np.int64)
    i = ends[0]
    for t in range(T - 1, 0, -1):
        cells[t] = i
        if reach[t - 1, i]:
            pass
        elif i >= 1 and reach[t - 1, i - 1]:
            i -= 1
        else:
            assert i >= 2 and skip[i] and reach[t - 1, i - 2]
            i -= 2
    cells[0] = i
    assert reach[0, i]
    return cells


def path_score(lp, labels):
    """The labelling's score, the emissions added in frame order."""
    lp = np.asarray(lp, dtype=np.float64)
    s = lp[0, labels[0]]
    for t in range(1, len(labels)):
        s = s + lp[t, labels[t]]
    return s


def feasible(targets, T, is_ctc):
    """Enough frames for the labelling (CTC: a blank between doubled labels)."""
    tg = np.asarray(targets, dtype=np.int64).reshape(-1)
    need = len(tg) + (int((tg[1:] == tg[:-1]).sum()) if is_ctc else 0)
    return T >= need


def check_utterance(lp, labels, targets, T, is_ctc, blank):
    """A feasible utterance of at least two frames and one label: `labels` is a legal walk and none scores higher."""
    ext = extended(targets, is_ctc, blank)
    labels = np.asarray(labels)[:T]
    cells = path_cells(labels, ext, is_ctc, blank)
    assert np.array_equal(ext[cells], labels)
    got, want = path_score(lp, labels), best_score(lp, ext, T, is_ctc, blank)
    assert got == want, ("the labelling is legal but not the best", got, want)


def quantised(rng, shape, step=1 / 8, lo=-8):
    """Emissions that are multiples of `step` in [lo, 0]: exact in f16, bf16, f32 and f64, and exact under f64 addition --
    every dtype must give one and the same labelling, and ties are everywhere."""
    n = int(round(-lo / step))
    return rng.integers(0, n + 1, size=shape).astype(np.float64) * step + lo
