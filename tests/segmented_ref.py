"""Plain-Python restatement of word-segmented CTC (the Definition in include/e2e_ctc.h): boundaries,
segments, and losses as the sum of oracle_lib.ctc_loss in f64 over the segments' log-softmaxed frames.  TEST
INFRASTRUCTURE ONLY: the checker of tests/test_segmented_cpu.py and tests/test_gpu_segmented.py.
"""
import itertools

import numpy as np

import oracle_lib as O

WHOLE, FRAME, CHUNK = 0, 1, 2


def log_softmax(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max(axis=-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


def argmax_first(x):
    """First maximum per row; NaN counts as the maximum (np.argmax does both)."""
    return np.argmax(np.asarray(x), axis=-1)


def boundaries(a, p, n, space, blank, min_word_length):
    bounds, start_space, clean, wl, last, last_blank = [0], -1, True, 0, -1, False
    for t in range(n):
        if a[t] != p[t]:
            clean = False
            continue
        if a[t] == space:
            if clean and wl >= min_word_length:
                if start_space != -1 and bounds[-1] != start_space:
                    bounds.append(start_space)
                if t > 0:
                    bounds.append(t)
            start_space, clean, wl, last, last_blank = t, True, 0, -1, False
        elif a[t] == blank:
            last_blank = True
        else:
            if last_blank or a[t] != last:
                wl += 1
            last, last_blank = a[t], False
    if bounds[-1] != n - 1:
        bounds.append(n - 1)
    return bounds


def utterance_valid(targets_row, n, tl, T, V, Smax):
    return 1 <= n <= T and 0 <= tl <= Smax and all(0 <= int(c) < V for c in targets_row[:tl])


def segments(align, argmax, targets, x_len, t_len, V, space, blank, min_word_length):
    """-> list of (utterance, start, length, kind, target list), utterance-major, in the Definition's order."""
    B, T = np.asarray(align).shape
    targets = np.asarray(targets).reshape(B, -1)
    Smax = targets.shape[1]
    out = []
    for b in range(B):
        n, tl = int(x_len[b]), int(t_len[b])
        if not utterance_valid(targets[b], n, tl, T, V, Smax):
            out.append((b, 0, n if 1 <= n <= T else 1, WHOLE, []))
            continue
        a = [int(v) for v in align[b, :n]]
        bounds = boundaries(a, [int(v) for v in argmax[b, :n]], n, space, blank, min_word_length)
        if len(bounds) <= 2:
            out.append((b, 0, n, WHOLE, [int(c) for c in targets[b, :tl]]))
            continue
        for k, start in enumerate(bounds[:-1]):
            if start != 0:
                out.append((b, start, 1, FRAME, [a[start]]))
                start += 1
            end = bounds[k + 1] - (0 if k == len(bounds) - 2 else 1)
            if end >= start:
                tg = [c for c, _ in itertools.groupby(a[start:end + 1]) if c != blank]
                out.append((b, start, end - start + 1, CHUNK, tg))
    return out


def plan(logits, align, targets, x_len, t_len, space, blank=0, min_word_length=3):
    """Segments of a batch from its raw logits and its alignment."""
    logits = np.asarray(logits)
    return segments(align, argmax_first(logits), targets, x_len, t_len, logits.shape[2], space, blank, min_word_length)


def alignment(logp, targets, x_len, t_len, blank=0):
    """The Viterbi alignment of log-probabilities, by the oracle (f64)."""
    return O.ctc_align(np.asarray(logp, dtype=np.float64), targets, x_len, t_len, blank=blank, is_ctc=True)


def losses_and_grads(logits, segs, blank=0, logp=None):
    """(losses (B,) f64, gradient (B,T,V) f64) of the segments `segs` of `logits`: each segment's CTC loss on its own
    log-softmaxed frames, summed per utterance in order; softmax - posterior on the segment's frames, 0 elsewhere.  `logp`:
    the log-softmax to use instead of the f64 one of `logits` (upstream takes it in f32).  Whole segments of invalid
    utterances (empty target list and bad lengths) are the caller's business: skip them before."""
    logits = np.asarray(logits, dtype=np.float64)
    B, T, V = logits.shape
    lp = log_softmax(logits) if logp is None else np.asarray(logp, dtype=np.float64)
    loss = np.zeros(B)
    grad = np.zeros((B, T, V))
    for (b, s, n, kind, tg) in segs:
        piece = np.ascontiguousarray(lp[b:b + 1, s:s + n])
        tgt = np.asarray(tg if tg else [0], dtype=np.int64).reshape(1, -1)
        l, g = O.ctc_loss(piece, tgt, np.array([n]), np.array([len(tg)]), blank, n_threads=1)
        loss[b] += l[0]
        grad[b, s:s + n] = g[0]
    return loss, grad
