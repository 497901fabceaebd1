"""Test-side restatement of ASG (the definition of include/e2e_ctc.h) in f64 numpy: a plain log-domain loop per utterance
with alpha-beta gradients, the best path in the order the header states, and a brute-force enumerator for tiny shapes
(all V^n paths, all alignments k).  Upstream has no ASG to compare with.

    x (B,T,V) emissions, A (V,V) transitions, A[j,i] = score of j after i
    score(pi) = sum_t x[t,pi_t] + sum_{t>=1} A[pi_t, pi_{t-1}]
    loss = FCC - FAL
"""
import itertools

import numpy as np


def _lse(a, axis=None):
    m = np.max(a, axis=axis, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        r = np.log(np.sum(np.exp(a - m), axis=axis, keepdims=True)) + m
    return float(r.reshape(-1)[0]) if axis is None else np.squeeze(r, axis=axis)


def fcc_one(x, A):
    """x (n,V), A (V,V) -> (FCC, P[t,v], G[j,i] = sum_t P(pi_t=j, pi_{t-1}=i))."""
    n, V = x.shape
    al = np.zeros((n, V))
    be = np.zeros((n, V))
    al[0] = x[0]
    for t in range(1, n):
        al[t] = x[t] + _lse(al[t - 1][None, :] + A, axis=1)
    for t in range(n - 2, -1, -1):
        be[t] = _lse((x[t + 1] + be[t + 1])[:, None] + A, axis=0)
    z = float(_lse(al[n - 1]))
    P = np.exp(al + be - z)
    G = np.zeros((V, V))
    for t in range(1, n):
        G += np.exp(al[t - 1][None, :] + A + (x[t] + be[t])[:, None] - z)
    return z, P, G


def fal_one(x, A, y):
    """x (n,V), A (V,V), y (s,) with s <= n -> (FAL, P[t,v], G[j,i]) over the alignments k."""
    n, V = x.shape
    s = len(y)
    ninf = -np.inf
    stay = A[y, y]
    adv = np.concatenate([[ninf], A[y[1:], y[:-1]]])            # adv[k] = A[y_k, y_{k-1}]
    al = np.full((n, s), ninf)
    be = np.full((n, s), ninf)
    al[0, 0] = x[0, y[0]]
    for t in range(1, n):
        prev = al[t - 1]
        shifted = np.concatenate([[ninf], prev[:-1]])
        al[t] = np.logaddexp(prev + stay, shifted + adv) + x[t, y]
    be[n - 1, s - 1] = 0.0
    for t in range(n - 2, -1, -1):
        h = x[t + 1, y] + be[t + 1]
        up = np.concatenate([(h + adv)[1:], [ninf]])
        be[t] = np.logaddexp(h + stay, up)
    z = al[n - 1, s - 1]
    P = np.zeros((n, V))
    G = np.zeros((V, V))
    with np.errstate(invalid="ignore"):
        post = np.exp(al + be - z)
    for k in range(s):                                          # cells in increasing k, as the definition counts them
        P[:, y[k]] += post[:, k]
    for t in range(1, n):
        h = x[t, y] + be[t]
        st = np.exp(al[t - 1] + stay + h - z)
        ad = np.exp(np.concatenate([[ninf], al[t - 1][:-1]]) + adv + h - z)
        np.add.at(G, (y, y), st)                                # (unbuffered: cells of one label pair add up)
        np.add.at(G, (y[1:], y[:-1]), ad[1:])
    return float(z), P, G


def asg_ref(x, A, targets, x_len, t_len):
    """-> (losses (B), grads (B,T,V), tgrads (B,V,V)) in f64, with the header's edge cases: an infeasible utterance
    (x_len < t_len) gets +inf, NaN rows t < x_len and a NaN slab; bad lengths or labels get NaN everywhere."""
    x = np.asarray(x, dtype=np.float64)
    A = np.asarray(A, dtype=np.float64)
    targets = np.asarray(targets)
    B, T, V = x.shape
    Smax = targets.shape[1]
    losses = np.zeros(B)
    grads = np.zeros((B, T, V))
    tgrads = np.zeros((B, V, V))
    for b in range(B):
        n, s = int(x_len[b]), int(t_len[b])
        bad = not (1 <= n <= T and 1 <= s <= Smax)
        if not bad:
            y = targets[b, :s].astype(np.int64)
            bad = bool(((y < 0) | (y >= V)).any())
        if bad:
            losses[b], grads[b], tgrads[b] = np.nan, np.nan, np.nan
            continue
        if n < s:
            losses[b] = np.inf
            grads[b, :n] = np.nan
            tgrads[b] = np.nan
            continue
        zc, Pc, Gc = fcc_one(x[b, :n], A)
        za, Pa, Ga = fal_one(x[b, :n], A, y)
        losses[b] = zc - za
        grads[b, :n] = Pc - Pa
        tgrads[b] = Gc - Ga
    return losses, grads, tgrads


def viterbi_one(x, A):
    """x (n,V) f64, A (V,V) f64 -> (path [n], score): delta_t[j] = (max_i (delta_{t-1}[i] + A[j,i])) + x[t,j], ties to the
    lowest i, the end state the lowest j of the largest delta."""
    n, V = x.shape
    d = x[0].copy()
    bp = np.zeros((n, V), dtype=np.int64)
    for t in range(1, n):
        cand = d[None, :] + A                                   # [j, i]
        bp[t] = np.argmax(cand, axis=1)                         # (first maximum)
        d = cand[np.arange(V), bp[t]] + x[t]
    j = int(np.argmax(d))
    score = float(d[j])
    path = [j]
    for t in range(n - 1, 0, -1):
        j = int(bp[t, j])
        path.append(j)
    return path[::-1], score


def viterbi_ref(x, A, x_len, pad=-100):
    """-> (paths (B,T) int64 padded, scores (B) f64, collapsed (B,T) zero padded, lengths (B))."""
    x = np.asarray(x, dtype=np.float64)
    A = np.asarray(A, dtype=np.float64)
    B, T, V = x.shape
    paths = np.full((B, T), pad, dtype=np.int64)
    coll = np.zeros((B, T), dtype=np.int64)
    scores = np.full(B, np.nan)
    lengths = np.zeros(B, dtype=np.int64)
    for b in range(B):
        n = int(x_len[b])
        if not 1 <= n <= T:
            continue
        p, scores[b] = viterbi_one(x[b, :n], A)
        paths[b, :n] = p
        merged = [c for i, c in enumerate(p) if i == 0 or c != p[i - 1]]
        coll[b, :len(merged)] = merged
        lengths[b] = len(merged)
    return paths, scores, coll, lengths


# ---- brute force: every path, every alignment ----

def path_score(x, A, pi):
    return sum(x[t, pi[t]] for t in range(len(pi))) + sum(A[pi[t], pi[t - 1]] for t in range(1, len(pi)))


def alignments(n, s):
    """Every k with k(0) = 0, k(n-1) = s-1, steps in {0, 1}."""
    for steps in itertools.product((0, 1), repeat=n - 1):
        if sum(steps) == s - 1:
            k = [0]
            for d in steps:
                k.append(k[-1] + d)
            yield k


def brute_loss(x, A, y):
    """x (n,V), A (V,V), y (s,) -> FCC - FAL by enumeration."""
    x = np.asarray(x, dtype=np.float64)
    A = np.asarray(A, dtype=np.float64)
    n, V = x.shape
    fcc = _lse(np.array([path_score(x, A, pi) for pi in itertools.product(range(V), repeat=n)]))
    fal = _lse(np.array([path_score(x, A, [y[c] for c in k]) for k in alignments(n, len(y))]))
    return float(fcc) - float(fal)
