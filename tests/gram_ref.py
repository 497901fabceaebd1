"""Test-side restatement of Gram-CTC (the definition of include/e2e_ctc.h; upstream's engine is empty, so there is no
reference to make fixtures from).  Two independent forms:
  * brute_force: every one of the V**T paths, labelled from the definition (collapse runs of a column, drop blanks,
    concatenate the grams' base sequences); the loss and the per-(t, column) posteriors straight from the sum;
  * lattice: the f64 log-domain forward-backward over the boundary lattice the kernel runs, vectorised over the states.
Only tests import it."""
import itertools

import numpy as np

NINF = -np.inf


def grams_of(num_base_labels, total_labels, label2ids):
    """{column: base-id tuple} for the columns 1 .. V-1."""
    g = {c: (c,) for c in range(1, num_base_labels)}
    for c, ids in label2ids.items():
        g[int(c)] = tuple(int(i) for i in ids)
    assert sorted(g) == list(range(1, total_labels))
    return g


def labelling(path, grams):
    out, prev = [], None
    for c in path:
        if c != prev and c != 0:
            out.extend(grams[c])
        prev = c
    return tuple(out)


def brute_force(lp, target, grams):
    """lp (T, V) f64 -> (loss, posterior (T, V)); loss +inf when no path spells the target."""
    T, V = lp.shape
    target = tuple(int(v) for v in target)
    total = NINF
    post = np.full((T, V), NINF)
    for path in itertools.product(range(V), repeat=T):
        if labelling(path, grams) != target:
            continue
        s = float(sum(lp[t, c] for t, c in enumerate(path)))
        total = np.logaddexp(total, s)
        for t, c in enumerate(path):
            post[t, c] = np.logaddexp(post[t, c], s)
    if total == NINF:
        return np.inf, np.full((T, V), np.nan)
    return -total, np.exp(post - total)


def _lse_rows(a):
    m = np.max(a, axis=1)
    mf = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return np.where(np.isfinite(m), mf + np.log(np.sum(np.exp(a - mf[:, None]), axis=1)), m)


def states(target, grams):
    """The lattice: [(j, k, column)] with k = 0 the blank of boundary j, and the predecessor lists."""
    S = len(target)
    key = {v: c for c, v in grams.items()}
    order = max(len(v) for v in grams.values()) if grams else 1
    st, idx = [], {}
    for j in range(S + 1):
        idx[(j, 0)] = len(st)
        st.append((j, 0, 0))
        for k in range(1, order + 1):
            if j >= k and tuple(target[j - k:j]) in key:
                idx[(j, k)] = len(st)
                st.append((j, k, key[tuple(target[j - k:j])]))
    ending = {j: [idx[(j, k)] for k in range(1, order + 1) if (j, k) in idx] for j in range(S + 1)}
    preds = []
    for s, (j, k, c) in enumerate(st):
        if k == 0:
            preds.append([s] + ending[j])
        else:
            preds.append([s, idx[(j - k, 0)]] + [g for g in ending[j - k] if st[g][2] != c])
    return st, preds, idx


def lattice(lp, target, grams):
    """lp (T, V) f64 -> (loss, posterior (T, V)) by the log-domain forward-backward."""
    T, V = lp.shape
    target = [int(v) for v in target]
    S = len(target)
    st, preds, idx = states(target, grams)
    N = len(st)
    P = max(len(p) for p in preds)
    pred = np.full((N, P), N)
    for s, p in enumerate(preds):
        pred[s, :len(p)] = p
    succ_lists = [[] for _ in range(N)]
    for s, p in enumerate(preds):
        for q in p:
            succ_lists[q].append(s)
    Q = max(len(p) for p in succ_lists)
    succ = np.full((N, Q), N)
    for s, p in enumerate(succ_lists):
        succ[s, :len(p)] = p
    cols = np.array([c for _, _, c in st])
    e = lp[:, cols]                                              # (T, N)
    start = np.full(N, NINF)
    for (j, k), s in idx.items():
        if (k == 0 and j == 0) or (k > 0 and j == k):
            start[s] = 0.0
    end = np.array([0.0 if j == S else NINF for j, _, _ in st])
    alpha = np.full((T, N), NINF)
    alpha[0] = start + e[0]
    for t in range(1, T):
        prev = np.append(alpha[t - 1], NINF)
        alpha[t] = _lse_rows(prev[pred]) + e[t]
    beta = np.full((T, N), NINF)
    beta[T - 1] = end
    for t in range(T - 2, -1, -1):
        g = np.append(beta[t + 1] + e[t + 1], NINF)
        beta[t] = _lse_rows(g[succ])
    logz = _lse_rows((alpha[T - 1] + end)[None, :])[0]
    if logz == NINF:
        return np.inf, np.full((T, V), np.nan)
    ab = alpha + beta
    post = np.full((T, V), NINF)
    for c in np.unique(cols):
        post[:, c] = _lse_rows(ab[:, cols == c])
    return -logz, np.exp(post - logz)


def loss_grad(lp, targets, x_len, t_len, grams, method=lattice):
    """Batch driver: lp (B, T, V) f64 log-probabilities -> (losses (B,), grads (B, T, V)) with grads = exp(lp) - posterior
    on rows t < x_len (NaN there for an infeasible utterance), 0 beyond."""
    lp = np.asarray(lp, dtype=np.float64)
    B, T, V = lp.shape
    losses = np.zeros(B)
    grads = np.zeros_like(lp)
    for b in range(B):
        n, s = int(x_len[b]), int(t_len[b])
        losses[b], post = method(lp[b, :n], targets[b][:s], grams)
        with np.errstate(invalid="ignore"):
            grads[b, :n] = np.exp(lp[b, :n]) - post
    return losses, grads


def random_tiny_case(rng):
    """A tiny random table and utterance for brute force: at most 5 columns and V**T <= 4096 paths, grams of order 2
    and 3, targets rich in repeats ("aaa" with the gram "aa", "abab" with "ab")."""
    R = int(rng.integers(2, 4))                                  # blank + 1 or 2 base labels
    n_grams = int(rng.integers(0, min(5 - R, 2 if R == 2 else 3) + 1))   # (R = 2: only 'aa' and 'aaa' exist)
    V = R + n_grams
    seqs = set()
    while len(seqs) < n_grams:
        k = int(rng.integers(2, 4))
        seqs.add(tuple(int(v) for v in rng.integers(1, R, size=k)))
    label2ids = {R + i: list(s) for i, s in enumerate(sorted(seqs))}
    T = int(rng.integers(1, 7))
    while V ** T > 4096:
        T -= 1
    S = int(rng.integers(0, T + 2))
    if label2ids and rng.random() < 0.6:                         # spell the target out of grams, repeats included
        tgt = []
        while len(tgt) < S:
            tgt += list(label2ids[int(rng.choice(list(label2ids)))]) if rng.random() < 0.7 else [int(rng.integers(1, R))]
        tgt = tgt[:S]
    else:
        tgt = [int(v) for v in rng.integers(1, R, size=S)]
    x = rng.normal(size=(T, V)) * float(rng.choice([0.5, 1.0, 3.0]))
    return R, V, label2ids, x, tgt
