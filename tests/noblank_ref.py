"""Test-side restatement of CTC without blank (pytorch_end2end/functions/ctc_without_blank.py:13-138 upstream): the f64
log-domain lattice, vectorised over the cells of a frame with numpy, for shapes the pure-Python reference is too slow
for.  Same arithmetic as upstream: log_sum_exp(a, b) = max + log(1 + exp(min - max)), alpha from (j, j-1), beta from
(j, j+1), per-label sums in increasing j.  Only tests import it."""
import numpy as np

NINF = -np.inf


def lse2(a, b):
    """Upstream's log_sum_exp (functions/utils.py), elementwise."""
    a, b = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
    hi, lo = np.maximum(a, b), np.minimum(a, b)
    with np.errstate(invalid="ignore", over="ignore"):
        out = hi + np.log(1.0 + np.exp(lo - hi))
    out = np.where(a == NINF, b, np.where(b == NINF, a, out))
    return out


def extended_target(target, space_idx):
    target = [int(v) for v in target]
    if len(target) == 0 or (len(target) == 1 and target[0] == space_idx):
        return [space_idx], False
    if space_idx == -1:
        return target, False
    return [space_idx] + target + [space_idx], True


def utterance(lp, target, space_idx):
    """lp (T, V) f64 log-probabilities of one utterance -> (loss, grad (T, V)) as upstream's _ctc_without_blank_loss."""
    T, V = lp.shape
    ext, two = extended_target(target, space_idx)
    ext = np.asarray(ext, dtype=np.int64)
    L = len(ext)
    e = lp[:, ext]                                         # (T, L); label -1 reads column V-1 (Q10)
    alpha = np.full((T, L), NINF)
    alpha[0, 0] = e[0, 0]
    if two:
        alpha[0, 1] = e[0, 1]
    for t in range(1, T):
        prev = alpha[t - 1]
        shifted = np.concatenate(([NINF], prev[:-1]))
        alpha[t] = lse2(prev, shifted) + e[t]
    logz = lse2(alpha[T - 1, L - 1], alpha[T - 1, L - 2]) if two else alpha[T - 1, L - 1]
    beta = np.full((T, L), NINF)
    beta[T - 1, L - 1] = 0.0
    if two:
        beta[T - 1, L - 2] = 0.0
    for t in range(T - 2, -1, -1):
        g = beta[t + 1] + e[t + 1]
        beta[t] = lse2(g, np.concatenate((g[1:], [NINF])))
    ab = alpha + beta
    prob_sum = np.full((T, V), NINF)
    for i in range(L):
        prob_sum[:, ext[i]] = lse2(prob_sum[:, ext[i]], ab[:, i])
    with np.errstate(invalid="ignore", over="ignore"):
        grad = np.exp(lp) - np.exp(prob_sum - logz)
    return -float(logz), grad


def noblank_loss_grad(lp, targets, x_len, t_len, space_idx=-1):
    """Batch driver: lp (B, T, V) f64 -> (losses (B,), grads (B, T, V)); rows t >= x_len are 0."""
    lp = np.asarray(lp, dtype=np.float64)
    B, T, V = lp.shape
    losses = np.zeros(B)
    grads = np.zeros_like(lp)
    for b in range(B):
        n, s = int(x_len[b]), int(t_len[b])
        losses[b], grads[b, :n] = utterance(lp[b, :n], targets[b][:s], space_idx)
    return losses, grads
