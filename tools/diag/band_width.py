"""How many label pairs of the CTC lattice carry a 16-step segment's posterior mass (CPU, f64, log domain).

The banded segment kernel (end2end_amd/csrc/ctc_loss_fast.hip, segment_wave_band) walks 128 label pairs per segment instead of
the up to 256 of the whole lattice.  This tool measures, with the reference's recurrence in f64, how wide the band really is:

  measured   window [lowest pair whose posterior alpha*beta/Z exceeds the threshold at the segment's first step, highest at the
             step after its last], maximum over the segments of an utterance -- for thresholds 2^-40, 2^-50, 2^-60;
  rule       the window the kernel itself derives (the same arithmetic on f64 cells: kBandCut = -50 on the bound from the
             exponents of the checkpoint rows' four-pair groups and, where that window does not fit, kBandCutCells = -39 on
             the groups' weights cell by cell), in pairs, and how many segments would not fit 128.

    python3 tools/diag/band_width.py            # the table of DESIGN.md 4.1 (a few minutes)
    python3 tools/diag/band_width.py --quick    # one seed per shape, fewer utterances

numpy and the project's own oracle (tests/oracle_lib.py: the loss cross-checks the recurrence here) only; needs no GPU."""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
KSEG = 16           # steps per segment (kFastSeg)
BAND_CUT = -50      # kBandCut
BAND_CUT_CELLS = -39   # kBandCutCells
BAND_PAIRS = 128    # kBandPairs


def fast_tilt(S, T):
    rho = min(max(S / T, 1.0 / 33.0), 0.8)
    return 2.0 * rho / (1.0 - rho) if S > 0 else 1.0


def lattice(lp, tg, blank=0):
    """lp: (T, V) log-probabilities, tg: (S,) labels.  Returns (log alpha [T, L], log q [T, L], log Z): alpha with the emission
    of its step, q = beta * emission (what the chains checkpoint), L = 2S + 1."""
    lp = np.asarray(lp, dtype=np.float64)
    T = lp.shape[0]
    S = len(tg)
    L = 2 * S + 1
    ext = np.full(L, blank, dtype=np.int64)
    ext[1::2] = tg
    skip = np.zeros(L, dtype=bool)                  # j-2 -> j allowed
    skip[3::2] = ext[3::2] != ext[1:-2:2]
    ninf = -np.inf
    em = lp[:, ext]                                 # (T, L)
    la = np.full((T, L), ninf)
    la[0, 0] = em[0, 0]
    if L > 1:
        la[0, 1] = em[0, 1]
    with np.errstate(invalid="ignore"):
        for t in range(1, T):
            a = la[t - 1]
            a1 = np.concatenate(([ninf], a[:-1]))
            a2 = np.where(skip, np.concatenate(([ninf, ninf], a[:-2])), ninf)
            la[t] = np.logaddexp(np.logaddexp(a, a1), a2) + em[t]
        lq = np.full((T, L), ninf)
        lq[T - 1, L - 1] = em[T - 1, L - 1]
        if L > 1:
            lq[T - 1, L - 2] = em[T - 1, L - 2]
        skipn = np.concatenate((skip[2:], [False, False]))     # j -> j+2 allowed
        for t in range(T - 2, -1, -1):
            q = lq[t + 1]
            q1 = np.concatenate((q[1:], [ninf]))
            q2 = np.where(skipn, np.concatenate((q[2:], [ninf, ninf])), ninf)
            lq[t] = np.logaddexp(np.logaddexp(q, q1), q2) + em[t]
    lz = np.logaddexp(la[T - 1, L - 1], la[T - 1, L - 2]) if L > 1 else la[T - 1, 0]
    return la, lq, lz, em


def measured_width(la, lq, lz, em, log2_thr):
    """The widest window over the utterance's segments, in pairs."""
    T, L = la.shape
    with np.errstate(invalid="ignore"):
        post = (la + lq - em - lz) / math.log(2.0)          # log2 of alpha*beta/Z
    post = np.where(np.isnan(post), -np.inf, post)
    widest = 0
    for t0 in range(0, T, KSEG):
        t1 = min(t0 + KSEG, T - 1)
        lo = np.nonzero(post[t0] > log2_thr)[0]
        hi = np.nonzero(post[t1] > log2_thr)[0]
        if len(lo) and len(hi):
            widest = max(widest, int(hi[-1]) // 2 - int(lo[0]) // 2 + 1)
    return widest


def rule_windows(la, lq, lz, S, second_stage=True):
    """The kernel's own rule on f64 cells: per segment (lo, hi) in four-pair groups, and whether the window fits 128 pairs.
    First the bound from the group exponents; where that window does not fit, the groups' weights cell by cell (the kernel's
    second stage, band_group_matters)."""
    T, L = la.shape
    ln2 = math.log(2.0)
    r = fast_tilt(S, T)
    lr = math.log(r)
    j = np.arange(L)
    G = S // 4 + 1                                         # groups the chains store (4 g <= S)
    pad = 8 * G - L
    ninf = -np.inf

    def groups(row):
        return np.concatenate((row, np.full(pad, ninf))).reshape(G, 8)

    def group_exp(row):                                    # floor(log2(max of the group's cells)), -30000 for an empty group
        v = groups(row).max(axis=1) / ln2
        return np.where(np.isfinite(v), np.floor(v), -30000.0)

    def group_weight_exp(row):                             # the exponent e with (sum of the group's cells) < 2^e; -inf if empty
        v = groups(row)
        m = v.max(axis=1)
        ok = np.isfinite(m)
        with np.errstate(invalid="ignore", divide="ignore"):
            s = np.where(ok, np.where(ok, m, 0.0) + np.log(np.exp(v - np.where(ok, m, 0.0)[:, None]).sum(axis=1)), ninf)
        return np.where(ok, np.floor(s / ln2) + 1, ninf)

    def up(v, k):                                          # v[j + k], -inf past the end
        return np.concatenate((v[k:], np.full(k, ninf)))

    def down(v, k):                                        # v[j - k]
        return np.concatenate((np.full(k, ninf), v[:-k]))
    zint = math.floor((lz + (L - 1) * lr) / ln2)
    out = []
    for t0 in range(0, T, KSEG):
        sides = {}
        if t0 > 0:
            a, q = la[t0 - 1] + j * lr, lq[t0] + (L - 1 - j) * lr            # the tilted cells
            ea, eb = group_exp(a), group_exp(q)
            m = ea + np.maximum(eb, np.concatenate((eb[1:], [-30000.0]))) - zint
            with np.errstate(invalid="ignore"):
                w = group_weight_exp(a + np.logaddexp(np.logaddexp(q, up(q, 1) + lr), up(q, 2) + 2 * lr)) - zint
            sides["lo"] = (m, w)
        if t0 + KSEG < T:
            a, q = la[t0 + KSEG - 1] + j * lr, lq[t0 + KSEG] + (L - 1 - j) * lr
            ea, eb = group_exp(a), group_exp(q)
            m = eb + np.maximum(ea, np.concatenate(([-30000.0], ea[:-1]))) - zint
            with np.errstate(invalid="ignore"):
                w = group_weight_exp(np.logaddexp(np.logaddexp(a, down(a, 1) + lr), down(a, 2) + 2 * lr) + q) - zint
            sides["hi"] = (m, w)

        def window(second):
            lo, hi = 0, S // 4
            for side, (m, w) in sides.items():
                k = m > BAND_CUT
                if second:
                    k = k & ((m > 72) | (w > BAND_CUT_CELLS))
                k = np.nonzero(k)[0]
                if side == "lo":
                    lo = int(k[0]) if len(k) else 0
                else:
                    hi = int(k[-1]) if len(k) else lo
            return lo, hi, 4 * hi + 3 <= min(4 * lo, 256 - BAND_PAIRS) + BAND_PAIRS - 1
        win = window(False)
        if not win[2] and second_stage:
            win = window(True)
        out.append(win)
    return out


def utterance_numbers(lp, tg, blank=0, thresholds=(-40, -50, -60)):
    """{'measured': {thr: pairs}, 'rule_pairs': widest rule window in pairs, 'misses': segments that do not fit, 'loss': -log Z}"""
    la, lq, lz, em = lattice(lp, tg, blank)
    win = rule_windows(la, lq, lz, len(tg))
    return {"measured": {k: measured_width(la, lq, lz, em, k) for k in thresholds},
            "rule_pairs": max(4 * (hi - lo + 1) for lo, hi, _ in win), "misses": sum(1 for w in win if not w[2]), "loss": -lz}


def log_softmax(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max(axis=-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


def no_repeat_targets(rng, S, V):
    """S labels in [1, V) without equal neighbours."""
    tg = rng.integers(1, V, size=S)
    for i in range(1, S):
        while tg[i] == tg[i - 1]:
            tg[i] = rng.integers(1, V)
    return tg


def two_alignment_logits(tg, T, V, blank=0, peak=0.49):
    """Emissions that are an even mixture of two alignments of the same targets: one emits every label in the first half of the
    frames, the other in the last half.  At mid-utterance the posterior sits at both ends of the lattice: a window that no 128
    pairs hold (tests/test_gpu_banded_segments.py).  Returns (T, V) log-probabilities."""
    tg = np.asarray(tg)
    S = len(tg)
    assert S <= T // 2 and (tg[1:] != tg[:-1]).all(), "one label per frame: no equal neighbours, and the halves must hold S frames"
    paths = []
    for first in (True, False):
        path = np.full(T, blank)
        path[np.arange(S) + (0 if first else T - S)] = tg       # packed to the front / to the back, blanks elsewhere
        paths.append(path)
    y = np.full((T, V), (1.0 - 2 * peak) / V)
    for path in paths:
        y[np.arange(T), path] += peak
    return np.log(y / y.sum(axis=1, keepdims=True))


def _report(name, batches, check_oracle):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    rows = []
    for lp, tg, tl in batches:
        for b in range(lp.shape[0]):
            rows.append(utterance_numbers(lp[b], tg[b, :tl[b]]))
        if check_oracle:
            import oracle_lib as O
            B, T, _ = lp.shape
            want, _ = O.ctc_loss(lp, tg, np.full(B, T), tl, 0)
            got = np.array([r["loss"] for r in rows[-B:]])
            assert np.allclose(got, want, rtol=1e-9, atol=1e-9), (name, np.abs(got - want).max())
    cols = ["%d-%d" % (min(r["measured"][k] for r in rows), max(r["measured"][k] for r in rows)) for k in (-40, -50, -60)]
    print("%-44s %9s %9s %9s   rule %3d-%3d pairs, %d of %d utterances with a segment that does not fit"
          % (name, *cols, min(r["rule_pairs"] for r in rows), max(r["rule_pairs"] for r in rows),
             sum(1 for r in rows if r["misses"]), len(rows)))


def main(argv):
    quick = "--quick" in argv
    seeds = (0,) if quick else (0, 1, 2)
    n = 2 if quick else 4
    V = 29
    print("%-44s %9s %9s %9s" % ("emissions, shape (V=29, random targets)", "2^-40", "2^-50", "2^-60"))

    def noise(scale, T, S):
        out = []
        for s in seeds:
            rng = np.random.default_rng(s)
            out.append((log_softmax(rng.standard_normal((n, T, V)) * scale), rng.integers(1, V, size=(n, S)), np.full(n, S)))
        return out
    _report("randn, T=1000 S=200", noise(1.0, 1000, 200), True)
    _report("flat (randn x 0.1), T=1000 S=200", noise(0.1, 1000, 200), False)
    _report("flat, T=600 S=223", noise(0.1, 600, 223), False)
    if not quick:
        _report("flat, T=3000 S=223", noise(0.1, 3000, 223), False)
        _report("randn, T=2000 S=223", noise(1.0, 2000, 223), False)
    _report("flat, T=450 S=200", noise(0.1, 450, 200), False)
    # a blank that dominates (an untrained model): the steepest rows, where the group maxima overestimate most
    def blank_biased(bias, scale, T, S):
        out = []
        for lp, tg, tl in noise(scale, T, S):
            x = lp.copy()
            x[:, :, 0] += bias
            out.append((log_softmax(x), tg, tl))
        return out
    for bias, scale, T, S in ((2, 0.1, 1000, 200), (4, 0.1, 1000, 200), (6, 0.1, 1000, 200), (6, 1.0, 1000, 200), (8, 1.0, 1000, 223),
                              (6, 0.1, 1000, 170)) + (() if quick else ((5, 0.1, 2000, 223), (8, 0.1, 3000, 223))):
        _report("blank + %g, randn x %g, T=%d S=%d" % (bias, scale, T, S), blank_biased(bias, scale, T, S), False)
    _report("randn x 3, T=1000 S=200 (fallback_regime)", noise(3.0, 1000, 200), False)
    _report("randn x 8, T=1000 S=200 (sharp_unrelated)", noise(8.0, 1000, 200), False)
    # bench.py's regime generators
    sys.path.insert(0, ROOT)
    import bench
    for boost in (6.0, 10.0, 14.0):
        x, tg, _, tl = bench.aligned_batch(int(boost), n, 1000, V, 200, boost)
        _report("aligned_batch boost %g (trained_regime)" % boost, [(log_softmax(x.numpy()), tg.numpy(), tl.numpy())], False)
    tg = no_repeat_targets(np.random.default_rng(5), 223, V)
    r = utterance_numbers(two_alignment_logits(tg, 480, V), tg)
    print("two-alignment mixture, T=480 S=223: measured %s pairs, rule %d pairs, %d segments do not fit"
          % (r["measured"], r["rule_pairs"], r["misses"]))


if __name__ == "__main__":
    main(sys.argv[1:])
