"""Time Gram-CTC (e2e_gram_ctc_fwd_bwd through GramCTCLossEngine, f32, fused log-softmax) with HIP events on seeded
inputs: the headline gram shape (B=256, T=1000, R=29: 28 unigrams, 300 bigrams, 50 trigrams, V=379, S<=200 ragged), the
same batch with unigrams only (V=29; compare CTCLoss and CTC without blank on it), and a wide table (B=64, T=256, R=29,
V=8000, grams up to order 4).

    python tools/diag/gram_time.py [--iters N]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

from end2end_amd.engines import CTCLossEngine, GramCTCLossEngine


def table(rng, R, counts):
    """{column: base ids} with counts[k] distinct grams of order k (k >= 2), columns from R up."""
    l2i, seen, c = {}, set(), R
    for k in sorted(counts):
        n = 0
        while n < counts[k]:
            s = tuple(int(v) for v in rng.integers(1, R, size=k))
            if s not in seen:
                seen.add(s)
                l2i[c] = list(s)
                c += 1
                n += 1
    return l2i, c


def shape(B, T, V, R, S, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, V, generator=g)
    tg = torch.randint(1, R, (B, S), generator=g)
    tl = torch.randint(S // 2, S + 1, (B,), generator=g)
    xl = torch.maximum(torch.randint(T // 2, T + 1, (B,), generator=g), 2 * tl + 1)
    xl[0] = T
    d = torch.device("cuda", 0)
    return x.to(d), tg.to(d), xl.to(d), tl.to(d)


def time_call(eng, args, iters):
    for _ in range(3):
        eng.compute(*args, input_is_logprobs=False)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        eng.compute(*args, input_is_logprobs=False)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def redone(eng):
    f = eng.redo_flags()
    return "utterances redone in the log domain: %d after the forward, %d after the backward, of %d" % (
        int((f == 1).sum()), int((f == 2).sum()), len(f))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    rng = np.random.default_rng(7)
    R = 29
    l2i, V = table(rng, R, {2: 300, 3: 50})
    args = shape(256, 1000, V, R, 200, 7)
    eng = GramCTCLossEngine(0, R, V, l2i)
    ms = time_call(eng, args, a.iters)
    print("gram  B=256 T=1000 R=29 V=%d (300 bigrams, 50 trigrams) S<=200: %.3f ms per call; %s"
          % (V, ms, redone(eng)))
    args = shape(256, 1000, R, R, 200, 7)
    eng = GramCTCLossEngine(0, R, R, {})
    ms = time_call(eng, args, a.iters)
    print("gram  B=256 T=1000 V=29 unigrams only S<=200: %.3f ms per call; %s" % (ms, redone(eng)))
    print("ctc   B=256 T=1000 V=29 S<=200 (CTCLoss engine, same batch): %.3f ms per call"
          % time_call(CTCLossEngine(0), args, a.iters))
    l2i, V = table(rng, R, {2: 700, 3: 4000, 4: 3271})
    args = shape(64, 256, V, R, 60, 8)
    eng = GramCTCLossEngine(0, R, V, l2i)
    ms = time_call(eng, args, a.iters)
    print("gram  B=64 T=256 R=29 V=%d (orders 2-4) S<=60: %.3f ms per call; %s" % (V, ms, redone(eng)))


if __name__ == "__main__":
    main()
