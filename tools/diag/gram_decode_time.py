"""Time the Gram-CTC beam search (e2e_gram_ctc_beam_nbest through GramCTCDecoderEngine, f32 log-probabilities) with HIP
events on seeded inputs, 20 calls after warm-up: B=64, T=1000 at the loss's headline table (R=29: 28 unigrams, 300
bigrams, 50 trigrams, V=379) at widths 16 and 100; the same batch with unigrams only (V=29) at width 100, beside
e2e_ctc_beam_nbest on that input in the same process; and B=64, T=256, V=8000 (orders 2-4) at width 16.  Greedy decoding of
the headline batch is timed too.

    python tools/diag/gram_decode_time.py [--iters N] [--out FILE]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

from end2end_amd.engines import CTCDecoderEngine, GramCTCDecoderEngine
from gram_time import table

DEV = torch.device("cuda", 0)


def batch(B, T, V, seed):
    g = torch.Generator().manual_seed(seed)
    lp = torch.log_softmax(torch.randn(B, T, V, generator=g), -1)
    xl = torch.randint(T // 2, T + 1, (B,), generator=g)
    xl[0] = T
    return lp.to(DEV), xl.to(DEV)


def time_call(fn, iters, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    rng = np.random.default_rng(7)
    R = 29
    l2i, V = table(rng, R, {2: 300, 3: 50})
    lp, xl = batch(64, 1000, V, 7)
    frames = int(xl.sum())
    for w in (16, 100):
        eng = GramCTCDecoderEngine(0, R, V, l2i, w, keep_on_device=True)
        ms = time_call(lambda: eng.decode_nbest(lp, xl, nbest=1), a.iters)
        say("gram beam  B=64 T=1000 V=%d (300 bigrams, 50 trigrams) width %d: %.2f ms per call, %.1f us per frame of the longest "
            "utterance (%d frames in the batch)" % (V, w, ms, ms * 1e3 / 1000, frames))
    eng = GramCTCDecoderEngine(0, R, V, l2i, 1, keep_on_device=True)
    say("gram greedy B=64 T=1000 V=%d: %.3f ms per call" % (V, time_call(lambda: eng.decode_greedy(lp, xl), a.iters)))
    lp, xl = batch(64, 1000, R, 7)
    eng = GramCTCDecoderEngine(0, R, R, {}, 100, keep_on_device=True)
    say("gram beam  B=64 T=1000 V=29 unigrams only width 100: %.2f ms per call"
        % time_call(lambda: eng.decode_nbest(lp, xl, nbest=1), a.iters))
    ctc = CTCDecoderEngine(0, 100, keep_on_device=True)
    say("ctc beam   B=64 T=1000 V=29 width 100 (e2e_ctc_beam_nbest, same input): %.2f ms per call"
        % time_call(lambda: ctc.decode_nbest(lp, xl, nbest=1), a.iters))
    l2i, V = table(rng, R, {2: 700, 3: 4000, 4: 3271})
    lp, xl = batch(64, 256, V, 8)
    eng = GramCTCDecoderEngine(0, R, V, l2i, 16, keep_on_device=True)
    say("gram beam  B=64 T=256 V=%d (orders 2-4) width 16: %.2f ms per call"
        % (V, time_call(lambda: eng.decode_nbest(lp, xl, nbest=1), a.iters)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
