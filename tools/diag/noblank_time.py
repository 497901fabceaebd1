"""Time CTC without blank (e2e_ctc_noblank_fwd_bwd through CTCWithoutBlankLossEngine, f32, fused log-softmax) with HIP
events: B=256, T=1000, V=29, S<=200 ragged (the headline shape, with and without spaces), and B=64, T=256, V=8000.

    python tools/diag/noblank_time.py [--iters N]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

from end2end_amd.engines import CTCWithoutBlankLossEngine


def shape(B, T, V, S, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, V, generator=g)
    tg = torch.randint(0, V - 1, (B, S), generator=g)
    tl = torch.randint(S // 2, S + 1, (B,), generator=g)
    xl = torch.maximum(torch.randint(T // 2, T + 1, (B,), generator=g), tl)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    for (B, T, V, S), sp in [((256, 1000, 29, 200), -1), ((256, 1000, 29, 200), 28), ((64, 256, 8000, 60), 3)]:
        ms = time_call(CTCWithoutBlankLossEngine(sp), shape(B, T, V, S, 7), a.iters)
        print("noblank B=%d T=%d V=%d S<=%d space_idx=%d: %.3f ms per call" % (B, T, V, S, sp, ms))


if __name__ == "__main__":
    main()
