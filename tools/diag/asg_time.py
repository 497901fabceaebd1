"""Time ASG (e2e_asg_fwd_bwd through ASGLossEngine, f32: loss and both gradients) with HIP events at B=256, T=1000, V=29,
S<=200 and at B=64, T=256, V=128, S<=60, ragged; CTCWithoutBlankLossEngine on the same inputs after log-softmax is timed in
the same process, the two alternating round by round, as the yardstick.  Also the best path (e2e_asg_viterbi) at the first
shape.  Medians over the rounds; the records go to profiles/asg/.

    python tools/diag/asg_time.py [--iters N] [--rounds R] [--out profiles/asg] [--profile]

--profile: a few calls of each and no records, for `rocprofv3 --kernel-trace --stats -- python tools/diag/asg_time.py --profile`.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch

from end2end_amd.engines import ASGLossEngine, ASGViterbiEngine, CTCWithoutBlankLossEngine

SHAPES = [(256, 1000, 29, 200), (64, 256, 128, 60)]


def shape(B, T, V, S, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, V, generator=g)
    A = torch.randn(V, V, generator=g)
    tg = torch.randint(0, V, (B, S), generator=g)
    tl = torch.randint(S // 2, S + 1, (B,), generator=g)
    xl = torch.maximum(torch.randint(T // 2, T + 1, (B,), generator=g), tl)
    xl[0] = T
    d = torch.device("cuda", 0)
    return x.to(d), A.to(d), tg.to(d), xl.to(d), tl.to(d)


def timed(fn, iters):
    for _ in range(3):
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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "asg"))
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    if a.profile:
        a.iters, a.rounds = 3, 1
    asg, vit, nb = ASGLossEngine(), ASGViterbiEngine(keep_on_device=True), CTCWithoutBlankLossEngine(-1)
    records, lines = [], []
    for n, (B, T, V, S) in enumerate(SHAPES):
        x, A, tg, xl, tl = shape(B, T, V, S, 7)
        lp = torch.log_softmax(x, -1)
        calls = {"asg_fwd_bwd_ms": lambda: asg.compute(x, A, tg, xl, tl),
                 "noblank_fwd_bwd_ms": lambda: nb.compute(lp, tg, xl, tl)}
        if n == 0:
            calls["asg_viterbi_ms"] = lambda: vit.compute(x, A, xl)
        ms = {k: [] for k in calls}
        for _ in range(a.rounds):                      # alternated: a round of each, then the next round
            for k, fn in calls.items():
                ms[k].append(timed(fn, a.iters))
        rec = {"B": B, "T": T, "V": V, "Smax": S, "dtype": "f32", "iters": a.iters, "rounds": a.rounds,
               "device": torch.cuda.get_device_name(0)}
        for k, v in ms.items():
            rec[k] = statistics.median(v)
            rec[k.replace("_ms", "_min_ms")] = min(v)
        rec["asg_over_noblank"] = rec["asg_fwd_bwd_ms"] / rec["noblank_fwd_bwd_ms"]
        records.append(rec)
        line = "B=%d T=%d V=%d S<=%d f32: ASG fwd+bwd %.3f ms, CTC without blank %.3f ms (x%.2f)" % (
            B, T, V, S, rec["asg_fwd_bwd_ms"], rec["noblank_fwd_bwd_ms"], rec["asg_over_noblank"])
        if n == 0:
            line += ", best path %.3f ms" % rec["asg_viterbi_ms"]
        lines.append(line)
        print(line, flush=True)
    if not a.profile:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "asg_time.json"), "w") as f:
            json.dump(records, f, indent=1)
        with open(os.path.join(a.out, "asg_time.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
