"""Time CTCLossSegmented (f32) with HIP events at B=256, T=1000, V=29, S<=200, targets with spaces, next to plain CTCLoss
forward and backward on the same batch in the same process.  Two cases: logits peaky along an alignment of the targets, so
that most words are cut; randn logits, so that nothing is cut.  Per phase: log-softmax + align, plan, read-back, gather,
loss calls, finish; and the number of segments of each kind, the number of loss groups, the largest gathered buffer.

    python tools/diag/segmented_time.py [--iters N] [--out FILE.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

from end2end_amd import CTCLoss, CTCLossSegmented
from end2end_amd.utils.alignment import get_alignment_3d

SPACE, PHASES = 28, ("align", "plan", "read-back", "gather", "loss", "finish")


def batch(B, T, V, S, peaky, seed):
    """Targets of words of 3..7 letters (1..27) separated by spaces; peaky: +8 on a frame path that spells them."""
    rng = np.random.default_rng(seed)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, V, generator=g)
    tg = torch.zeros((B, S), dtype=torch.long)
    xl, tl = [], []
    for b in range(B):
        n_lab = int(rng.integers(S // 2, S + 1))
        labs = []
        while len(labs) < n_lab:
            labs += [int(c) for c in rng.integers(1, SPACE, int(rng.integers(3, 8)))] + [SPACE]
        labs = labs[:n_lab]
        tg[b, :n_lab] = torch.tensor(labs)
        n = int(rng.integers(max(T // 2, 3 * n_lab), T + 1)) if b else T
        xl.append(n)
        tl.append(n_lab)
        if peaky:
            # every label gets its share of the frames; a blank in front of a repeated label
            cuts = np.sort(rng.choice(np.arange(1, n), n_lab - 1, replace=False))
            start = np.concatenate([[0], cuts])
            path = np.repeat(np.array(labs), np.diff(np.concatenate([start, [n]])))
            for i in range(1, n_lab):
                if labs[i] == labs[i - 1]:
                    path[start[i]] = 0
            keep = rng.random(n) < 0.97
            idx = torch.from_numpy(np.nonzero(keep)[0])
            x[b, idx, torch.from_numpy(path[keep])] += 8.0
    d = torch.device("cuda", 0)
    return x.to(d), tg.to(d), torch.tensor(xl).to(d), torch.tensor(tl).to(d)


def timed(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def phases(mod, args, iters):
    marks = []

    def mark(name):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        marks.append((name, e))

    total = dict.fromkeys(PHASES, 0.0)
    mod._mark = mark
    try:
        for it in range(iters + 3):
            del marks[:]
            mark("start")
            mod.compute(*args)
            torch.cuda.synchronize()
            if it >= 3:
                for (_, a), (name, b) in zip(marks, marks[1:]):
                    total[name] += a.elapsed_time(b)
    finally:
        mod._mark = None
    return {k: v / iters for k, v in total.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B, T, V, S = 256, 1000, 29, 200
    result = {"shape": dict(B=B, T=T, V=V, S=S, space_idx=SPACE, min_word_length=3), "iters": a.iters, "cases": {}}
    for name, peaky in (("peaky", True), ("randn", False)):
        x, tg, xl, tl = batch(B, T, V, S, peaky, 7)
        seg, ctc = CTCLossSegmented(space_idx=SPACE), CTCLoss()

        def step(mod):
            xr = x.detach().requires_grad_()
            mod(xr, tg, xl, tl).sum().backward()

        lp = torch.log_softmax(x, 2)
        r = {"align_kernel_ms": timed(lambda: get_alignment_3d(lp, tg, xl, tl, keep_on_device=True), a.iters),
             "ctc_loss_fwd_bwd_ms": timed(lambda: step(ctc), a.iters),
             "segmented_fwd_bwd_ms": timed(lambda: step(seg), a.iters),
             "phases_ms": phases(seg, (x, tg, xl, tl), a.iters)}
        p = seg.last_plan
        r.update(segments=dict(whole=p["whole"], frame=p["frame"], chunk=p["chunk"]), utterances_cut=p["utterances_cut"],
                 loss_groups=len(p["groups"]), groups=p["groups"], largest_gathered_buffer_elems=p["max_buffer_elems"],
                 input_elems=B * T * V)
        result["cases"][name] = r
        print("%s: CTCLoss fwd+bwd %.3f ms, CTCLossSegmented fwd+bwd %.3f ms" % (name, r["ctc_loss_fwd_bwd_ms"], r["segmented_fwd_bwd_ms"]))
        print("  e2e_ctc_align alone %.3f ms" % r["align_kernel_ms"])
        print("  phases (ms): " + ", ".join("%s %.3f" % (k, r["phases_ms"][k]) for k in PHASES))
        print("  segments %s, utterances cut %d, loss groups %d, largest gathered buffer %d of %d input elements"
              % (r["segments"], r["utterances_cut"], r["loss_groups"], r["largest_gathered_buffer_elems"], B * T * V))
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
