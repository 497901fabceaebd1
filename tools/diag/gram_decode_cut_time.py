"""Time the pruned Gram-CTC beam search (cutoff_top_n; e2e_gram_ctc_beam_nbest_cut through GramCTCDecoderEngine, f32
log-probabilities) beside the unpruned search of the same library, in one process, on gram_decode_time.py's shapes and seeds:
a HIP event pair around every call, the median of `--iters` calls after warm-up.
  B=64 T=256  V=8000 (orders 2-4) width 16, cutoff_top_n=40, and width 100 (which has no unpruned counterpart)
  B=64 T=1000 V=379 (300 bigrams, 50 trigrams) width 100, cutoff_top_n=40, without a model and with bench.py's synthetic 3-gram
  B=64 T=1000 V=29 unigrams only width 100, cutoff_top_n=10
and the workspace bytes of each.  The records go to profiles/gram_cut/.

    python tools/diag/gram_decode_cut_time.py [--iters N] [--out profiles/gram_cut]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bench
from end2end_amd import _lib
from end2end_amd.engines import GramCTCDecoderEngine
from gram_decode_time import batch
from gram_time import table

DEV = torch.device("cuda", 0)


def median_ms(fn, iters, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gram_cut"))
    a = ap.parse_args()
    L = _lib.load()
    labels = ["_"] + [chr(97 + i) for i in range(26)] + [" ", "'"]
    R = len(labels)
    rng = np.random.default_rng(7)
    small, Vs = table(rng, R, {2: 300, 3: 50})
    big, Vb = table(rng, R, {2: 700, 3: 4000, 4: 3271})
    records, lines = [], []
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "synthetic_3gram.arpa")
        bench.synthetic_arpa(path, labels)
        # (table, V, B, T, seed, width, cutoff_top_n, with the model, is there an unpruned call of this width)
        for l2i, V, B, T, seed, W, top_n, with_lm, unpruned in ((big, Vb, 64, 256, 8, 16, 40, False, True),
                                                                (big, Vb, 64, 256, 8, 100, 40, False, False),
                                                                (small, Vs, 64, 1000, 7, 100, 40, False, True),
                                                                (small, Vs, 64, 1000, 7, 100, 40, True, True),
                                                                ({}, R, 64, 1000, 7, 100, 10, False, True)):
            lp, xl = batch(B, T, V, seed)
            rec = {"B": B, "T": T, "V": V, "beam_width": W, "cutoff_top_n": top_n, "cutoff_prob": 1.0, "dtype": "f32",
                   "lm": "synthetic 3-gram (10k words)" if with_lm else None, "iters": a.iters,
                   "device": torch.cuda.get_device_name(0)}
            for name, kw in (("pruned", dict(cutoff_top_n=top_n)), ("unpruned", {})):
                if name == "unpruned" and not unpruned:
                    continue
                eng = GramCTCDecoderEngine(0, R, V, l2i, W, labels, keep_on_device=True, **kw)
                if with_lm:
                    eng.configure(path, 1.0, 1.0, -10.0, True)
                K = eng.max_order
                rec[name + "_ms"] = median_ms(lambda: eng.decode_nbest(lp, xl, nbest=1), a.iters)
                rec[name + "_workspace_bytes"] = (
                    L.e2e_gram_beam_cut_workspace_bytes(B, T, V, K, W, int(with_lm), int(with_lm), top_n) if kw
                    else L.e2e_gram_beam_workspace_bytes_lm(B, T, V, K, W, int(with_lm)))
            line = "B=%d T=%d V=%d width %d cutoff_top_n=%d%s: pruned %.2f ms (workspace %.1f MB)" % (
                B, T, V, W, top_n, " 3-gram" if with_lm else "", rec["pruned_ms"], rec["pruned_workspace_bytes"] / 1e6)
            if unpruned:
                rec["unpruned_over_pruned"] = rec["unpruned_ms"] / rec["pruned_ms"]
                line += ", unpruned %.2f ms (workspace %.1f MB): x %.2f" % (
                    rec["unpruned_ms"], rec["unpruned_workspace_bytes"] / 1e6, rec["unpruned_over_pruned"])
            records.append(rec)
            lines.append(line)
            print(line, flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "gram_decode_cut_time.json"), "w") as f:
        json.dump(records, f, indent=1)
    with open(os.path.join(a.out, "gram_decode_cut_time.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
