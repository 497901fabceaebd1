"""Time the Gram-CTC beam search restricted to a vocabulary, and its timesteps (e2e_gram_ctc_beam_nbest_opt, f32
log-probabilities), with HIP events around the C call, as tools/diag/gram_decode_lm_time.py times the search with a model: the
same three shapes -- B=64 T=1000 at the loss's headline table (V=379) at widths 100 and 16, and unigrams only (V=29) at
width 100 --, the same model (bench.py's synthetic 10k-word 3-gram, its lexicon enabled, one handle for every variant).  Four
variants in one process, interleaved round by round: unrestricted, restricted to the model's words, and each of the two with
timesteps.  The records go to profiles/gram_decode/.

    python tools/diag/gram_decode_lexicon_time.py [--rounds N] [--iters N] [--out profiles/gram_decode]
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
from end2end_amd import _runtime as R
from end2end_amd._runtime import _C
from end2end_amd.engines import GramCTCDecoderEngine, LanguageModel
from gram_time import table

DEV = torch.device("cuda", 0)
VARIANTS = (("unrestricted", False, False), ("restricted", True, False), ("unrestricted_ts", False, True),
            ("restricted_ts", True, True))


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gram_decode"))
    a = ap.parse_args()
    labels = ["_"] + [chr(97 + i) for i in range(26)] + [" ", "'"]
    nb = len(labels)
    space = labels.index(" ")
    code = R.dtype_code(torch.float32)
    stream = R.stream_handle(DEV)
    B, T = 64, 1000
    l2i, V = table(np.random.default_rng(7), nb, {2: 300, 3: 50})
    records, lines = [], []
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "synthetic_3gram.arpa")
        bench.synthetic_arpa(path, labels)
        lm = LanguageModel(path, labels, True, lexicon=True)
        h = lm.on(DEV).handle
        for grams, V, W in ((l2i, V, 100), (l2i, V, 16), ({}, nb, 100)):
            g = torch.Generator().manual_seed(7)
            lp = torch.log_softmax(torch.randn(B, T, V, generator=g), -1).to(DEV)
            xl = torch.randint(T // 2, T + 1, (B,), generator=g)
            xl[0] = T
            xl = xl.to(DEV)
            eng = GramCTCDecoderEngine(0, nb, V, grams, W)
            ids, lens = eng._table(DEV)
            K, N = eng.max_order, 1
            sB, sT, sV = lp.stride()
            max_out = T * K
            out = torch.empty((B, N, max_out), dtype=torch.long, device=DEV)
            ts = torch.empty((B, N, max_out), dtype=torch.long, device=DEV)
            out_len = torch.empty((B, N), dtype=torch.long, device=DEV)
            n_hyp = torch.empty(B, dtype=torch.long, device=DEV)
            scores = torch.empty((B, N, 3), dtype=torch.float64, device=DEV)
            counts = torch.empty((B, N, 2), dtype=torch.int32, device=DEV)
            ws = torch.empty(_C.gram_beam_workspace_bytes_lm(B, T, V, K, W, True), dtype=torch.uint8, device=DEV)

            def call(restrict, with_ts):
                _C.gram_ctc_beam_nbest_opt(lp.data_ptr(), code, sB, sT, sV, xl.data_ptr(), B, T, V, ids.data_ptr(), lens.data_ptr(),
                                           K, nb, W, space, h, 1.0, 1.0, -10.0, N, out.data_ptr(), max_out, out_len.data_ptr(),
                                           n_hyp.data_ptr(), scores.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel(),
                                           stream, (restrict, ts.data_ptr() if with_ts else 0))

            ms = {name: [] for name, _, _ in VARIANTS}
            info = {}
            for name, restrict, with_ts in VARIANTS:                  # warm-up, and what the variants decode
                for _ in range(2):
                    call(restrict, with_ts)
                torch.cuda.synchronize()
                assert int(n_hyp.min()) >= 0
                info[name] = dict(mean_length=float(out_len.double().mean()), mean_oov=float(counts[:, :, 1].double().mean()),
                                  utterances_without_hypothesis=int((n_hyp == 0).sum()))
            for _ in range(a.rounds):
                for name, restrict, with_ts in VARIANTS:
                    ms[name].append(timed(lambda: call(restrict, with_ts), a.iters))
            rec = {"B": B, "T": T, "V": V, "num_base_labels": nb, "max_order": K, "beam_width": W, "dtype": "f32",
                   "lm": "synthetic 3-gram (10k words), lexicon enabled", "rounds": a.rounds, "iters": a.iters,
                   "device": torch.cuda.get_device_name(0), "decoded": info}
            for name in ms:
                rec[name + "_ms"] = statistics.median(ms[name])
                rec[name + "_ms_rounds"] = ms[name]
            rec["restricted_over_unrestricted"] = rec["restricted_ms"] / rec["unrestricted_ms"]
            rec["ts_over_no_ts_unrestricted"] = rec["unrestricted_ts_ms"] / rec["unrestricted_ms"]
            rec["ts_over_no_ts_restricted"] = rec["restricted_ts_ms"] / rec["restricted_ms"]
            line = ("B=%d T=%d V=%d width %d: unrestricted %.2f ms, restricted %.2f ms (x %.3f); with timesteps %.2f ms (x %.3f) "
                    "and %.2f ms (x %.3f); mean length %.0f -> %.0f ids, OOVs per result %.1f -> %.1f" % (
                        B, T, V, W, rec["unrestricted_ms"], rec["restricted_ms"], rec["restricted_over_unrestricted"],
                        rec["unrestricted_ts_ms"], rec["ts_over_no_ts_unrestricted"], rec["restricted_ts_ms"],
                        rec["ts_over_no_ts_restricted"], info["unrestricted"]["mean_length"], info["restricted"]["mean_length"],
                        info["unrestricted"]["mean_oov"], info["restricted"]["mean_oov"]))
            records.append(rec)
            lines.append(line)
            print(line, flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "gram_decode_lexicon_time.json"), "w") as f:
        json.dump(records, f, indent=1)
    with open(os.path.join(a.out, "gram_decode_lexicon_time.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
