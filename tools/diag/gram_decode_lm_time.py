"""Time the Gram-CTC beam search with a word language model (e2e_gram_ctc_beam_nbest_lm, f32 log-probabilities) with HIP
events around the C call, 20 calls after 3 of warm-up, beside e2e_gram_ctc_beam_nbest on the same input in the same process:
B=64 T=1000 at the loss's headline table (R=29: 28 unigrams, 300 bigrams, 50 trigrams, V=379) at widths 100 and 16, and with
unigrams only (V=29) at width 100 -- there also e2e_ctc_beam_nbest with the same model.  The model is bench.py's synthetic
10k-word 3-gram, the base labels its alphabet (the space is base id 27).  The records go to profiles/gram_decode/.

    python tools/diag/gram_decode_lm_time.py [--iters N] [--out profiles/gram_decode]
"""
import argparse
import json
import os
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
        lm = LanguageModel(path, labels, True)
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
            out_len = torch.empty((B, N), dtype=torch.long, device=DEV)
            n_hyp = torch.empty(B, dtype=torch.long, device=DEV)
            scores = torch.empty((B, N, 3), dtype=torch.float64, device=DEV)
            counts = torch.empty((B, N, 2), dtype=torch.int32, device=DEV)
            ws_bytes = _C.gram_beam_workspace_bytes_lm(B, T, V, K, W, True)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)

            def plain():
                _C.gram_ctc_beam_nbest(lp.data_ptr(), code, sB, sT, sV, xl.data_ptr(), B, T, V, ids.data_ptr(), lens.data_ptr(), K,
                                       W, N, out.data_ptr(), max_out, out_len.data_ptr(), n_hyp.data_ptr(), scores.data_ptr(),
                                       ws.data_ptr(), ws.numel(), stream)

            def with_lm(handle=h):
                _C.gram_ctc_beam_nbest_lm(lp.data_ptr(), code, sB, sT, sV, xl.data_ptr(), B, T, V, ids.data_ptr(), lens.data_ptr(),
                                          K, nb, W, space, handle, 1.0, 1.0, -10.0, N, out.data_ptr(), max_out,
                                          out_len.data_ptr(), n_hyp.data_ptr(), scores.data_ptr(), counts.data_ptr(),
                                          ws.data_ptr(), ws.numel(), stream)

            rec = {"B": B, "T": T, "V": V, "num_base_labels": nb, "max_order": K, "beam_width": W, "dtype": "f32",
                   "lm": "synthetic 3-gram (10k words)", "iters": a.iters, "device": torch.cuda.get_device_name(0),
                   "workspace_bytes_no_lm": _C.gram_beam_workspace_bytes(B, T, V, K, W), "workspace_bytes_lm": ws_bytes,
                   "gram_beam_ms": timed(plain, a.iters), "gram_beam_lm_ms": timed(with_lm, a.iters),
                   "gram_beam_words_only_ms": timed(lambda: with_lm(0), a.iters)}
            assert int(n_hyp.min()) >= 0
            rec["lm_over_no_lm"] = rec["gram_beam_lm_ms"] / rec["gram_beam_ms"]
            line = "B=%d T=%d V=%d width %d: no LM %.2f ms, 3-gram %.2f ms (x %.2f), lm == NULL with wip %.2f ms" % (
                B, T, V, W, rec["gram_beam_ms"], rec["gram_beam_lm_ms"], rec["lm_over_no_lm"], rec["gram_beam_words_only_ms"])
            if not grams:                                         # unigrams only: CTCDecoder's search with the same model
                cws = torch.empty(_C.ctc_beam_nbest_workspace_bytes(B, T, V, W, True, False), dtype=torch.uint8, device=DEV)
                cout = torch.empty((B, N, T + 1), dtype=torch.long, device=DEV)

                def ctc_beam():
                    _C.ctc_beam_nbest(lp.data_ptr(), code, sB, sT, sV, xl.data_ptr(), B, T, V, 0, W, space, h, 1.0, 1.0, -10.0, N,
                                      cout.data_ptr(), T + 1, out_len.data_ptr(), n_hyp.data_ptr(), scores.data_ptr(),
                                      counts.data_ptr(), 0, cws.data_ptr(), cws.numel(), stream)

                rec["ctc_beam_nbest_lm_ms"] = timed(ctc_beam, a.iters)
                rec["lm_over_ctc_beam"] = rec["gram_beam_lm_ms"] / rec["ctc_beam_nbest_lm_ms"]
                line += ", CTC beam with the model %.2f ms (x %.2f)" % (rec["ctc_beam_nbest_lm_ms"], rec["lm_over_ctc_beam"])
            records.append(rec)
            lines.append(line)
            print(line, flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "gram_decode_lm_time.json"), "w") as f:
        json.dump(records, f, indent=1)
    with open(os.path.join(a.out, "gram_decode_lm_time.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
