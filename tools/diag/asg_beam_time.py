"""Time the ASG beam search (e2e_asg_beam_nbest, f32) with HIP events around the C call: 20 calls after 3 of warm-up, at
B=64 T=1000 V=29 (27 characters + 2 repeat labels) at widths 100 and 16 without and with bench.py's synthetic 3-gram, and at
B=64 T=256 V=128 at width 16.  Beside each, in the same process: e2e_asg_viterbi on the same input, and e2e_ctc_beam_nbest on
the log-softmax of the same B, T, V at the same width (with the same model where there is one).  The records go to
profiles/asg_beam/.

    python tools/diag/asg_beam_time.py [--iters N] [--out profiles/asg_beam] [--profile] [--scan]

--scan: the search alone at B=64 T=1000 V=29 over widths 1 .. 128, without and with the model -- the fixed cost of a frame and
the cost of a pair, read off the line through them (asg_beam_scan.txt).

--profile: three calls of each and no records, for `rocprofv3 --kernel-trace --stats -- python tools/diag/asg_beam_time.py --profile`.
"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch

import bench
from end2end_amd import _runtime as R
from end2end_amd._runtime import _C
from end2end_amd.engines import LanguageModel

DEV = torch.device("cuda", 0)
CASES = [(64, 1000, 29, 2, 100, False), (64, 1000, 29, 2, 100, True), (64, 1000, 29, 2, 16, False), (64, 1000, 29, 2, 16, True),
         (64, 256, 128, 0, 16, False)]


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


def buffers(B, T, N):
    return (torch.empty((B, N, T + 1), dtype=torch.long, device=DEV), torch.empty((B, N), dtype=torch.long, device=DEV),
            torch.empty(B, dtype=torch.long, device=DEV), torch.empty((B, N, 3), dtype=torch.float64, device=DEV),
            torch.empty((B, N, 2), dtype=torch.int32, device=DEV))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "asg_beam"))
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--scan", action="store_true")
    a = ap.parse_args()
    if a.profile:
        a.iters = 3
    asg_labels = [" "] + [chr(97 + i) for i in range(26)] + ["<1>", "<2>"]
    ctc_labels = ["_"] + [chr(97 + i) for i in range(26)] + [" ", "'"]
    code = R.dtype_code(torch.float32)
    stream = R.stream_handle(DEV)
    records, lines = [], []
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "synthetic_3gram.arpa")
        bench.synthetic_arpa(path, ctc_labels)
        lm_asg = LanguageModel(path, asg_labels, True)
        lm_ctc = LanguageModel(path, ctc_labels, True)
        cases = [(64, 1000, 29, 2, W, lm) for lm in (False, True) for W in (1, 4, 16, 50, 100, 128)] if a.scan else CASES
        for B, T, V, Rl, W, with_lm in cases:
            g = torch.Generator().manual_seed(2)
            x = (torch.randn(B, T, V, generator=g) * 3).to(DEV)
            A = torch.randn(V, V, generator=g).to(DEV)
            lp = torch.log_softmax(x, -1)
            xl = torch.full((B,), T, dtype=torch.long, device=DEV)
            sB, sT, sV = x.stride()
            out, out_len, n_hyp, scores, counts = buffers(B, T, W)
            ws = torch.empty(_C.asg_beam_workspace_bytes(B, T, V, W, with_lm), dtype=torch.uint8, device=DEV)
            space = 0 if V == 29 else -1
            h_asg = lm_asg.on(DEV).handle if with_lm else 0

            def asg_beam():
                _C.asg_beam_nbest(x.data_ptr(), code, sB, sT, sV, A.data_ptr(), xl.data_ptr(), B, T, V, Rl, W, space, h_asg,
                                  1.0, 1.0, -10.0, W, out.data_ptr(), T, out_len.data_ptr(), n_hyp.data_ptr(),
                                  scores.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel(), stream)

            path_buf = torch.empty((B, T), dtype=torch.long, device=DEV)
            coll = torch.empty((B, T), dtype=torch.long, device=DEV)
            vscores = torch.empty(B, dtype=torch.float64, device=DEV)
            vlen = torch.empty(B, dtype=torch.long, device=DEV)
            vws = torch.empty(_C.asg_viterbi_workspace_bytes(B, T, V), dtype=torch.uint8, device=DEV)

            def viterbi():
                _C.asg_viterbi(x.data_ptr(), code, sB, sT, sV, A.data_ptr(), xl.data_ptr(), B, T, V, path_buf.data_ptr(), -100,
                               vscores.data_ptr(), coll.data_ptr(), vlen.data_ptr(), vws.data_ptr(), vws.numel(), stream)

            cws = torch.empty(_C.ctc_beam_nbest_workspace_bytes(B, T, V, W, with_lm, False), dtype=torch.uint8, device=DEV)
            h_ctc = lm_ctc.on(DEV).handle if with_lm else 0
            cspace = ctc_labels.index(" ") if V == 29 else -1

            def ctc_beam():
                _C.ctc_beam_nbest(lp.data_ptr(), code, sB, sT, sV, xl.data_ptr(), B, T, V, 0, W, cspace, h_ctc, 1.0, 1.0, -10.0, W,
                                  out.data_ptr(), T + 1, out_len.data_ptr(), n_hyp.data_ptr(), scores.data_ptr(),
                                  counts.data_ptr(), 0, cws.data_ptr(), cws.numel(), stream)

            rec = {"B": B, "T": T, "V": V, "num_replabels": Rl, "beam_width": W, "lm": "synthetic 3-gram (10k words)" if with_lm else None,
                   "dtype": "f32", "iters": a.iters, "device": torch.cuda.get_device_name(0),
                   "asg_beam_ms": timed(asg_beam, a.iters)}
            if a.scan:
                rec["pairs_per_frame"] = W * V
                records.append(rec)
                lines.append("width %3d (%4d pairs) %s: %.2f us per frame" % (W, W * V, "3-gram" if with_lm else "no LM", rec["asg_beam_ms"] * 1e3 / T))
                print(lines[-1], flush=True)
                continue
            rec["asg_viterbi_ms"] = timed(viterbi, a.iters)
            rec["ctc_beam_nbest_ms"] = timed(ctc_beam, a.iters)
            rec["asg_beam_us_per_frame"] = rec["asg_beam_ms"] * 1e3 / T
            rec["ctc_beam_us_per_frame"] = rec["ctc_beam_nbest_ms"] * 1e3 / T
            assert int(n_hyp.min()) >= 0
            records.append(rec)
            line = "B=%d T=%d V=%d width %d %s: ASG beam %.2f ms (%.2f us/frame), CTC beam %.2f ms (%.2f us/frame), best path %.3f ms" % (
                B, T, V, W, "3-gram" if with_lm else "no LM", rec["asg_beam_ms"], rec["asg_beam_us_per_frame"],
                rec["ctc_beam_nbest_ms"], rec["ctc_beam_us_per_frame"], rec["asg_viterbi_ms"])
            lines.append(line)
            print(line, flush=True)
    if not a.profile:
        os.makedirs(a.out, exist_ok=True)
        name = "asg_beam_scan" if a.scan else "asg_beam_time"
        with open(os.path.join(a.out, name + ".json"), "w") as f:
            json.dump(records, f, indent=1)
        with open(os.path.join(a.out, name + ".txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
