"""Time the pruned ASG beam search (cutoff_top_n; e2e_asg_beam_nbest_cut, e2e_asg_beam_stream_cut, f32) against the unpruned
search of the same library in ONE process, the legs of a shape alternating: HIP events around CALLS calls, ROUNDS interleaved
rounds after every leg has been warmed, median and least.  asg_beam_time.py's inputs (seed 2, randn * 3, random transitions):
  B=64 T=1000 V=29 (27 characters + 2 repeat labels), widths 100 and 16, without and with bench.py's synthetic 3-gram,
      cutoff_top_n in {5, 10, 20}
  B=64 T=256 V=128 width 16, cutoff_top_n = 20
  B=64 T=1000 V=29 width 100 in ten chunks of 100 frames (fed only, one read-out at the end), cutoff_top_n = 10
  B=64 T=1000 V=29 width 100 restricted to the 3-gram's words, cutoff_top_n = 10
Beside every ratio: what DESIGN.md 4.10's cost model (9 us per frame and 7 us per 1 000 pairs, without a model) predicts, and
-- as information only -- the share of the 64 utterances whose best hypothesis is the unpruned search's.

    python tools/diag/asg_beam_cut_time.py [--out profiles/asg_cut]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

import bench
from asg_beam_ab import ASG_LABELS, CTC_LABELS, DEV, inputs, load_arpa
from end2end_amd import _lib

ROUNDS, CALLS, CHUNK = 7, 3, 100
KNOBS = (1.0, 1.0, -10.0)
HEADER = 256


def predicted(W, V, K):
    return (9.0 + 7.0 * W * K / 1000.0) / (9.0 + 7.0 * W * V / 1000.0)


def whole(L, x, A, xl, bufs, Rl, W, space, lm, opts, top_n):
    """One whole call: top_n None, the unpruned entry."""
    B, T, V = x.shape
    out, out_len, n_hyp, scores, counts = bufs
    with_lm = 1 if lm else 0
    n = L.e2e_asg_beam_workspace_bytes(B, T, V, W, with_lm) if top_n is None else L.e2e_asg_beam_cut_workspace_bytes(B, T, V, W, with_lm, top_n)
    ws = torch.empty(n, dtype=torch.uint8, device=DEV)
    args = [x.data_ptr(), _lib.F32, *x.stride(), A.data_ptr(), xl.data_ptr(), B, T, V, Rl, W, space, lm, *KNOBS, W, out.data_ptr(), T,
            out_len.data_ptr(), n_hyp.data_ptr(), scores.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel(), None,
            C.byref(opts) if opts is not None else None]

    def call():
        rc = L.e2e_asg_beam_nbest_opt(*args) if top_n is None else L.e2e_asg_beam_nbest_cut(*args, top_n)
        assert rc == 0, L.e2e_last_error()
    return call, n


def chunked(L, x, A, bufs, Rl, W, space, lm, top_n):
    """All frames through the stream in chunks of CHUNK, fed only, the best hypotheses read out with the last chunk."""
    B, T, V = x.shape
    out, out_len, n_hyp, scores, counts = bufs
    with_lm = 1 if lm else 0
    row = L.e2e_asg_beam_stream_row_bytes(T, V, W, with_lm)
    state = torch.empty((B, row), dtype=torch.uint8, device=DEV)
    n = (L.e2e_asg_beam_stream_workspace_bytes(B, V, W, with_lm) if top_n is None
         else L.e2e_asg_beam_cut_stream_workspace_bytes(B, CHUNK, V, W, with_lm, top_n))
    ws = torch.empty(n, dtype=torch.uint8, device=DEV)
    cl = torch.full((B,), CHUNK, dtype=torch.long, device=DEV)
    done = torch.empty(B, dtype=torch.long, device=DEV)

    def call():
        state[:, :HEADER].zero_()                                  # (a new batch of utterances: part of what is timed)
        for a in range(0, T, CHUNK):
            c = x[:, a:a + CHUNK]
            args = [c.data_ptr(), _lib.F32, *c.stride(), A.data_ptr(), cl.data_ptr(), B, c.shape[1], V, Rl, W, space, lm, *KNOBS,
                    state.data_ptr(), row, T, W if a + CHUNK >= T else 0, out.data_ptr(), T, out_len.data_ptr(), n_hyp.data_ptr(),
                    scores.data_ptr(), counts.data_ptr(), done.data_ptr(), ws.data_ptr(), ws.numel(), None, None]
            rc = L.e2e_asg_beam_stream(*args) if top_n is None else L.e2e_asg_beam_stream_cut(*args, top_n)
            assert rc == 0, L.e2e_last_error()
    return call, n


def best(bufs):
    out, out_len = bufs[0], bufs[1]
    torch.cuda.synchronize()
    return out[:, 0].clone(), out_len[:, 0].clone()


def measure(legs, bufs):
    """{name: call} -> {name: record}: every leg warmed (and its best hypotheses kept), then the rounds, interleaved."""
    res, hyp = {k: [] for k in legs}, {}
    for k, f in legs.items():
        f()
        f()
        hyp[k] = best(bufs)
    for _ in range(ROUNDS):
        for k, f in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(CALLS):
                f()
            e1.record()
            torch.cuda.synchronize()
            res[k].append(e0.elapsed_time(e1) / CALLS)
    ids0, len0 = hyp["unpruned"]
    out = {}
    for k, v in res.items():
        ids, ln = hyp[k]
        same = ((ln == len0) & ((ids == ids0) | (torch.arange(ids.shape[1], device=ids.device)[None, :] >= len0[:, None])).all(1))
        out[k] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "best_equals_unpruned": float(same.float().mean())}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "asg_cut"))
    a = ap.parse_args()
    L = _lib.load()
    records, lines = [], []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "synthetic_3gram.arpa")
        bench.synthetic_arpa(path, CTC_LABELS)
        plain, lex = load_arpa(L, path), load_arpa(L, path)
        assert L.e2e_lm_enable_lexicon(lex) == 0, L.e2e_last_error()
        on = _lib.AsgBeamOpts(1, None)
        # (what, B, T, V, R, width, model, opts, the cutoff_top_n values, streamed)
        shapes = [("whole", 64, 1000, 29, 2, W, lm, None, (5, 10, 20), False) for W in (100, 16) for lm in (None, plain)]
        shapes += [("whole", 64, 256, 128, 0, 16, None, None, (20,), False),
                   ("ten chunks", 64, 1000, 29, 2, 100, None, None, (10,), True),
                   ("ten chunks", 64, 1000, 29, 2, 100, plain, None, (10,), True),
                   ("restricted", 64, 1000, 29, 2, 100, lex, on, (10,), False)]
        say("%s; ms per call, median of %d interleaved rounds of %d calls (least in brackets); pruned / unpruned beside the cost "
            "model's prediction; the share of utterances whose best hypothesis is the unpruned one" % (torch.cuda.get_device_name(0), ROUNDS, CALLS))
        for what, B, T, V, Rl, W, lm, opts, tops, streamed in shapes:
            x, A, xl, bufs = inputs(B, T, V, W)
            space = 0 if V == 29 else -1
            legs, nbytes = {}, {}
            for top_n in (None,) + tuple(tops):
                name = "unpruned" if top_n is None else "cutoff_top_n=%d" % top_n
                if streamed:
                    legs[name], nbytes[name] = chunked(L, x, A, bufs, Rl, W, space, lm, top_n)
                else:
                    legs[name], nbytes[name] = whole(L, x, A, xl, bufs, Rl, W, space, lm, opts, top_n)
            r = measure(legs, bufs)
            base = r["unpruned"]["median_ms"]
            model = "3-gram" if lm else "no LM"
            for top_n in (None,) + tuple(tops):
                name = "unpruned" if top_n is None else "cutoff_top_n=%d" % top_n
                v = r[name]
                v.update(what=what, B=B, T=T, V=V, num_replabels=Rl, beam_width=W, lm="synthetic 3-gram (10k words)" if lm else None,
                         cutoff_top_n=top_n, dtype="f32", workspace_bytes=nbytes[name], rounds=ROUNDS, calls_per_round=CALLS,
                         device=torch.cuda.get_device_name(0))
                line = "%-10s B=%d T=%d V=%d width %3d %-6s %-16s %8.2f ms (%.2f)" % (what, B, T, V, W, model, name, v["median_ms"], v["min_ms"])
                if top_n is not None:
                    v["pruned_over_unpruned"] = v["median_ms"] / base
                    v["cost_model_predicts"] = predicted(W, V, min(top_n, V)) if not lm else None
                    line += "  x %.3f" % v["pruned_over_unpruned"]
                    line += " (model: %.3f)" % v["cost_model_predicts"] if not lm else " (model: none with an LM)"
                    line += "  best hypothesis kept in %.0f %%" % (100 * v["best_equals_unpruned"])
                records.append(v)
                say(line)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "asg_beam_cut_time.json"), "w") as f:
        json.dump(records, f, indent=1)
    with open(os.path.join(a.out, "asg_beam_cut_time.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
