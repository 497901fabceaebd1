"""A/B builds of libe2e_ctc.so on the ASG beam search in ONE process: tools/diag/asg_beam_time.py's five shapes (f32, HIP events
around e2e_asg_beam_nbest, 20 calls after 3 of warm-up), tools/diag/ab_time.py's alternation (12 interleaved rounds, median
and least).  Every library loads its own copy of bench.py's synthetic 3-gram.  Give the parent build twice (two copies of one
file) to see the spread a build shows against itself.

    python tools/diag/asg_beam_ab.py [--out profiles/asg_beam/unrestricted_ab.txt] LIB [LIB ...]

--restricted: instead, this build alone (the first LIB) on the two V = 29 shapes: unrestricted, restricted to the synthetic
3-gram's words (e2e_asg_beam_nbest_opt), and restricted to a word list of the same words without the model -- beside the search
without a model.  The same rounds.
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch

import bench
from end2end_amd import _lib

DEV = torch.device("cuda", 0)
CASES = [(64, 1000, 29, 2, 100, False), (64, 1000, 29, 2, 100, True), (64, 1000, 29, 2, 16, False), (64, 1000, 29, 2, 16, True),
         (64, 256, 128, 0, 16, False)]
ASG_LABELS = [" "] + [chr(97 + i) for i in range(26)] + ["<1>", "<2>"]
CTC_LABELS = ["_"] + [chr(97 + i) for i in range(26)] + [" ", "'"]
ROUNDS, WARM, ITERS = 12, 3, 20


def bind(path):
    L = C.CDLL(path)
    ref = _lib.load()
    for name in ("e2e_asg_beam_workspace_bytes", "e2e_asg_beam_nbest", "e2e_lm_load_arpa", "e2e_last_error"):
        getattr(L, name).restype = getattr(ref, name).restype
        if name != "e2e_last_error":
            getattr(L, name).argtypes = getattr(ref, name).argtypes
    return L


def strings(items):
    arr = (C.c_char_p * len(items))(*[s.encode() for s in items])
    return arr


def arpa_words(path):
    """The words of the file's unigrams, <unk>, <s> and </s> left out."""
    words, on = [], False
    for line in open(path, encoding="utf-8"):
        line = line.strip()
        if line.startswith("\\"):
            on = line == "\\1-grams:"
            continue
        f = line.split()
        if on and len(f) >= 2 and f[1] not in ("<unk>", "<s>", "</s>"):
            words.append(f[1])
    return words


def load_arpa(L, path):
    h = C.c_void_p()
    rc = L.e2e_lm_load_arpa(path.encode(), strings(ASG_LABELS), len(ASG_LABELS), 1, C.byref(h))
    assert rc == 0, L.e2e_last_error()
    return h


def inputs(B, T, V, W):
    g = torch.Generator().manual_seed(2)
    x = (torch.randn(B, T, V, generator=g) * 3).to(DEV)
    A = torch.randn(V, V, generator=g).to(DEV)
    xl = torch.full((B,), T, dtype=torch.long, device=DEV)
    bufs = (torch.empty((B, W, T + 1), dtype=torch.long, device=DEV), torch.empty((B, W), dtype=torch.long, device=DEV),
            torch.empty(B, dtype=torch.long, device=DEV), torch.empty((B, W, 3), dtype=torch.float64, device=DEV),
            torch.empty((B, W, 2), dtype=torch.int32, device=DEV))
    return x, A, xl, bufs


def caller(L, x, A, xl, bufs, Rl, W, space, lm, ws, opts=None):
    B, T, V = x.shape
    out, out_len, n_hyp, scores, counts = bufs
    args = [x.data_ptr(), _lib.F32, *x.stride(), A.data_ptr(), xl.data_ptr(), B, T, V, Rl, W, space, lm, 1.0, 1.0, -10.0, W,
            out.data_ptr(), T, out_len.data_ptr(), n_hyp.data_ptr(), scores.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel(),
            None]

    def call():
        rc = L.e2e_asg_beam_nbest(*args) if opts is None else L.e2e_asg_beam_nbest_opt(*args, C.byref(opts))
        assert rc == 0, L.e2e_last_error()
    return call


def rounds(calls):
    """{name: call} -> {name: [ms per call, one per round]}, the calls interleaved."""
    res = {k: [] for k in calls}
    for _ in range(ROUNDS):
        for k, call in calls.items():
            for _ in range(WARM):
                call()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(ITERS):
                call()
            e1.record()
            torch.cuda.synchronize()
            res[k].append(e0.elapsed_time(e1) / ITERS)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--restricted", action="store_true")
    ap.add_argument("libs", nargs="+")
    a = ap.parse_args()
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "synthetic_3gram.arpa")
        bench.synthetic_arpa(path, CTC_LABELS)
        if a.restricted:
            L = _lib.load() if os.path.abspath(a.libs[0]) == os.path.abspath(_lib.LIB_PATH) else None
            assert L is not None, "--restricted times the package's own library"
            words = arpa_words(path)
            plain, lex, lst = load_arpa(L, path), load_arpa(L, path), C.c_void_p()
            assert L.e2e_lm_enable_lexicon(lex) == 0, L.e2e_last_error()
            rc = L.e2e_lm_load_words(strings(words), len(words), strings(ASG_LABELS), len(ASG_LABELS), 1, C.byref(lst))
            assert rc == 0 and L.e2e_lm_enable_lexicon(lst) == 0, L.e2e_last_error()
            say("%d words; ms per call, median of %d rounds of %d calls (least in brackets)" % (len(words), ROUNDS, ITERS))
            for B, T, V, Rl, W in [(64, 1000, 29, 2, 100), (64, 1000, 29, 2, 16)]:
                x, A, xl, bufs = inputs(B, T, V, W)
                ws = torch.empty(L.e2e_asg_beam_workspace_bytes(B, T, V, W, 1), dtype=torch.uint8, device=DEV)
                on = _lib.AsgBeamOpts(1, None)
                calls = {"no model": caller(L, x, A, xl, bufs, Rl, W, 0, None, ws),
                         "3-gram": caller(L, x, A, xl, bufs, Rl, W, 0, plain, ws),
                         "3-gram, restricted": caller(L, x, A, xl, bufs, Rl, W, 0, lex, ws, on),
                         "word list, unrestricted": caller(L, x, A, xl, bufs, Rl, W, 0, lst, ws),
                         "word list, restricted": caller(L, x, A, xl, bufs, Rl, W, 0, lst, ws, on)}
                res = rounds(calls)
                for k, v in res.items():
                    say("B=%d T=%d V=%d width %3d %-24s %8.2f ms (%.2f)  %.2f us/frame" % (B, T, V, W, k, statistics.median(v), min(v),
                                                                                      statistics.median(v) * 1e3 / T))
        else:
            libs = {p: bind(os.path.join(ROOT, p)) for p in a.libs}
            lms = {p: load_arpa(L, path) for p, L in libs.items()}
            say("ms per call, median of %d rounds of %d calls (least in brackets); the libraries interleaved" % (ROUNDS, ITERS))
            for B, T, V, Rl, W, with_lm in CASES:
                x, A, xl, bufs = inputs(B, T, V, W)
                n = max(L.e2e_asg_beam_workspace_bytes(B, T, V, W, 1) for L in libs.values())
                ws = torch.empty(n, dtype=torch.uint8, device=DEV)
                calls = {p: caller(L, x, A, xl, bufs, Rl, W, 0 if V == 29 else -1, lms[p] if with_lm else None, ws) for p, L in libs.items()}
                res = rounds(calls)
                for p, v in res.items():
                    say("B=%d T=%d V=%d width %3d %-6s %-36s %8.3f ms (%.3f)" % (B, T, V, W, "3-gram" if with_lm else "no LM",
                                                                               os.path.basename(p), statistics.median(v), min(v)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
