"""What the vocabulary restriction costs at BASELINE configs[3] (B=64, T=1500, V=29, beam 100, the synthetic 3-gram): HIP events,
two builds of libe2e_ctc.so in ONE process, interleaved rounds, median:
    python3 tools/diag/time_beam_lexicon.py [build/diag/ab_parent.so]
(a) e2e_ctc_beam and the n-best call with the flag off (e2e_ctc_beam_nbest_opt, nbest = 1) of this tree against the parent
    commit's build (the argument: the parent's library, built from a checkout of that commit with its Makefile);
(b) the same two on a model whose lexicon has been built (the tables then hold the prefixes too), still unrestricted;
(c) the restricted call against the flag-off call of this build;
(d) the load time of the model with and without e2e_lm_enable_lexicon (wall clock, median of 3), the table sizes (E2E_LM_DEBUG).
LEXICON_JSON=path: also write the numbers there (profiles/lexicon/)."""
import ctypes as C, json, os, statistics, sys, tempfile, time
root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, root)
os.environ["E2E_LM_DEBUG"] = "1"
import torch
import bench
from end2end_amd import _lib

ROUNDS, CALLS = 7, 3
B, T, V, W = 64, 1500, 29, 100
this = _lib.load()
parent = None
if len(sys.argv) > 1:
    parent = C.CDLL(os.path.join(root, sys.argv[1]))
    for name in ("e2e_ctc_beam", "e2e_ctc_beam_nbest", "e2e_lm_load_arpa", "e2e_lm_free"):
        getattr(parent, name).restype = getattr(this, name).restype
        getattr(parent, name).argtypes = getattr(this, name).argtypes
d = torch.device("cuda", 0)
labels = ["_"] + [chr(97 + i) for i in range(26)] + [" ", "'"]
g = torch.Generator().manual_seed(2)
x = torch.log_softmax(torch.randn(B, T, V, generator=g) * 3, -1).to(d)
xl = torch.full((B,), T, dtype=torch.long, device=d)
max_out = T + 1
out = torch.empty((B, 1, max_out), dtype=torch.long, device=d)
out_len = torch.empty((B, 1), dtype=torch.long, device=d)
n_hyp = torch.empty(B, dtype=torch.long, device=d)
scores = torch.empty((B, 1, 3), dtype=torch.float64, device=d)
counts = torch.empty((B, 1, 2), dtype=torch.int32, device=d)
ws = torch.empty(this.e2e_ctc_beam_nbest_workspace_bytes(B, T, V, W, 1, 0), dtype=torch.uint8, device=d)
stream = _lib.stream_ptr(d)
ARGS = (1.0, 1.0, -10.0)


def load_lm(L, path, lexicon=False):
    h = C.c_void_p()
    arr = (C.c_char_p * V)(*[s.encode() for s in labels])
    assert L.e2e_lm_load_arpa(path.encode(), arr, V, 1, C.byref(h)) == 0
    if lexicon:
        assert L.e2e_lm_enable_lexicon(h) == 0, L.e2e_last_error()
    return h


def plain(L, lm):
    return lambda: L.e2e_ctc_beam(x.data_ptr(), _lib.F32, *x.stride(), xl.data_ptr(), B, T, V, 0, W, 27, lm, *ARGS,
                                  out.data_ptr(), max_out, out_len.data_ptr(), ws.data_ptr(), ws.numel(), stream)


def nbest_args(lm):
    return (x.data_ptr(), _lib.F32, *x.stride(), xl.data_ptr(), B, T, V, 0, W, 27, lm, *ARGS, 1, out.data_ptr(), max_out,
            out_len.data_ptr(), n_hyp.data_ptr(), scores.data_ptr(), counts.data_ptr(), None, ws.data_ptr(), ws.numel(), stream)


def nbest_parent(lm):
    return lambda: parent.e2e_ctc_beam_nbest(*nbest_args(lm))


def nbest_opt(lm, flag):
    opts = _lib.BeamOpts(flag)
    return lambda: this.e2e_ctc_beam_nbest_opt(*nbest_args(lm), C.byref(opts))


def measure(legs):
    res = {k: [] for k in legs}
    for k, f in legs.items():
        assert f() == 0, (k, this.e2e_last_error())
    torch.cuda.synchronize()
    for _ in range(ROUNDS):
        for k, f in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(CALLS):
                f()
            e1.record(); torch.cuda.synchronize()
            res[k].append(e0.elapsed_time(e1) / CALLS)
    return {k: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3)} for k, v in res.items()}


def wall(f, n=3):
    ts = []
    for _ in range(n):
        t0 = time.perf_counter(); h = f(); ts.append(time.perf_counter() - t0)
        this.e2e_lm_free(h)
    return round(statistics.median(ts) * 1e3, 1)


record = {"shape": "B=64 T=1500 V=29 beam=100 f32 log-probabilities, synthetic 3-gram", "rounds": ROUNDS, "calls_per_round": CALLS}
with tempfile.TemporaryDirectory() as td:
    path = os.path.join(td, "synthetic_3gram.arpa")
    bench.synthetic_arpa(path, labels)
    record["load_ms"] = wall(lambda: load_lm(this, path))
    record["load_with_lexicon_ms"] = wall(lambda: load_lm(this, path, True))
    lm_plain, lm_lex = load_lm(this, path), load_lm(this, path, True)
    lm_parent = load_lm(parent, path) if parent is not None else None
    legs = {}
    if parent is not None:
        legs["beam_parent"] = plain(parent, lm_parent)
        legs["nbest1_parent"] = nbest_parent(lm_parent)
    legs["beam"] = plain(this, lm_plain)
    legs["nbest1_flag_off"] = nbest_opt(lm_plain, 0)
    legs["beam_lexicon_tables"] = plain(this, lm_lex)
    legs["nbest1_flag_off_lexicon_tables"] = nbest_opt(lm_lex, 0)
    legs["nbest1_restricted"] = nbest_opt(lm_lex, 1)
    r = measure(legs)
    base = {"beam": "beam_parent", "nbest1_flag_off": "nbest1_parent", "beam_lexicon_tables": "beam_parent",
            "nbest1_flag_off_lexicon_tables": "nbest1_parent", "nbest1_restricted": "nbest1_flag_off_lexicon_tables"}
    for k, v in r.items():
        b = base.get(k)
        if b in r:
            v["ratio"], v["ratio_to"] = round(v["median_ms"] / r[b]["median_ms"], 4), b
        print("%-32s median %8.3f ms  min %8.3f ms  %s" % (k, v["median_ms"], v["min_ms"],
                                                            "x%.4f of %s" % (v["ratio"], b) if "ratio" in v else ""))
    record["timing"] = r
    # how much the restriction leaves of the search: words and length of the results
    nbest_opt(lm_lex, 0)(); torch.cuda.synchronize(); record["mean_length_unrestricted"] = float(out_len.double().mean())
    nbest_opt(lm_lex, 1)(); torch.cuda.synchronize(); record["mean_length_restricted"] = float(out_len.double().mean())
    record["mean_oov_restricted"] = float(counts[:, 0, 1].double().mean())
    for h in (lm_plain, lm_lex):
        this.e2e_lm_free(h)
    if lm_parent is not None:
        parent.e2e_lm_free(lm_parent)
print({k: v for k, v in record.items() if k != "timing"})
if os.environ.get("LEXICON_JSON"):
    with open(os.environ["LEXICON_JSON"], "w") as f:
        json.dump(record, f, indent=1)
