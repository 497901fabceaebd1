"""Time the n-best read-out at BASELINE configs[3] (B=64, T=1500, V=29, beam 100; without the LM and with the synthetic 3-gram),
HIP events, two builds of libe2e_ctc.so in ONE process, interleaved rounds, median:
    python3 tools/diag/time_beam_nbest.py [build/diag/ab_parent.so]
(a) e2e_ctc_beam of this tree against the parent commit's build (the argument: the parent's ctc_beam.hip compiled as
    tools/diag/build_variant.sh compiles a variant and linked with this tree's other objects);
(b) e2e_ctc_beam_nbest at nbest = 1, 10, 100, with and without timestamps, as a ratio to the parent's e2e_ctc_beam (to this
    tree's when no parent build is given).
NBEST_JSON=path: also write the numbers there (profiles/nbest/)."""
import ctypes as C, json, os, statistics, sys, tempfile
root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, root)
import torch
import bench
from end2end_amd import _lib

ROUNDS, CALLS = 7, 3
B, T, V, W = 64, 1500, 29, 100
this = _lib.load()
parent = None
if len(sys.argv) > 1:
    parent = C.CDLL(os.path.join(root, sys.argv[1]))
    for name in ("e2e_ctc_beam", "e2e_ctc_beam_workspace_bytes_lm", "e2e_lm_load_arpa", "e2e_lm_free"):
        getattr(parent, name).restype = getattr(this, name).restype
        getattr(parent, name).argtypes = getattr(this, name).argtypes
d = torch.device("cuda", 0)
labels = ["_"] + [chr(97 + i) for i in range(26)] + [" ", "'"]
g = torch.Generator().manual_seed(2)
x = torch.log_softmax(torch.randn(B, T, V, generator=g) * 3, -1).to(d)
xl = torch.full((B,), T, dtype=torch.long, device=d)
max_out = T + 1
out = torch.empty((B, W, max_out), dtype=torch.long, device=d)
ts = torch.empty((B, W, max_out), dtype=torch.long, device=d)
out_len = torch.empty((B, W), dtype=torch.long, device=d)
n_hyp = torch.empty(B, dtype=torch.long, device=d)
scores = torch.empty((B, W, 3), dtype=torch.float64, device=d)
counts = torch.empty((B, W, 2), dtype=torch.int32, device=d)
ws = torch.empty(this.e2e_ctc_beam_nbest_workspace_bytes(B, T, V, W, 1, 1), dtype=torch.uint8, device=d)
stream = _lib.stream_ptr(d)


def load_lm(L, path):
    h = C.c_void_p()
    arr = (C.c_char_p * V)(*[s.encode() for s in labels])
    assert L.e2e_lm_load_arpa(path.encode(), arr, V, 1, C.byref(h)) == 0
    return h


def plain(L, lm):
    args = (1.0, 1.0, -10.0) if lm else (0.0, 1.0, -10.0)
    return lambda: L.e2e_ctc_beam(x.data_ptr(), _lib.F32, *x.stride(), xl.data_ptr(), B, T, V, 0, W, 27, lm, *args,
                                  out.data_ptr(), max_out, out_len.data_ptr(), ws.data_ptr(), ws.numel(), stream)


def nbest(lm, n, with_ts):
    args = (1.0, 1.0, -10.0) if lm else (0.0, 1.0, -10.0)
    return lambda: this.e2e_ctc_beam_nbest(x.data_ptr(), _lib.F32, *x.stride(), xl.data_ptr(), B, T, V, 0, W, 27, lm, *args, n,
                                           out.data_ptr(), max_out, out_len.data_ptr(), n_hyp.data_ptr(), scores.data_ptr(),
                                           counts.data_ptr(), ts.data_ptr() if with_ts else None, ws.data_ptr(), ws.numel(), stream)


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


record = {"shape": "B=64 T=1500 V=29 beam=100 f32 log-probabilities", "rounds": ROUNDS, "calls_per_round": CALLS}
with tempfile.TemporaryDirectory() as td:
    path = os.path.join(td, "synthetic_3gram.arpa")
    bench.synthetic_arpa(path, labels)
    for mode in ("no_lm", "lm"):
        lm_this = load_lm(this, path) if mode == "lm" else None
        lm_parent = load_lm(parent, path) if mode == "lm" and parent is not None else None
        legs = {"beam": plain(this, lm_this)}
        if parent is not None:
            legs["beam_parent"] = plain(parent, lm_parent)
        for n in (1, 10, 100):
            for with_ts in (False, True):
                legs["nbest%d%s" % (n, "_timesteps" if with_ts else "")] = nbest(lm_this, n, with_ts)
        r = measure(legs)
        base = r["beam_parent" if parent is not None else "beam"]["median_ms"]
        for k, v in r.items():
            v["ratio"] = round(v["median_ms"] / base, 4)
            print("%-6s %-20s median %8.3f ms  min %8.3f ms  x%.4f" % (mode, k, v["median_ms"], v["min_ms"], v["ratio"]))
        record[mode] = r
        if lm_this is not None:
            this.e2e_lm_free(lm_this)
        if lm_parent is not None:
            parent.e2e_lm_free(lm_parent)
record["ratio_to"] = "beam_parent" if parent is not None else "beam"
if os.environ.get("NBEST_JSON"):
    with open(os.environ["NBEST_JSON"], "w") as f:
        json.dump(record, f, indent=1)
