"""Time the streaming beam search at BASELINE configs[3] (B=64, T=1500, V=29, beam 100; without the LM and with the synthetic
3-gram), HIP events, two builds of libe2e_ctc.so in ONE process, interleaved rounds, median:
    python3 tools/diag/time_beam_stream.py [build/diag/ab_parent.so]
(a) the utterances fed to e2e_ctc_beam_stream in chunks of 100 frames, the 15 calls summed -- with the best hypothesis read out
    after every chunk (nbest = 1), and fed only (nbest = 0) with one read-out at the end -- against ONE e2e_ctc_beam call of the
    parent commit's build over the same input (the argument: the parent's library; this tree's when none is given);
(b) e2e_ctc_beam of this tree against the parent's, and the parent against itself (two legs of the same build: the run-to-run
    spread the first comparison has to sit in).
STREAM_JSON=path: also write the numbers there (profiles/stream/)."""
import ctypes as C, json, os, statistics, sys, tempfile
root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, root)
import torch
import bench
from end2end_amd import _lib

ROUNDS, CALLS = 7, 3
B, T, V, W, CHUNK = 64, 1500, 29, 100, 100
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
cl = torch.full((B,), CHUNK, dtype=torch.long, device=d)
max_out = T + 1
out = torch.empty((B, max_out), dtype=torch.long, device=d)
out_len = torch.empty((B,), dtype=torch.long, device=d)
n_hyp = torch.empty(B, dtype=torch.long, device=d)
done = torch.empty(B, dtype=torch.long, device=d)
scores = torch.empty((B, 1, 3), dtype=torch.float64, device=d)
counts = torch.empty((B, 1, 2), dtype=torch.int32, device=d)
ws = torch.empty(this.e2e_ctc_beam_workspace_bytes_lm(B, T, V, W, 1), dtype=torch.uint8, device=d)
stream = _lib.stream_ptr(d)
HEADER = 256


def load_lm(L, path):
    h = C.c_void_p()
    arr = (C.c_char_p * V)(*[s.encode() for s in labels])
    assert L.e2e_lm_load_arpa(path.encode(), arr, V, 1, C.byref(h)) == 0
    return h


def plain(L, lm):
    args = (1.0, 1.0, -10.0) if lm else (0.0, 1.0, -10.0)
    return lambda: L.e2e_ctc_beam(x.data_ptr(), _lib.F32, *x.stride(), xl.data_ptr(), B, T, V, 0, W, 27, lm, *args,
                                  out.data_ptr(), max_out, out_len.data_ptr(), ws.data_ptr(), ws.numel(), stream)


def chunked(lm, every):
    """All T frames through the stream in chunks of CHUNK; every: read out after every chunk, else after the last only."""
    args = (1.0, 1.0, -10.0) if lm else (0.0, 1.0, -10.0)
    row = this.e2e_ctc_beam_stream_row_bytes(T, V, W, 1 if lm else 0, 0)
    state = torch.empty((B, row), dtype=torch.uint8, device=d)

    def run():
        state[:, :HEADER].zero_()                                  # (a new batch of utterances: part of what is timed)
        rc = 0
        for a in range(0, T, CHUNK):
            c = x[:, a:a + CHUNK]
            n = 1 if every or a + CHUNK >= T else 0
            rc |= this.e2e_ctc_beam_stream(c.data_ptr(), _lib.F32, *c.stride(), cl.data_ptr(), B, c.shape[1], V, 0, W, 27, lm,
                                           *args, state.data_ptr(), row, T, 0, n, out.data_ptr(), max_out, out_len.data_ptr(),
                                           n_hyp.data_ptr(), scores.data_ptr(), counts.data_ptr(), None, done.data_ptr(),
                                           None, 0, stream, None)
        return rc
    return run


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
    return {k: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)} for k, v in res.items()}


record = {"shape": "B=64 T=1500 V=29 beam=100 f32 log-probabilities, chunks of %d frames" % CHUNK, "rounds": ROUNDS,
          "calls_per_round": CALLS}
with tempfile.TemporaryDirectory() as td:
    path = os.path.join(td, "synthetic_3gram.arpa")
    bench.synthetic_arpa(path, labels)
    for mode in ("no_lm", "lm"):
        lm_this = load_lm(this, path) if mode == "lm" else None
        lm_parent = load_lm(parent, path) if mode == "lm" and parent is not None else None
        base_lib, base_lm = (parent, lm_parent) if parent is not None else (this, lm_this)
        legs = {"beam_parent_a": plain(base_lib, base_lm), "beam": plain(this, lm_this), "beam_parent_b": plain(base_lib, base_lm),
                "stream_read_out_every_chunk": chunked(lm_this, True), "stream_read_out_at_the_end": chunked(lm_this, False)}
        r = measure(legs)
        # the streamed result is the whole call's
        plain(this, lm_this)(); torch.cuda.synchronize()
        want_ids, want_len = out.clone(), out_len.clone()
        chunked(lm_this, False)(); torch.cuda.synchronize()
        assert torch.equal(out, want_ids) and torch.equal(out_len, want_len) and done.tolist() == [T] * B
        base = r["beam_parent_a"]["median_ms"]
        for k, v in r.items():
            v["ratio"] = round(v["median_ms"] / base, 4)
            print("%-6s %-28s median %8.3f ms  min %8.3f  max %8.3f  x%.4f" % (mode, k, v["median_ms"], v["min_ms"], v["max_ms"], v["ratio"]))
        record[mode] = r
        if lm_this is not None:
            this.e2e_lm_free(lm_this)
        if lm_parent is not None:
            parent.e2e_lm_free(lm_parent)
record["ratio_to"] = "beam_parent_a (the parent commit's e2e_ctc_beam)" if parent is not None else "beam_parent_a (this tree: no parent build given)"
if os.environ.get("STREAM_JSON"):
    os.makedirs(os.path.dirname(os.environ["STREAM_JSON"]), exist_ok=True)
    with open(os.environ["STREAM_JSON"], "w") as f:
        json.dump(record, f, indent=1)
