"""Time the streaming ASG beam search at B=64, T=1000, V=29 (27 characters + 2 repeat labels), beam 100 and 16, without a model
and with bench.py's synthetic 3-gram of 10k words (asg_beam_time.py's), f32, HIP events, two builds of libe2e_ctc.so in ONE
process, interleaved rounds, medians:
    python3 tools/diag/asg_beam_stream_time.py [build/diag/ab_parent.so]
(a) e2e_asg_beam_nbest of this tree against the parent commit's build (the argument, built with tools/diag/build_variant.sh or
    copied from a parent checkout; this tree's when none is given), and the parent against itself: two legs of the same build,
    the run-to-run spread the first comparison has to sit in;
(b) the utterances fed to e2e_asg_beam_stream in ten chunks of 100 frames, the ten calls summed -- fed only (nbest = 0) with
    one read-out at the end, and with the best hypothesis read out after every chunk (nbest = 1) -- against ONE whole call of
    the parent's build over the same input (nbest = 1).
ASG_STREAM_JSON=path: also write the numbers there (profiles/asg_stream/)."""
import ctypes as C, json, os, statistics, sys, tempfile
root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, root)
import torch
import bench
from end2end_amd import _lib

ROUNDS, CALLS = 7, 3
B, T, V, R, CHUNK = 64, 1000, 29, 2, 100
WIDTHS = (100, 16)
this = _lib.load()
parent = None
if len(sys.argv) > 1:
    parent = C.CDLL(os.path.join(root, sys.argv[1]))
    for name in ("e2e_asg_beam_nbest", "e2e_asg_beam_workspace_bytes", "e2e_lm_load_arpa", "e2e_lm_free"):
        getattr(parent, name).restype = getattr(this, name).restype
        getattr(parent, name).argtypes = getattr(this, name).argtypes
d = torch.device("cuda", 0)
asg_labels = [" "] + [chr(97 + i) for i in range(26)] + ["<1>", "<2>"]
ctc_labels = ["_"] + [chr(97 + i) for i in range(26)] + [" ", "'"]      # (the alphabet bench.py spells its 3-gram's words in)
g = torch.Generator().manual_seed(2)
x = (torch.randn(B, T, V, generator=g) * 3).to(d)
A = torch.randn(V, V, generator=g).to(d)
xl = torch.full((B,), T, dtype=torch.long, device=d)
cl = torch.full((B,), CHUNK, dtype=torch.long, device=d)
out = torch.empty((B, 1, T), dtype=torch.long, device=d)
out_len = torch.empty((B, 1), dtype=torch.long, device=d)
n_hyp = torch.empty(B, dtype=torch.long, device=d)
done = torch.empty(B, dtype=torch.long, device=d)
scores = torch.empty((B, 1, 3), dtype=torch.float64, device=d)
counts = torch.empty((B, 1, 2), dtype=torch.int32, device=d)
stream = _lib.stream_ptr(d)
HEADER = 256
KNOBS = (1.0, 1.0, -10.0)


def load_lm(L, path):
    h = C.c_void_p()
    arr = (C.c_char_p * V)(*[s.encode() for s in asg_labels])
    assert L.e2e_lm_load_arpa(path.encode(), arr, V, 1, C.byref(h)) == 0
    return h


def whole(L, W, lm):
    ws = torch.empty(L.e2e_asg_beam_workspace_bytes(B, T, V, W, 1), dtype=torch.uint8, device=d)
    return lambda: L.e2e_asg_beam_nbest(x.data_ptr(), _lib.F32, *x.stride(), A.data_ptr(), xl.data_ptr(), B, T, V, R, W, 0, lm,
                                        *KNOBS, 1, out.data_ptr(), T, out_len.data_ptr(), n_hyp.data_ptr(), scores.data_ptr(),
                                        counts.data_ptr(), ws.data_ptr(), ws.numel(), stream)


def chunked(W, lm, every):
    """All T frames through the stream in chunks of CHUNK; every: read out after every chunk, else after the last only."""
    row = this.e2e_asg_beam_stream_row_bytes(T, V, W, 1 if lm else 0)
    state = torch.empty((B, row), dtype=torch.uint8, device=d)
    ws = torch.empty(this.e2e_asg_beam_stream_workspace_bytes(B, V, W, 1 if lm else 0), dtype=torch.uint8, device=d)

    def run():
        state[:, :HEADER].zero_()                                  # (a new batch of utterances: part of what is timed)
        rc = 0
        for a in range(0, T, CHUNK):
            c = x[:, a:a + CHUNK]
            n = 1 if every or a + CHUNK >= T else 0
            rc |= this.e2e_asg_beam_stream(c.data_ptr(), _lib.F32, *c.stride(), A.data_ptr(), cl.data_ptr(), B, c.shape[1], V, R, W,
                                           0, lm, *KNOBS, state.data_ptr(), row, T, n, out.data_ptr(), T, out_len.data_ptr(),
                                           n_hyp.data_ptr(), scores.data_ptr(), counts.data_ptr(), done.data_ptr(),
                                           ws.data_ptr(), ws.numel(), stream, None)
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


record = {"shape": "B=64 T=1000 V=29 (2 repeat labels) f32 emissions, nbest=1, chunks of %d frames" % CHUNK, "rounds": ROUNDS,
          "calls_per_round": CALLS}
with tempfile.TemporaryDirectory() as td:
    path = os.path.join(td, "synthetic_3gram.arpa")
    bench.synthetic_arpa(path, ctc_labels)
    for W in WIDTHS:
        for mode in ("no_lm", "lm"):
            lm_this = load_lm(this, path) if mode == "lm" else None
            lm_parent = load_lm(parent, path) if mode == "lm" and parent is not None else None
            base_lib, base_lm = (parent, lm_parent) if parent is not None else (this, lm_this)
            legs = {"whole_parent_a": whole(base_lib, W, base_lm), "whole": whole(this, W, lm_this),
                    "whole_parent_b": whole(base_lib, W, base_lm),
                    "stream_fed_only_read_out_at_the_end": chunked(W, lm_this, False),
                    "stream_read_out_every_chunk": chunked(W, lm_this, True)}
            r = measure(legs)
            # the streamed result is the whole call's
            whole(this, W, lm_this)(); torch.cuda.synchronize()
            want = [t.clone() for t in (out, out_len, n_hyp, scores, counts)]
            chunked(W, lm_this, False)(); torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip((out, out_len, n_hyp, scores, counts), want)) and done.tolist() == [T] * B
            base = r["whole_parent_a"]["median_ms"]
            for k, v in r.items():
                v["ratio"] = round(v["median_ms"] / base, 4)
                print("beam %3d %-6s %-36s median %8.3f ms  min %8.3f  max %8.3f  x%.4f" % (W, mode, k, v["median_ms"], v["min_ms"],
                                                                                         v["max_ms"], v["ratio"]), flush=True)
            record["beam_%d_%s" % (W, mode)] = r
            if lm_this is not None:
                this.e2e_lm_free(lm_this)
            if lm_parent is not None:
                parent.e2e_lm_free(lm_parent)
record["ratio_to"] = "whole_parent_a (the parent commit's e2e_asg_beam_nbest)" if parent is not None else "whole_parent_a (this tree: no parent build given)"
if os.environ.get("ASG_STREAM_JSON"):
    os.makedirs(os.path.dirname(os.path.abspath(os.environ["ASG_STREAM_JSON"])), exist_ok=True)
    with open(os.environ["ASG_STREAM_JSON"], "w") as f:
        json.dump(record, f, indent=1)
