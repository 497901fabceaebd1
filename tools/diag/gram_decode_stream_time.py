"""Time the streaming Gram-CTC beam search at B=64, T=1000, f32 log-probabilities (gram_decode_lm_time.py's inputs: ragged
lengths T/2 .. T): the loss's headline table (R=29, 300 bigrams, 50 trigrams, V=379) at widths 100 and 16 and unigrams only
(V=29) at width 100, each without a model (e2e_gram_ctc_beam_nbest; the stream with scored = 0) and with bench.py's synthetic
3-gram of 10k words (e2e_gram_ctc_beam_nbest_lm; scored = 1).  HIP events, two builds of libe2e_ctc.so in ONE process,
interleaved rounds, medians:
    python3 tools/diag/gram_decode_stream_time.py [build/diag/ab_parent.so]
(a) the whole call of this tree against the parent commit's build (the argument, built with tools/diag/build_variant.sh or
    from a parent checkout's ctc_gram_decode.hip; this tree's when none is given), and the parent against itself: two legs of
    the same build, the run-to-run spread the first comparison has to sit in;
(b) the utterances fed to e2e_gram_ctc_beam_stream in ten chunks of 100 frames, the ten calls summed -- fed only (nbest = 0)
    with one read-out at the end, and with the best hypothesis read out after every chunk (nbest = 1) -- against ONE whole call
    of the parent's build over the same input (nbest = 1).
GRAM_STREAM_OUT=dir: also write gram_stream_time.json / .txt there (profiles/gram_stream/).  GRAM_STREAM_ROUNDS: rounds (5)."""
import ctypes as C, json, os, statistics, sys, tempfile
root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, root)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch
import bench
from end2end_amd import _lib
from end2end_amd.engines import GramCTCDecoderEngine
from gram_time import table

ROUNDS, CALLS = int(os.environ.get("GRAM_STREAM_ROUNDS", "5")), 1
B, T, CHUNK = 64, 1000, 100
this = _lib.load()
parent = None
if len(sys.argv) > 1:
    parent = C.CDLL(os.path.join(root, sys.argv[1]))
    for name in ("e2e_gram_ctc_beam_nbest", "e2e_gram_ctc_beam_nbest_lm", "e2e_gram_beam_workspace_bytes_lm", "e2e_lm_load_arpa",
                 "e2e_lm_free"):
        getattr(parent, name).restype = getattr(this, name).restype
        getattr(parent, name).argtypes = getattr(this, name).argtypes
d = torch.device("cuda", 0)
labels = ["_"] + [chr(97 + i) for i in range(26)] + [" ", "'"]          # (the alphabet bench.py spells its 3-gram's words in)
NB, SPACE = len(labels), labels.index(" ")
stream = _lib.stream_ptr(d)
HEADER = 256
KNOBS = (1.0, 1.0, -10.0)


def load_lm(L, path):
    h = C.c_void_p()
    arr = (C.c_char_p * NB)(*[s.encode() for s in labels])
    assert L.e2e_lm_load_arpa(path.encode(), arr, NB, 1, C.byref(h)) == 0
    return h


class Case:
    def __init__(self, grams, V, W):
        g = torch.Generator().manual_seed(7)
        self.V, self.W = V, W
        self.lp = torch.log_softmax(torch.randn(B, T, V, generator=g), -1).to(d)
        xl = torch.randint(T // 2, T + 1, (B,), generator=g)
        xl[0] = T
        self.xl = xl.to(d)
        self.cl = [(xl - a).clamp(0, CHUNK).to(d) for a in range(0, T, CHUNK)]
        self.eng = GramCTCDecoderEngine(0, NB, V, grams, W)
        self.ids, self.lens = self.eng._table(d)
        self.K = self.eng.max_order
        self.max_out = T * self.K
        self.out = torch.empty((B, 1, self.max_out), dtype=torch.long, device=d)
        self.out_len = torch.empty((B, 1), dtype=torch.long, device=d)
        self.n_hyp = torch.empty(B, dtype=torch.long, device=d)
        self.done = torch.empty(B, dtype=torch.long, device=d)
        self.scores = torch.empty((B, 1, 3), dtype=torch.float64, device=d)
        self.counts = torch.empty((B, 1, 2), dtype=torch.int32, device=d)

    def outputs(self):
        return (self.out, self.out_len, self.n_hyp, self.scores, self.counts)

    def whole(self, L, lm):
        c = self
        ws = torch.empty(L.e2e_gram_beam_workspace_bytes_lm(B, T, c.V, c.K, c.W, 1), dtype=torch.uint8, device=d)
        head = (c.lp.data_ptr(), _lib.F32, *c.lp.stride(), c.xl.data_ptr(), B, T, c.V, c.ids.data_ptr(), c.lens.data_ptr(), c.K)
        tail = (1, c.out.data_ptr(), c.max_out, c.out_len.data_ptr(), c.n_hyp.data_ptr(), c.scores.data_ptr())
        if lm is None:
            return lambda: L.e2e_gram_ctc_beam_nbest(*head, c.W, *tail, ws.data_ptr(), ws.numel(), stream)
        return lambda: L.e2e_gram_ctc_beam_nbest_lm(*head, NB, c.W, SPACE, lm, *KNOBS, *tail, c.counts.data_ptr(), ws.data_ptr(),
                                                    ws.numel(), stream)

    def chunked(self, lm, every):
        """All T frames through the stream in chunks of CHUNK; every: read out after every chunk, else after the last only."""
        c = self
        scored = 1 if lm is not None else 0
        row = this.e2e_gram_beam_stream_row_bytes(T, c.V, c.K, c.W, scored, scored)
        state = torch.empty((B, row), dtype=torch.uint8, device=d)
        ws = torch.empty(this.e2e_gram_beam_stream_workspace_bytes(B, c.V, c.K, c.W, scored, scored), dtype=torch.uint8, device=d)

        def run():
            state[:, :HEADER].zero_()                                  # (a new batch of utterances: part of what is timed)
            rc = 0
            for i, a in enumerate(range(0, T, CHUNK)):
                x = c.lp[:, a:a + CHUNK]
                n = 1 if every or a + CHUNK >= T else 0
                rc |= this.e2e_gram_ctc_beam_stream(x.data_ptr(), _lib.F32, *x.stride(), c.cl[i].data_ptr(), B, x.shape[1], c.V,
                                                    c.ids.data_ptr(), c.lens.data_ptr(), c.K, NB, c.W, scored, SPACE, lm, *KNOBS,
                                                    state.data_ptr(), row, T, n, c.out.data_ptr(), c.max_out, c.out_len.data_ptr(),
                                                    c.n_hyp.data_ptr(), c.scores.data_ptr(), c.counts.data_ptr() if scored else None,
                                                    c.done.data_ptr(), ws.data_ptr(), ws.numel(), stream, None)
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


record = {"shape": "B=64 T=1000 (lengths T/2 .. T) f32 log-probabilities, nbest=1, chunks of %d frames" % CHUNK, "rounds": ROUNDS,
          "calls_per_round": CALLS, "device": torch.cuda.get_device_name(0)}
lines = []
with tempfile.TemporaryDirectory() as td:
    path = os.path.join(td, "synthetic_3gram.arpa")
    bench.synthetic_arpa(path, labels)
    l2i, V379 = table(np.random.default_rng(7), NB, {2: 300, 3: 50})
    for grams, V, W in ((l2i, V379, 100), (l2i, V379, 16), ({}, NB, 100)):
        case = Case(grams, V, W)
        for mode in ("no_lm", "lm"):
            lm_this = load_lm(this, path) if mode == "lm" else None
            lm_parent = load_lm(parent, path) if mode == "lm" and parent is not None else None
            base_lib, base_lm = (parent, lm_parent) if parent is not None else (this, lm_this)
            legs = {"whole_parent_a": case.whole(base_lib, base_lm), "whole": case.whole(this, lm_this),
                    "whole_parent_b": case.whole(base_lib, base_lm),
                    "stream_fed_only_read_out_at_the_end": case.chunked(lm_this, False),
                    "stream_read_out_every_chunk": case.chunked(lm_this, True)}
            r = measure(legs)
            # the streamed result is the whole call's
            case.whole(this, lm_this)(); torch.cuda.synchronize()
            keep = case.outputs() if mode == "lm" else case.outputs()[:3]
            want = [t.clone() for t in keep]
            want_scores = case.scores.clone()
            case.chunked(lm_this, False)(); torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(keep, want)) and case.done.tolist() == case.xl.tolist()
            assert torch.equal(case.scores.view(-1)[:B if mode == "no_lm" else 3 * B], want_scores.view(-1)[:B if mode == "no_lm" else 3 * B])
            base = r["whole_parent_a"]["median_ms"]
            for k, v in r.items():
                v["ratio"] = round(v["median_ms"] / base, 4)
                lines.append("V=%3d beam %3d %-6s %-36s median %8.3f ms  min %8.3f  max %8.3f  x%.4f" % (
                    V, W, mode, k, v["median_ms"], v["min_ms"], v["max_ms"], v["ratio"]))
                print(lines[-1], flush=True)
            record["V_%d_beam_%d_%s" % (V, W, mode)] = r
            if lm_this is not None:
                this.e2e_lm_free(lm_this)
            if lm_parent is not None:
                parent.e2e_lm_free(lm_parent)
record["ratio_to"] = ("whole_parent_a (the parent commit's whole call)" if parent is not None
                      else "whole_parent_a (this tree: no parent build given)")
if os.environ.get("GRAM_STREAM_OUT"):
    os.makedirs(os.environ["GRAM_STREAM_OUT"], exist_ok=True)
    with open(os.path.join(os.environ["GRAM_STREAM_OUT"], "gram_stream_time.json"), "w") as f:
        json.dump(record, f, indent=1)
    with open(os.path.join(os.environ["GRAM_STREAM_OUT"], "gram_stream_time.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
