"""What per-frame label pruning (cutoff_top_n, cutoff_prob) costs and saves: HIP events, medians, every leg in ONE process
(separate processes differ by 2-4 % for one binary), interleaved rounds.
    python3 tools/diag/label_cut_time.py [build/diag/parent.so]
(the argument: the parent commit's library, for the unpruned calls -- they must not have changed; it is timed twice per round,
so the same run gives the parent-against-itself spread).
  a. the selection alone (e2e_ctc_label_cut, cutoff_top_n 40, cutoff_prob 0.99): time, and the read of lp it achieves as a
     fraction of HBM_PEAK, at B=16 T=256 V=8000 f32 and at B=64 T=1500 V=29;
  b. B=16 T=256 V=8000 W=100 without a model: unpruned (parent, this tree) against cutoff_top_n = 40;
  c. the same shape with a model -- a synthetic word-piece transcription lexicon over bench.py's synthetic 3-gram, every word
     spelled by 1 to 3 of the 7998 pieces: unpruned (parent, this tree) against cutoff_top_n = 40;
  d. C4 (B=64 T=1500 V=29 W=100, the synthetic 3-gram spelled by letters): unpruned, the one-workgroup kernel, against
     cutoff_top_n = 10, which moves the call to the general kernel.
LABEL_CUT_JSON=path: also write the numbers there (profiles/label_cut/).  LABEL_CUT_LEGS=abcd: only these."""
import ctypes as C, json, os, random, statistics, sys, tempfile
root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))
import torch
import bench
import lexicon_ref as LR
from end2end_amd import _lib

HBM_PEAK = 8.0e12                       # bytes / s, the MI355X's nominal HBM3E bandwidth
LEGS = os.environ.get("LABEL_CUT_LEGS", "abcd")
this = _lib.load()
parent = None
if len(sys.argv) > 1:
    parent = C.CDLL(os.path.join(root, sys.argv[1]))
    for name in ("e2e_ctc_beam_nbest_opt", "e2e_ctc_beam_nbest_workspace_bytes", "e2e_lm_load_arpa", "e2e_lm_load_transcriptions",
                 "e2e_lm_free", "e2e_last_error"):
        getattr(parent, name).restype = getattr(this, name).restype
        getattr(parent, name).argtypes = getattr(this, name).argtypes
d = torch.device("cuda", 0)
stream = _lib.stream_ptr(d)
record = {"hbm_peak_bytes_per_s": HBM_PEAK}


def measure(legs, rounds, calls):
    res = {k: [] for k in legs}
    for k, f in legs.items():
        assert f() == 0, (k, this.e2e_last_error())
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, f in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                f()
            e1.record(); torch.cuda.synchronize()
            res[k].append(e0.elapsed_time(e1) / calls)
    return {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)} for k, v in res.items()}


def ratios(r, base):
    for k, b in base.items():
        if k in r and b in r:
            r[k]["ratio"], r[k]["ratio_to"] = round(r[k]["median_ms"] / r[b]["median_ms"], 4), b
    for k, v in r.items():
        print("  %-26s median %10.4f ms  min %10.4f  max %10.4f  %s" % (k, v["median_ms"], v["min_ms"], v["max_ms"],
                                                                   "x%.4f of %s" % (v["ratio"], v["ratio_to"]) if "ratio" in v else ""))
    return r


def logprobs(B, T, V, scale, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.log_softmax(torch.randn(B, T, V, generator=g) * scale, -1).to(d)


class Search:
    """The buffers of one shape and the calls on them (nbest = 1, no timesteps)."""

    def __init__(self, B, T, V, W, space_id):
        self.B, self.T, self.V, self.W, self.space_id = B, T, V, W, space_id
        self.x = logprobs(B, T, V, 3.0, 2)
        self.xl = torch.full((B,), T, dtype=torch.long, device=d)
        self.max_out = T + 1
        self.out = torch.empty((B, 1, self.max_out), dtype=torch.long, device=d)
        self.out_len = torch.empty((B, 1), dtype=torch.long, device=d)
        self.n_hyp = torch.empty(B, dtype=torch.long, device=d)
        self.scores = torch.empty((B, 1, 3), dtype=torch.float64, device=d)
        self.counts = torch.empty((B, 1, 2), dtype=torch.int32, device=d)
        self.ws = None

    def _ws(self, nbytes):
        if self.ws is None or self.ws.numel() < nbytes:
            self.ws = torch.empty(nbytes, dtype=torch.uint8, device=d)
        return self.ws

    def args(self, lm, knobs):
        x = self.x
        return (x.data_ptr(), _lib.F32, *x.stride(), self.xl.data_ptr(), self.B, self.T, self.V, 0, self.W, self.space_id, lm,
                *knobs, 1, self.out.data_ptr(), self.max_out, self.out_len.data_ptr(), self.n_hyp.data_ptr(),
                self.scores.data_ptr(), self.counts.data_ptr(), None)

    def unpruned(self, L, lm, knobs=(0.0, 0.0, 0.0)):
        ws = self._ws(max(L.e2e_ctc_beam_nbest_workspace_bytes(self.B, self.T, self.V, self.W, 1 if lm else 0, 0), 256))
        a = self.args(lm, knobs)
        return lambda: L.e2e_ctc_beam_nbest_opt(*a, ws.data_ptr(), ws.numel(), stream, None)

    def pruned(self, lm, top_n, prob, knobs=(0.0, 0.0, 0.0)):
        ws = self._ws(this.e2e_ctc_beam_cut_workspace_bytes(self.B, self.T, self.V, self.W, 1 if lm else 0, 0, top_n))
        a = self.args(lm, knobs)
        return lambda: this.e2e_ctc_beam_nbest_cut(*a, ws.data_ptr(), ws.numel(), stream, None, top_n, prob)


def label_array(labels):
    return (C.c_char_p * len(labels))(*[s.encode() for s in labels])


if "a" in LEGS:
    print("a. the selection alone, cutoff_top_n = 40, cutoff_prob = 0.99")
    record["selection"] = {}
    for B, T, V, calls in ((16, 256, 8000, 10), (64, 1500, 29, 10)):
        x = logprobs(B, T, V, 3.0, 1)
        xl = torch.full((B,), T, dtype=torch.long, device=d)
        K = min(40, V)
        ids = torch.empty((B, T, K + 1), dtype=torch.int32, device=d)
        n = torch.empty((B, T), dtype=torch.int32, device=d)
        f = lambda: this.e2e_ctc_label_cut(x.data_ptr(), _lib.F32, *x.stride(), xl.data_ptr(), B, T, V, 0, 40, 0.99,   # noqa: E731
                                           ids.data_ptr(), n.data_ptr(), None, 0, stream)
        r = ratios(measure({"label_cut": f}, 9, calls), {})["label_cut"]
        r["lp_bytes"] = B * T * V * 4
        r["read_bytes_per_s"] = round(r["lp_bytes"] / (r["median_ms"] * 1e-3))
        r["fraction_of_hbm_peak"] = round(r["read_bytes_per_s"] / HBM_PEAK, 4)
        r["mean_kept"] = round(float(n.float().mean()), 2)
        print("  B=%d T=%d V=%d: %.1f GB/s of lp, %.3f of the HBM peak, %.1f labels kept per frame"
              % (B, T, V, r["read_bytes_per_s"] / 1e9, r["fraction_of_hbm_peak"], r["mean_kept"]))
        record["selection"]["B%d_T%d_V%d" % (B, T, V)] = r
        del x, ids, n

if "b" in LEGS:
    print("b. B=16 T=256 V=8000 W=100, no model")
    s = Search(16, 256, 8000, 100, -1)
    legs = {}
    if parent is not None:
        legs["unpruned_parent"] = s.unpruned(parent, None)
        legs["unpruned_parent_again"] = s.unpruned(parent, None)
    legs["unpruned"] = s.unpruned(this, None)
    legs["top_n_40"] = s.pruned(None, 40, 1.0)
    legs["top_n_40_prob_0.99"] = s.pruned(None, 40, 0.99)
    record["wide_no_model"] = ratios(measure(legs, 7, 3), {"unpruned_parent_again": "unpruned_parent", "unpruned": "unpruned_parent",
                                                          "top_n_40": "unpruned", "top_n_40_prob_0.99": "unpruned"})
    del s

if "c" in LEGS:
    print("c. B=16 T=256 V=8000 W=100, word pieces transcribed over the synthetic 3-gram")
    V = 8000
    labels = ["_"] + ["p%d" % i for i in range(V - 2)] + [" "]
    letters = ["_"] + [chr(97 + i) for i in range(26)] + [" ", "'"]
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "synthetic_3gram.arpa")
        bench.synthetic_arpa(path, letters)
        words = LR.arpa_words(path)
        rnd = random.Random(7)
        flat, off = [], [0]
        for _ in words:
            flat += [rnd.randint(1, V - 2) for _ in range(rnd.randint(1, 3))]
            off.append(len(flat))
        arr = label_array(labels)

        def load(L):
            h = C.c_void_p()
            rc = L.e2e_lm_load_transcriptions(path.encode(), (C.c_char_p * len(words))(*[w.encode() for w in words]),
                                              (C.c_int32 * len(flat))(*flat), (C.c_int32 * len(off))(*off), len(words), arr, V, 1,
                                              C.byref(h))
            assert rc == 0, L.e2e_last_error()
            return h
        s = Search(16, 256, V, 100, V - 1)
        knobs = (1.0, 1.0, -10.0)
        lm_this = load(this)
        legs = {}
        if parent is not None:
            lm_parent = load(parent)
            legs["unpruned_parent"] = s.unpruned(parent, lm_parent, knobs)
            legs["unpruned_parent_again"] = s.unpruned(parent, lm_parent, knobs)
        legs["unpruned"] = s.unpruned(this, lm_this, knobs)
        legs["top_n_40"] = s.pruned(lm_this, 40, 1.0, knobs)
        legs["top_n_40_prob_0.99"] = s.pruned(lm_this, 40, 0.99, knobs)
        record["wide_with_model"] = ratios(measure(legs, 3, 1), {"unpruned_parent_again": "unpruned_parent", "unpruned": "unpruned_parent",
                                                                "top_n_40": "unpruned_parent" if parent is not None else "unpruned",
                                                                "top_n_40_prob_0.99": "unpruned"})
        record["wide_with_model"]["words"] = len(words)
        this.e2e_lm_free(lm_this)
        if parent is not None:
            parent.e2e_lm_free(lm_parent)
        del s

if "d" in LEGS:
    print("d. C4: B=64 T=1500 V=29 W=100, the synthetic 3-gram")
    letters = ["_"] + [chr(97 + i) for i in range(26)] + [" ", "'"]
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "synthetic_3gram.arpa")
        bench.synthetic_arpa(path, letters)
        arr = label_array(letters)

        def load(L):
            h = C.c_void_p()
            assert L.e2e_lm_load_arpa(path.encode(), arr, 29, 1, C.byref(h)) == 0, L.e2e_last_error()
            return h
        s = Search(64, 1500, 29, 100, 27)
        knobs = (1.0, 1.0, -10.0)
        lm_this = load(this)
        legs = {}
        if parent is not None:
            lm_parent = load(parent)
            legs["unpruned_parent"] = s.unpruned(parent, lm_parent, knobs)
            legs["unpruned_parent_again"] = s.unpruned(parent, lm_parent, knobs)
        legs["unpruned"] = s.unpruned(this, lm_this, knobs)
        legs["top_n_10"] = s.pruned(lm_this, 10, 1.0, knobs)
        record["c4"] = ratios(measure(legs, 7, 3), {"unpruned_parent_again": "unpruned_parent", "unpruned": "unpruned_parent",
                                                   "top_n_10": "unpruned"})
        this.e2e_lm_free(lm_this)
        if parent is not None:
            parent.e2e_lm_free(lm_parent)

if os.environ.get("LABEL_CUT_JSON"):
    with open(os.environ["LABEL_CUT_JSON"], "w") as f:
        json.dump(record, f, indent=1)
