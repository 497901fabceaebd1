"""What custom transcriptions cost at BASELINE configs[3] (B=64, T=1500, V=29, beam 100, the synthetic 3-gram): HIP events, two
builds of libe2e_ctc.so in ONE process, interleaved rounds, median of 7 rounds of 3 calls:
    python3 tools/diag/time_beam_transcriptions.py [build/diag/ab_parent.so]
(a) the plain LM call (e2e_ctc_beam) and the restricted call (e2e_ctc_beam_nbest_opt, nbest = 1) on the UNTRANSCRIBED model of
    this tree against the parent commit's build (the argument: the parent's library, built from a checkout of that commit with
    its Makefile); the parent is timed twice per round, so the same run gives the parent-against-itself spread;
(b) the identity-lexicon model (every word transcribed by its own letters) against the plain model, both calls;
(c) a model in which 10 % of the transcriptions carry 2 to 4 homophones against (b).
TRANSCRIPTIONS_JSON=path: also write the numbers there (profiles/transcriptions/)."""
import ctypes as C, json, os, random, statistics, sys, tempfile
root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))
import torch
import bench
import lexicon_ref as LR
from end2end_amd import _lib

ROUNDS, CALLS = 7, 3
B, T, V, W = 64, 1500, 29, 100
this = _lib.load()
parent = None
if len(sys.argv) > 1:
    parent = C.CDLL(os.path.join(root, sys.argv[1]))
    for name in ("e2e_ctc_beam", "e2e_ctc_beam_nbest_opt", "e2e_lm_load_arpa", "e2e_lm_enable_lexicon", "e2e_lm_free"):
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
LABEL_ARR = (C.c_char_p * V)(*[s.encode() for s in labels])


def load_lm(L, path):
    h = C.c_void_p()
    assert L.e2e_lm_load_arpa(path.encode(), LABEL_ARR, V, 1, C.byref(h)) == 0
    assert L.e2e_lm_enable_lexicon(h) == 0, L.e2e_last_error()
    return h


def load_transcribed(path, entries):
    """entries: [(word, letters)] -> a model of this build keyed by them, with its lexicon."""
    flat, off = [], [0]
    for _, letters in entries:
        flat += [labels.index(c) for c in letters]
        off.append(len(flat))
    h = C.c_void_p()
    rc = this.e2e_lm_load_transcriptions(path.encode(), (C.c_char_p * len(entries))(*[w.encode() for w, _ in entries]),
                                         (C.c_int32 * len(flat))(*flat), (C.c_int32 * len(off))(*off), len(entries), LABEL_ARR, V, 1,
                                         C.byref(h))
    assert rc == 0, this.e2e_last_error()
    assert this.e2e_lm_transcriptions_dropped(h) == 0
    assert this.e2e_lm_enable_lexicon(h) == 0, this.e2e_last_error()
    return h


def plain(L, lm):
    return lambda: L.e2e_ctc_beam(x.data_ptr(), _lib.F32, *x.stride(), xl.data_ptr(), B, T, V, 0, W, 27, lm, *ARGS,
                                  out.data_ptr(), max_out, out_len.data_ptr(), ws.data_ptr(), ws.numel(), stream)


def restricted(L, lm):
    opts = _lib.BeamOpts(1)
    return lambda: L.e2e_ctc_beam_nbest_opt(x.data_ptr(), _lib.F32, *x.stride(), xl.data_ptr(), B, T, V, 0, W, 27, lm, *ARGS, 1,
                                            out.data_ptr(), max_out, out_len.data_ptr(), n_hyp.data_ptr(), scores.data_ptr(),
                                            counts.data_ptr(), None, ws.data_ptr(), ws.numel(), stream, C.byref(opts))


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


record = {"shape": "B=64 T=1500 V=29 beam=100 f32 log-probabilities, synthetic 3-gram", "rounds": ROUNDS, "calls_per_round": CALLS}
with tempfile.TemporaryDirectory() as td:
    path = os.path.join(td, "synthetic_3gram.arpa")
    bench.synthetic_arpa(path, labels)
    words = LR.arpa_words(path)
    identity = [(w, w) for w in words]
    # (c): every tenth word is also reachable by the letters of 1 to 3 other words -- those keys then hold 2 to 4 words
    rnd = random.Random(5)
    homophones = list(identity)
    shared = 0
    for w in words[::10]:
        for other in rnd.sample(words, rnd.randint(1, 3)):
            if other != w:
                homophones.append((other, w))
        shared += 1
    record["words"], record["keys_with_homophones"] = len(words), shared
    lm_plain, lm_id, lm_hom = load_lm(this, path), load_transcribed(path, identity), load_transcribed(path, homophones)
    legs = {}
    if parent is not None:
        lm_parent = load_lm(parent, path)
        legs["beam_parent"] = plain(parent, lm_parent)
        legs["restricted_parent"] = restricted(parent, lm_parent)
        legs["beam_parent_again"] = plain(parent, lm_parent)
        legs["restricted_parent_again"] = restricted(parent, lm_parent)
    legs["beam"] = plain(this, lm_plain)
    legs["restricted"] = restricted(this, lm_plain)
    legs["beam_identity"] = plain(this, lm_id)
    legs["restricted_identity"] = restricted(this, lm_id)
    legs["beam_homophones"] = plain(this, lm_hom)
    legs["restricted_homophones"] = restricted(this, lm_hom)
    r = measure(legs)
    base = {"beam_parent_again": "beam_parent", "restricted_parent_again": "restricted_parent", "beam": "beam_parent",
            "restricted": "restricted_parent", "beam_identity": "beam", "restricted_identity": "restricted",
            "beam_homophones": "beam_identity", "restricted_homophones": "restricted_identity"}
    for k, v in r.items():
        b = base.get(k)
        if b in r:
            v["ratio"], v["ratio_to"] = round(v["median_ms"] / r[b]["median_ms"], 4), b
        print("%-28s median %8.3f ms  min %8.3f ms  %s" % (k, v["median_ms"], v["min_ms"],
                                                        "x%.4f of %s" % (v["ratio"], b) if "ratio" in v else ""))
    record["timing"] = r
    # the identity lexicon decodes what the plain model decodes
    plain(this, lm_plain)(); torch.cuda.synchronize(); want = (out.clone(), out_len.clone())
    plain(this, lm_id)(); torch.cuda.synchronize()
    record["identity_same_result"] = bool(torch.equal(out_len, want[1]) and torch.equal(out, want[0]))
    for h in (lm_plain, lm_id, lm_hom):
        this.e2e_lm_free(h)
    if parent is not None:
        parent.e2e_lm_free(lm_parent)
print({k: v for k, v in record.items() if k != "timing"})
if os.environ.get("TRANSCRIPTIONS_JSON"):
    with open(os.environ["TRANSCRIPTIONS_JSON"], "w") as f:
        json.dump(record, f, indent=1)
