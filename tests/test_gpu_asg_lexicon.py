"""GPU: the ASG beam search restricted to a vocabulary, and its label timestamps (e2e_asg_beam_nbest_opt;
ASGDecoder.restrict_to_vocabulary, decode_nbest(timesteps=True)) against enumeration over the admissible labellings, the
plain-Python restatement (tests/asg_lexicon_ref.py) and known answers.  The tolerances are tests/test_gpu_asg_beam.py's: every
rank identical, counts and timesteps exact, scores to 1e-9 * max(1, |score|).  The seeded cases keep every cut 1e-7 apart
(tests/test_asg_lexicon_cpu.py)."""
import ctypes
import math
import os

import pytest
import torch

import asg_beam_util as U
import asg_lexicon_ref as LR
import asg_lexicon_util as LU
from test_gpu_asg_beam import DEV, DTYPES, check_ranking, close, decoder, hyps, views
from test_gpu_asg_beam_fuzz import shaped

pytestmark = pytest.mark.gpu

FIELDS = ("decoded_targets", "decoded_targets_lengths", "scores", "ctc_scores", "lm_scores", "num_words", "num_oov_words",
          "num_hypotheses")


def restricted(W, chars, R, lexicon=None, **kw):
    return decoder(W, chars, R, **kw).restrict_to_vocabulary(lexicon=lexicon)


def check_timesteps(res, b, want):
    """timesteps of utterance b: the restatement's frames, -1 behind every sequence and in the empty slots."""
    ts = res.timesteps[b]
    assert ts.shape == res.decoded_targets[b].shape and ts.dtype == torch.long
    for k, h in enumerate(want):
        m = len(h["ids"])
        assert ts[k, :m].tolist() == list(h["frames"]), (b, k, ts[k, :m].tolist(), h["frames"])
        assert (ts[k, m:] == -1).all()
    assert (ts[len(want):] == -1).all()


def same(a, b):
    for f in FIELDS:
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    assert a.decoded_sentences == b.decoded_sentences


# ---- 1. unpruned equals enumeration over the admissible labellings -------------------------------------------------------
@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("i", range(len(LU.GRIDS)))
def test_unpruned_equals_filtered_enumeration(i, dt):
    g = LU.GRIDS[i]
    x, A, lens, enum, _ = LU.grid_case(i)
    want = LU.grid_unbounded(i)
    xt, At = torch.from_numpy(x).to(DTYPES[dt]), torch.from_numpy(A).to(DTYPES[dt])
    res = restricted(128, g["chars"], g["R"], lexicon=g["words"], wip=0.0).decode_nbest(xt.to(DEV), At.to(DEV), torch.tensor(lens),
                                                                                       timesteps=True)
    for b in range(3):
        got = hyps(res, b)
        assert {h["ids"] for h in got} == set(enum[b])                  # exactly the admissible labellings
        for h in got:
            assert close(h["ac"], enum[b][h["ids"]]), (b, h)
            assert h["total"] == h["ac"] and h["lm"] == 0.0
        check_ranking(got, want[b])
        check_timesteps(res, b, want[b])


# ---- 2. pruned equals the restatement ------------------------------------------------------------------------------------
def pruned_decoder(name, W, **kw):
    m = LU.P_MODELS[name]
    if m["model"]:
        return restricted(W, m["chars"], LU.P_R, lm_path=os.path.join(U.GOLDEN, m["model"]), case_sensitive=m["case_sensitive"],
                          **LU.P_KNOBS, **kw)
    return restricted(W, m["chars"], LU.P_R, lexicon=LU.P_WORDS, wip=LU.P_KNOBS["wip"], case_sensitive=m["case_sensitive"], **kw)


@pytest.mark.parametrize("layout,dt", [("time_major", "f32"), ("strided", "f64")])
@pytest.mark.parametrize("W", LU.P_WIDTHS)
@pytest.mark.parametrize("name", sorted(LU.P_MODELS))
def test_pruned_equals_restatement(name, W, layout, dt):
    x, A = LU.pruned_case()
    want, gap = LU.pruned_ref(name, W)
    assert gap >= LU.MIN_GAP
    xt, At = torch.from_numpy(x).to(DTYPES[dt]), torch.from_numpy(A).to(DTYPES[dt])
    xv, kw = views(xt.to(DEV), layout)
    res = pruned_decoder(name, W, **kw).decode_nbest(xv, At.to(DEV), torch.tensor(LU.P_LENS), timesteps=True)
    assert res.num_hypotheses.tolist() == [len(r) for r in want]
    chars = LU.P_MODELS[name]["chars"]
    for b in range(4):
        got = hyps(res, b)
        check_ranking(got, want[b])
        check_timesteps(res, b, want[b])
        assert res.decoded_sentences[b] == [LR.expand(h["ids"], chars) for h in got]
    best = pruned_decoder(name, W, **kw).decode(xv, At.to(DEV), torch.tensor(LU.P_LENS))
    assert best.decoded_sentences == [s[0] if s else "" for s in res.decoded_sentences]


def test_pruned_wide_alphabet():
    x, A, chars, words = LU.wide_case()
    want, gap = LU.wide_ref()
    assert gap >= LU.MIN_GAP
    res = restricted(LU.WIDE_W, chars, LU.WIDE_R, lexicon=words, wip=0.25).decode_nbest(
        torch.from_numpy(x).to(DEV), torch.from_numpy(A).to(DEV), torch.tensor(LU.WIDE_LENS), timesteps=True)
    for b in range(3):
        check_ranking(hyps(res, b), want[b])
        check_timesteps(res, b, want[b])


# ---- 3. known answers ----------------------------------------------------------------------------------------------------
KNOWN_CHARS = [" ", "a", "b", "c", "d", "e", "'"]


def add_bed_emissions():
    """Near-one-hot emissions along a d <1> _ b e d, two frames a label."""
    V = len(KNOWN_CHARS) + 1
    ids = [KNOWN_CHARS.index(c) if c != "<1>" else V - 1 for c in ["a", "d", "<1>", " ", "b", "e", "d"]]
    x = torch.full((1, 2 * len(ids), V), -20.0)
    for k, c in enumerate(ids):
        x[0, 2 * k: 2 * k + 2, c] = 0.0
    return x, ids


def test_known_answer_add_bed():
    x, ids = add_bed_emissions()
    V = x.shape[2]
    ad = (KNOWN_CHARS.index("a"), KNOWN_CHARS.index("d"), KNOWN_CHARS.index(" "))
    lex = LR.Lexicon(["add", "bed"])
    plain = decoder(20, KNOWN_CHARS, 1, wip=0.0).decode_nbest(x.to(DEV), None)
    assert not all(LR.admissible(h["ids"], V, 1, 0, KNOWN_CHARS, lex) for h in hyps(plain, 0))   # unrestricted, non-words are in the beam ...
    res = restricted(20, KNOWN_CHARS, 1, lexicon=["add", "bed"], wip=0.0).decode_nbest(x.to(DEV), None, timesteps=True)
    got = hyps(res, 0)
    assert res.decoded_sentences[0][0] == "add bed" and got[0]["ids"] == tuple(ids)
    ts = res.timesteps[0, 0, :len(ids)].tolist()                        # (label k is heard from frame 2 k; at -20 it enters earlier)
    assert ts[0] == 0 and all(p < q for p, q in zip(ts, ts[1:])) and all(k <= t <= 2 * k for k, t in enumerate(ts))
    assert got[0]["words"] == 2 and got[0]["oov"] == 0
    for h in got:                                                       # ... restricted, nothing inadmissible is
        assert h["ids"][:3] != ad and LR.admissible(h["ids"], V, 1, 0, KNOWN_CHARS, lex), h
    # against {ad, bed}: "add" is never formed -- a d <1> is no prefix of a word
    res = restricted(20, KNOWN_CHARS, 1, lexicon=["ad", "bed"], wip=0.0).decode_nbest(x.to(DEV), None)
    got = hyps(res, 0)
    assert got and all("add" not in s for s in res.decoded_sentences[0])
    assert all(h["ids"][:3] != (ad[0], ad[1], V - 1) for h in got)
    assert all(LR.admissible(h["ids"], V, 1, 0, KNOWN_CHARS, LR.Lexicon(["ad", "bed"])) for h in got)


def test_known_answer_no_hypothesis():
    """The only word begins with a label that is -inf at frame 0, and there is no space: nothing can be formed."""
    chars = ["a", "b", "c"]
    x = torch.randn(2, 6, 4, generator=torch.Generator().manual_seed(1))
    x[0, 0, 1] = -math.inf
    res = restricted(8, chars, 1, lexicon=["ba"]).decode_nbest(x.to(DEV), None, timesteps=True)
    assert int(res.num_hypotheses[0]) == 0
    assert res.decoded_sentences[0] == [] and (res.scores[0] == -math.inf).all() and (res.decoded_targets_lengths[0] == 0).all()
    assert (res.timesteps[0] == -1).all()
    assert int(res.num_hypotheses[1]) > 0 and all(s.startswith("b") for s in res.decoded_sentences[1])


# ---- 4. timesteps, exact without a reference -----------------------------------------------------------------------------
@pytest.mark.parametrize("W", [2, 100])
def test_timesteps_of_a_forced_path(W):
    T, V = 30, 29
    g = torch.Generator().manual_seed(7)
    path = []
    while len(path) < T:                                                # runs of 1 to 4 frames over the 27 characters
        c = int(torch.randint(0, 27, (1,), generator=g))
        if path and c == path[-1]:
            continue
        path += [c] * min(int(torch.randint(1, 5, (1,), generator=g)), T - len(path))
    x = torch.full((1, T, V), -math.inf)
    x[0, torch.arange(T), torch.tensor(path)] = 0.0
    starts = [t for t in range(T) if t == 0 or path[t] != path[t - 1]]
    merged = [path[t] for t in starts]
    d = decoder(W, LU.LETTERS, 2, wip=0.0)
    res = d.decode_nbest(x.to(DEV), None, timesteps=True)
    assert res.num_hypotheses.tolist() == [1]
    assert res.decoded_targets[0, 0].tolist() == merged and res.timesteps[0, 0].tolist() == starts
    assert (res.timesteps[0, 1:] == -1).all() and float(res.ctc_scores[0, 0]) == 0.0
    # behind a shorter sequence of the same batch: -1
    x2 = torch.cat([x, x])
    res2 = d.decode_nbest(x2.to(DEV), None, torch.tensor([T, starts[3]]), timesteps=True)
    assert res2.timesteps[1, 0].tolist() == starts[:3] + [-1] * (len(starts) - 3)
    assert res2.timesteps[0, 0].tolist() == starts


def test_timesteps_change_nothing_else():
    x, A = U.pruned_case()
    xt, At, xl = torch.from_numpy(x).to(DEV), torch.from_numpy(A).to(DEV), torch.tensor(U.PRUNED_LENS)
    d = decoder(32, LU.LETTERS, 2)
    a, b = d.decode_nbest(xt, At, xl), d.decode_nbest(xt, At, xl, timesteps=True)
    assert a.timesteps is None and b.timesteps.shape == b.decoded_targets.shape
    same(a, b)
    n = b.decoded_targets_lengths
    for u in range(3):
        for k in range(32):
            ts = b.timesteps[u, k, :int(n[u, k])].tolist()
            assert ts[0] == 0 and all(p < q for p, q in zip(ts, ts[1:])) and ts[-1] < U.PRUNED_LENS[u]
            assert (b.timesteps[u, k, int(n[u, k]):] == -1).all()


# ---- 5. the options of the C call ----------------------------------------------------------------------------------------
def raw(x, A, xl, R, W, space, lm, knobs, nbest, opts):
    """One call through the C ABI (ctypes): opts None -- e2e_asg_beam_nbest; "null" -- _opt with NULL; else an AsgBeamOpts."""
    from end2end_amd import _lib, _runtime as RT
    L = _lib.load()
    B, T, V = x.shape
    out = torch.full((B, nbest, T), -7, dtype=torch.long, device=DEV)
    out_len = torch.full((B, nbest), -7, dtype=torch.long, device=DEV)
    n_hyp = torch.full((B,), -7, dtype=torch.long, device=DEV)
    scores = torch.full((B, nbest, 3), 7.0, dtype=torch.float64, device=DEV)
    counts = torch.full((B, nbest, 2), -7, dtype=torch.int32, device=DEV)
    ws = torch.empty(L.e2e_asg_beam_workspace_bytes(B, T, V, W, 1), dtype=torch.uint8, device=DEV)
    xl = xl.to(DEV)
    sB, sT, sV = x.stride()
    args = [x.data_ptr(), RT.dtype_code(x.dtype), sB, sT, sV, A.data_ptr(), xl.data_ptr(), B, T, V, R, W, space, lm, knobs[0], knobs[1],
            knobs[2], nbest, out.data_ptr(), T, out_len.data_ptr(), n_hyp.data_ptr(), scores.data_ptr(), counts.data_ptr(),
            ws.data_ptr(), ws.numel(), RT.stream_handle(DEV)]
    if opts is None:
        rc = L.e2e_asg_beam_nbest(*args)
    else:
        rc = L.e2e_asg_beam_nbest_opt(*args, None if opts == "null" else ctypes.byref(opts))
    torch.cuda.synchronize()
    return rc, (out.cpu(), out_len.cpu(), n_hyp.cpu(), scores.cpu(), counts.cpu()), L.e2e_last_error()


def test_opts():
    from end2end_amd import _lib
    from end2end_amd.engines import LanguageModel
    model = "tiny_3gram.arpa"
    chars = U.LM_MODELS[model]["chars"]
    x, A = U.lm_case(model)
    xt, At, xl = torch.from_numpy(x).to(DEV), torch.from_numpy(A).to(DEV), torch.tensor(U.LM_LENS)
    labels = chars + ["<1>"]
    lm = LanguageModel(os.path.join(U.GOLDEN, model), labels, True)
    knobs = (0.7, 0.4, -1.3)
    call = lambda h, opts: raw(xt, At, xl, U.LM_R, 32, chars.index(" "), h, knobs, 32, opts)  # noqa: E731
    h = lm.on(DEV).handle
    rc, base, _ = call(h, None)
    assert rc == 0 and int(base[2].min()) > 0
    for opts in ("null", _lib.AsgBeamOpts(0, None)):                    # NULL and zeroed opts: the plain call, bit for bit
        rc, got, _ = call(h, opts)
        assert rc == 0 and all(torch.equal(g, w) for g, w in zip(got, base))
    # restrict_to_lexicon without a model, or with a model without a lexicon: E2E_ERR_ARG, nothing launched
    for handle, words in ((None, "needs a model"), (h, "has no lexicon")):
        rc, got, err = call(handle, _lib.AsgBeamOpts(1, None))
        assert rc == -1 and words.encode() in err
        assert (got[0] == -7).all() and (got[2] == -7).all() and (got[3] == 7.0).all()
    # the lexicon enabled, the search unrestricted: the same model without it
    lex = LanguageModel(os.path.join(U.GOLDEN, model), labels, True, lexicon=True)
    assert lex.has_lexicon() and not lm.has_lexicon()
    rc, got, _ = call(lex.on(DEV).handle, None)
    assert rc == 0 and all(torch.equal(g, w) for g, w in zip(got, base))
    # ... and restricted it is another search
    rc, got, _ = call(lex.on(DEV).handle, _lib.AsgBeamOpts(1, None))
    assert rc == 0 and not torch.equal(got[0], base[0])


def test_a_later_configure_drops_the_restriction():
    x, _ = add_bed_emissions()
    d = restricted(20, KNOWN_CHARS, 1, lexicon=["add", "bed"], wip=0.0)
    plain = decoder(20, KNOWN_CHARS, 1, wip=0.0).decode_nbest(x.to(DEV), None)
    assert not torch.equal(d.decode_nbest(x.to(DEV), None).scores, plain.scores)
    same(d.configure(beam_width=20, wip=0.0).decode_nbest(x.to(DEV), None), plain)


def test_a_lexicon_together_with_a_model_is_refused():
    from end2end_amd.decoders.ctc_decoder import CTCDecoderError
    d = decoder(4, U.LM_MODELS["tiny_3gram.arpa"]["chars"], 1, lm_path=os.path.join(U.GOLDEN, "tiny_3gram.arpa"))
    with pytest.raises(CTCDecoderError, match="exclude each other"):
        d.restrict_to_vocabulary(lexicon=["ab"])
    assert d.restrict_to_vocabulary() is d                              # ... the model's own words are the way


# ---- 6. fuzz -------------------------------------------------------------------------------------------------------------
def run(c):
    dt = DTYPES[c.dtype]
    xv = shaped(torch.from_numpy(c.x).to(dt), c.shape, DEV)
    A = None if c.no_A else torch.from_numpy(c.A).to(dt).to(DEV)
    lens = torch.tensor(c.lens)
    model = dict(lm_path=os.path.join(U.GOLDEN, c.model), lmwt=c.lmwt, oov_penalty=c.oov) if c.model else {}
    if c.W == 1:
        # (ASGDecoder's width 1 is the best-path decoder: the search itself is reached through its engine)
        from end2end_amd.decoders.ctc_decoder import NBestResults
        from end2end_amd.engines import ASGBeamEngine
        eng = ASGBeamEngine(c.chars, c.R, 1, model.get("lm_path", ""), c.lmwt, c.wip, c.oov, c.case_sensitive).restrict(c.words)
        return NBestResults(*eng.decode_nbest(xv.transpose(0, 1) if c.shape["time_major"] else xv, A, lens, nbest=c.nbest,
                                              timesteps=c.timesteps))
    d = restricted(c.W, c.chars, c.R, lexicon=c.words, wip=c.wip, case_sensitive=c.case_sensitive,
                   time_major=c.shape["time_major"], **model)
    return d.decode_nbest(xv, A, lens, nbest=c.nbest, timesteps=c.timesteps)


@pytest.mark.parametrize("seed", [s for s in range(LU.FUZZ_N) if s not in LU.LEFT_OUT])
def test_fuzz(seed):
    c = LU.draw(seed)
    want, gap, _, _ = LU.reference(seed)
    assert gap >= LU.MIN_GAP
    res = run(c)
    N = c.W if c.nbest is None else c.nbest
    B = len(c.lens)
    assert res.scores.shape == (B, N) and (res.timesteps is not None) == c.timesteps
    for b in range(B):
        got = hyps(res, b)
        head = want[b][:N]
        assert int(res.num_hypotheses[b]) == len(head), (b, int(res.num_hypotheses[b]), len(head))
        check_ranking(got, head)
        assert res.decoded_sentences[b] == [LR.expand(h["ids"], c.chars) for h in got]
        if c.timesteps:
            check_timesteps(res, b, head)
