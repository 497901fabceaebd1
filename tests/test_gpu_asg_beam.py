"""GPU: the ASG beam search (e2e_asg_beam_nbest; ASGDecoder.configure(beam_width > 1)) against brute-force enumeration, the
plain-Python restatement (tests/asg_beam_ref.py), the ASG loss of the same inputs and the best path.  Scores are compared to
1e-9 * max(1, |score|) (f64 cells against Python floats: the Gram-CTC tests' tolerance); sequences, counts and orders
exactly.  The fixed-seed pruned cases keep every cut 1e-7 apart (tests/test_asg_beam_cpu.py), far above f64 evaluation order."""
import math
import os

import numpy as np
import pytest
import torch

import asg_beam_ref as REF
import asg_beam_util as U

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
DTYPES = {"f32": torch.float32, "f64": torch.float64}
TOL = 1e-9
LETTERS = [" "] + [chr(97 + i) for i in range(26)]           # the pruned cases' 27 characters, the space at 0


def close(got, want, tol=TOL):
    return abs(got - want) <= tol * max(1.0, abs(want))


def decoder(W, chars=None, R=0, **kw):
    from end2end_amd import ASGDecoder
    time_major = kw.pop("time_major", False)
    return ASGDecoder(labels=chars, num_replabels=R, time_major=time_major).configure(beam_width=W, **kw)


def hyps(res, b):
    """The hypotheses of utterance b as the reference lists them."""
    n = int(res.num_hypotheses[b])
    out = []
    for k in range(n):
        m = int(res.decoded_targets_lengths[b, k])
        out.append(dict(ids=tuple(res.decoded_targets[b, k, :m].tolist()), total=float(res.scores[b, k]),
                        ac=float(res.ctc_scores[b, k]), lm=float(res.lm_scores[b, k]), words=int(res.num_words[b, k]),
                        oov=int(res.num_oov_words[b, k])))
        assert not res.decoded_targets[b, k, m:].any()                  # zero filled behind the sequence
    N = res.scores.shape[1]
    assert (res.decoded_targets_lengths[b, n:] == 0).all() and (res.scores[b, n:] == -math.inf).all()
    assert n == N or (res.ctc_scores[b, n:] == -math.inf).all()
    return out


def check_ranking(got, want):
    assert [h["ids"] for h in got] == [h["ids"] for h in want]
    for g, w in zip(got, want):
        assert close(g["total"], w["total"]) and close(g["ac"], w["ac"]) and close(g["lm"], w["lm"]), (g, w)
        assert g["words"] == w["words"] and g["oov"] == w["oov"], (g, w)


def fcc(x, A, n):
    """log of the summed scores of all paths of n frames: the dense recurrence in f64 on the CPU."""
    x, A = x.double(), A.double()
    alpha = x[0]
    for t in range(1, n):
        alpha = torch.logsumexp(alpha[None, :] + A, dim=1) + x[t]
    return float(torch.logsumexp(alpha, 0))


def asg_losses(x, A, n, seqs):
    """ASGLoss(y) of every y in seqs on the first n frames of x (T,V), from the existing engine, in f64."""
    from end2end_amd.engines import ASGLossEngine
    H, S = len(seqs), max(len(s) for s in seqs)
    tg = torch.zeros((H, S), dtype=torch.long)
    for i, s in enumerate(seqs):
        tg[i, :len(s)] = torch.tensor(s)
    xs = x.double().to(DEV)[None].expand(H, -1, -1).contiguous()
    out = ASGLossEngine().compute(xs, A.double().to(DEV), tg.to(DEV), torch.full((H,), n, dtype=torch.long, device=DEV),
                                  torch.tensor([len(s) for s in seqs], device=DEV))
    return out[0].double().cpu().tolist()


# ---- 1. unpruned equals enumeration --------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("i", range(len(U.TINY_GRID)))
def test_unpruned_equals_enumeration(i, dt):
    V, T, R, space = U.TINY_GRID[i]
    x, A, lens, enum = U.tiny_case(i)
    want = U.tiny_unbounded(i)
    chars = ["a", " ", "b"] if space >= 0 else None
    xt, At = torch.from_numpy(x).to(DTYPES[dt]), torch.from_numpy(A).to(DTYPES[dt])
    res = decoder(128, chars, R, wip=0.0).decode_nbest(xt.to(DEV), At.to(DEV), torch.tensor(lens))
    assert res.timesteps is None
    for b in range(3):
        got = hyps(res, b)
        assert {h["ids"] for h in got} == set(enum[b])                  # every sequence is present
        for h in got:
            assert close(h["ac"], enum[b][h["ids"]]), (b, h)
            assert h["total"] == h["ac"] and h["lm"] == 0.0 and h["oov"] == 0
        assert [h["ids"] for h in got] == [h["ids"] for h in want[b]]   # the order matches
        if R == 0:
            n = lens[b]
            z = fcc(xt[b], At, n)
            acs = torch.tensor([h["ac"] for h in got], dtype=torch.float64)
            assert close(float(torch.logsumexp(acs, 0)), z)
            seqs = [h["ids"] for h in got if len(h["ids"]) <= n]
            assert len(seqs) == len(got)
            for h, loss in zip(got, asg_losses(xt[b], At, n, seqs)):
                assert close(h["ac"], z - loss), (b, h, z, loss)
            from end2end_amd.engines import ASGViterbiEngine
            _, vs, coll, cl = ASGViterbiEngine().compute(xt[b:b + 1].to(DEV), At.to(DEV), torch.tensor([n]))
            best = tuple(coll[0, :int(cl[0])].tolist())
            assert [h for h in got if h["ids"] == best][0]["ac"] >= float(vs[0])


def test_unpruned_order_with_repeat_labels():
    """The R > 0 grid cases, ranked as the restatement ranks them under the same word penalty."""
    for i in (4, 5):
        V, T, R, space = U.TINY_GRID[i]
        x, A, lens, _ = U.tiny_case(i)
        chars = ["a", " ", "b"] if space >= 0 else None
        want = REF.beam(x.tolist(), A.tolist(), lens, V, R, space, W=None, wip=0.25)[0]
        res = decoder(128, chars, R, wip=0.25).decode_nbest(torch.from_numpy(x).to(DEV), torch.from_numpy(A).to(DEV), torch.tensor(lens))
        for b in range(3):
            check_ranking(hyps(res, b), want[b])


# ---- 2. pruned equals the restatement ------------------------------------------------------------------------------
def views(x, layout):
    """x (B,T,V) on the GPU as a time-major view, or as a batch-major view that is not contiguous."""
    if layout == "time_major":
        return x.transpose(0, 1).contiguous(), dict(time_major=True)
    B, T, V = x.shape
    buf = torch.full((B, T + 3, 2 * V + 1), 7.0, dtype=x.dtype, device=x.device)
    v = buf[:, 2:2 + T, 1:1 + 2 * V:2]
    v.copy_(x)
    assert not v.is_contiguous()
    return v, {}


@pytest.mark.parametrize("layout,dt", [("time_major", "f32"), ("strided", "f64")])
@pytest.mark.parametrize("W", U.PRUNED_WIDTHS)
def test_pruned_equals_restatement(W, layout, dt):
    x, A = U.pruned_case()
    want, gap = U.pruned_ref(W)
    assert gap >= U.MIN_GAP
    xt, At = torch.from_numpy(x).to(DTYPES[dt]), torch.from_numpy(A).to(DTYPES[dt])
    xv, kw = views(xt.to(DEV), layout)
    if W == 1:
        # (ASGDecoder's width 1 is the best-path decoder: the search itself is reached through its engine)
        from end2end_amd.decoders.ctc_decoder import NBestResults
        from end2end_amd.engines import ASGBeamEngine
        eng = ASGBeamEngine(LETTERS, U.PRUNED_R, 1)
        res = NBestResults(*eng.decode_nbest(xv.transpose(0, 1) if kw else xv, At.to(DEV), torch.tensor(U.PRUNED_LENS)))
    else:
        res = decoder(W, LETTERS, U.PRUNED_R, wip=0.0, **kw).decode_nbest(xv, At.to(DEV), torch.tensor(U.PRUNED_LENS))
    for b in range(3):
        got = hyps(res, b)
        check_ranking(got, want[b])
        n = U.PRUNED_LENS[b]
        z = fcc(xt[b], At, n)
        for h, loss in zip(got, asg_losses(xt[b], At, n, [h["ids"] for h in got])):
            assert h["ac"] <= z - loss + 1e-7, (b, h, z, loss)         # pruning only loses mass
        assert res.decoded_sentences[b][0] == REF.expand(got[0]["ids"], LETTERS)


def test_pruned_wide_alphabet():
    x, A = U.wide_case()
    want, gap = U.wide_ref()
    assert gap >= U.MIN_GAP
    res = decoder(U.WIDE_W, wip=0.0).decode_nbest(torch.from_numpy(x).to(DEV), torch.from_numpy(A).to(DEV), torch.tensor(U.WIDE_LENS))
    for b in range(3):
        check_ranking(hyps(res, b), want[b])


# ---- 3. with a language model --------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_sensitive", [True, False])
@pytest.mark.parametrize("W", U.LM_WIDTHS)
@pytest.mark.parametrize("model", sorted(U.LM_MODELS))
def test_lm_equals_restatement(model, W, case_sensitive):
    chars = U.LM_MODELS[model]["chars"] if case_sensitive else U.upper_chars(U.LM_MODELS[model]["chars"])
    x, A = U.lm_case(model)
    want, gap = U.lm_ref(model, W, case_sensitive)
    assert gap >= U.MIN_GAP
    d = decoder(W, chars, U.LM_R, lm_path=os.path.join(U.GOLDEN, model), case_sensitive=case_sensitive, **U.LM_KNOBS)
    res = d.decode_nbest(torch.from_numpy(x).to(DEV), torch.from_numpy(A).to(DEV), torch.tensor(U.LM_LENS))
    for b in range(3):
        got = hyps(res, b)
        check_ranking(got, want[b])
        assert res.decoded_sentences[b] == [REF.expand(h["ids"], chars) for h in got]
    best = d.decode(torch.from_numpy(x).to(DEV), torch.from_numpy(A).to(DEV), torch.tensor(U.LM_LENS))
    assert best.decoded_sentences == [s[0] for s in res.decoded_sentences]
    assert best.decoded_targets_lengths.tolist() == res.decoded_targets_lengths[:, 0].tolist()


def test_lm_known_answer():
    """Near-one-hot emissions along the encoding of "add bed" (a d <1> _ b e d): the doubled letter is looked up expanded."""
    from end2end_amd.engines import LanguageModel
    chars = U.LM_MODELS["lm_order4.arpa"]["chars"]
    path = os.path.join(U.GOLDEN, "lm_order4.arpa")
    V = len(chars) + 1
    ids = [chars.index("a"), chars.index("d"), V - 1, chars.index(" "), chars.index("b"), chars.index("e"), chars.index("d")]
    x = torch.full((1, 2 * len(ids), V), -20.0)
    for k, c in enumerate(ids):
        x[0, 2 * k: 2 * k + 2, c] = 0.0
    d = decoder(7, chars, 1, lm_path=path, lmwt=0.8, wip=0.3, oov_penalty=-2.0)
    res = d.decode_nbest(x.to(DEV), None)
    assert res.decoded_sentences[0][0] == "add bed"
    assert res.decoded_targets[0, 0, :int(res.decoded_targets_lengths[0, 0])].tolist() == ids
    assert int(res.num_words[0, 0]) == 2 and int(res.num_oov_words[0, 0]) == 0
    lm = LanguageModel(path, chars + ["<1>"], True)
    bos, add, bed = lm.word_index("<s>"), lm.word_index("add"), lm.word_index("bed")
    assert add != 0 and bed != 0
    ln10 = math.log(10.0)
    chain = (0.0 + lm.score([bos], add) / ln10) + lm.score([add, bos], bed) / ln10
    # (the same two divisions and one addition in f64: a few ulp at most)
    assert abs(float(res.lm_scores[0, 0]) - chain) <= 1e-12
    assert close(float(res.scores[0, 0]), float(res.ctc_scores[0, 0]) + 0.8 * chain - 0.3 * 2)
    assert d.decode(x.to(DEV), None).decoded_sentences == ["add bed"]


# ---- 4. transitions=None -------------------------------------------------------------------------------------------
def test_no_transitions_is_a_zero_matrix():
    x, _ = U.pruned_case()
    xt = torch.from_numpy(x).to(DEV)
    d = decoder(16, LETTERS, 2)
    a = d.decode_nbest(xt, None, torch.tensor(U.PRUNED_LENS))
    z = d.decode_nbest(xt, torch.zeros(29, 29, device=DEV), torch.tensor(U.PRUNED_LENS))
    for f in ("decoded_targets", "decoded_targets_lengths", "scores", "ctc_scores", "lm_scores", "num_words", "num_hypotheses"):
        assert torch.equal(getattr(a, f), getattr(z, f)), f
    assert a.decoded_sentences == z.decoded_sentences
    # a CTC-without-blank model: log-softmax in, R = 0; unpruned, the scores are the labellings' log-probabilities
    V, T, _, _ = U.TINY_GRID[1]
    lp = torch.log_softmax(torch.from_numpy(U.tiny_case(1)[0]).double(), -1)
    res = decoder(128, wip=0.0).decode_nbest(lp.to(DEV), None)
    for b in range(3):
        got = hyps(res, b)
        assert len(got) == 93
        assert abs(math.fsum(math.exp(h["ac"]) for h in got) - 1.0) <= 1e-9


# ---- 5. ties and determinism ---------------------------------------------------------------------------------------
def test_ties_and_determinism():
    x = torch.full((2, 6, 5), 0.5, device=DEV)
    A = torch.full((5, 5), 0.25, device=DEV)
    d = decoder(8, wip=0.0)
    a, b = d.decode_nbest(x, A), d.decode_nbest(x, A)
    for f in ("decoded_targets", "decoded_targets_lengths", "scores", "ctc_scores", "num_hypotheses"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    assert a.num_hypotheses.tolist() == [8, 8]
    for u in range(2):
        got = hyps(a, u)
        keys = [(-h["total"], REF.key_of(h["ids"])) for h in got]
        assert keys == sorted(keys) and len({h["ids"] for h in got}) == 8
    # a single frame with more labels than places: the equal totals are cut by key
    V, W = 12, 5
    res = decoder(W, wip=0.0).decode_nbest(torch.full((1, 1, V), -0.75, device=DEV), None)
    want = sorted(((c,) for c in range(V)), key=REF.key_of)[:W]
    assert [h["ids"] for h in hyps(res, 0)] == want
    assert res.scores[0].tolist() == [-0.75] * W


# ---- 6. edges ------------------------------------------------------------------------------------------------------
def test_lengths_outside_the_range():
    x, A = U.pruned_case()
    T = U.PRUNED_T
    x5 = torch.from_numpy(np.concatenate([x, x[:2]])).to(DEV)
    At = torch.from_numpy(A).to(DEV)
    d = decoder(7, LETTERS, 2)
    res = d.decode_nbest(x5, At, torch.tensor([T, 0, 31, T + 1, 23]))
    ref = d.decode_nbest(x5[[0, 2, 4]], At, torch.tensor([T, 31, 23]))
    assert res.num_hypotheses.tolist() == [7, 0, 7, 0, 7]
    assert res.decoded_sentences[1] == [] and res.decoded_sentences[3] == []
    for f in ("decoded_targets", "decoded_targets_lengths", "scores", "ctc_scores", "num_words"):
        assert torch.equal(getattr(res, f)[[0, 2, 4]], getattr(ref, f)), f
    assert (res.decoded_targets_lengths[[1, 3]] == 0).all() and (res.scores[[1, 3]] == -math.inf).all()


def test_nbest_is_the_head_of_the_list():
    x, A = U.pruned_case()
    xt, At, xl = torch.from_numpy(x).to(DEV), torch.from_numpy(A).to(DEV), torch.tensor(U.PRUNED_LENS)
    d = decoder(32, LETTERS, 2)
    full, head = d.decode_nbest(xt, At, xl), d.decode_nbest(xt, At, xl, nbest=5)
    w = head.decoded_targets.shape[2]
    assert torch.equal(full.decoded_targets[:, :5, :w], head.decoded_targets) and not full.decoded_targets[:, :5, w:].any()
    for f in ("decoded_targets_lengths", "scores", "ctc_scores", "lm_scores", "num_words", "num_oov_words"):
        assert torch.equal(getattr(full, f)[:, :5], getattr(head, f)), f
    assert head.num_hypotheses.tolist() == [5, 5, 5]
    assert [s[:5] for s in full.decoded_sentences] == head.decoded_sentences
    one = d.decode(xt, At, xl)
    assert one.decoded_sentences == [s[0] for s in full.decoded_sentences]
    with pytest.raises(ValueError):
        d.decode_nbest(xt, At, xl, nbest=33)


def raw_call(x, A, xl, R, W, space, nbest, max_out):
    from end2end_amd import _runtime as RT
    from end2end_amd._runtime import _C
    B, T, V = x.shape
    out = torch.full((B, nbest, max(max_out, 1)), -7, dtype=torch.long, device=DEV)
    out_len = torch.full((B, nbest), -7, dtype=torch.long, device=DEV)
    n_hyp = torch.full((B,), -7, dtype=torch.long, device=DEV)
    scores = torch.full((B, nbest, 3), 7.0, dtype=torch.float64, device=DEV)
    counts = torch.full((B, nbest, 2), -7, dtype=torch.int32, device=DEV)
    ws = torch.empty(_C.asg_beam_workspace_bytes(B, T, V, W, False), dtype=torch.uint8, device=DEV)
    sB, sT, sV = x.stride()
    xl = xl.to(DEV)
    _C.asg_beam_nbest(x.data_ptr(), RT.dtype_code(x.dtype), sB, sT, sV, A.data_ptr() if A is not None else 0, xl.data_ptr(),
                      B, T, V, R, W, space, 0, 1.0, 0.0, 0.0, nbest, out.data_ptr(), max_out, out_len.data_ptr(),
                      n_hyp.data_ptr(), scores.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel(),
                      RT.stream_handle(DEV))
    torch.cuda.synchronize()
    return out.cpu(), out_len.cpu(), n_hyp.cpu(), scores.cpu(), counts.cpu()


def test_max_out_too_small_reports_the_length():
    x, A = U.pruned_case()
    xt, At, xl = torch.from_numpy(x).to(DEV), torch.from_numpy(A).to(DEV), torch.tensor(U.PRUNED_LENS)
    full = raw_call(xt, At, xl, 2, 7, 0, 7, U.PRUNED_T)
    short = raw_call(xt, At, xl, 2, 7, 0, 7, 2)
    assert int(full[1].min()) > 2 and torch.equal(full[1], short[1])    # the needed lengths, beyond max_out
    assert torch.equal(full[0][:, :, :2], short[0]) and torch.equal(full[3], short[3]) and torch.equal(full[2], short[2])
    # an utterance the call does not touch keeps what the buffers held
    odd = raw_call(xt, At, torch.tensor([40, 41, 0]), 2, 7, 0, 3, U.PRUNED_T)
    assert odd[2].tolist() == [3, 0, 0]
    assert (odd[1][1:] == -7).all() and (odd[0][1:] == -7).all() and (odd[3][1:] == 7.0).all() and (odd[4][1:] == -7).all()
    assert torch.equal(odd[0][0], full[0][0, :3])


def test_more_utterances_than_any_table():
    g = torch.Generator().manual_seed(3)
    base = torch.randn(7, 10, 29, generator=g)
    A = torch.randn(29, 29, generator=g).to(DEV)
    lens = torch.tensor([10, 9, 10, 4, 1, 7, 10])
    d = decoder(16, LETTERS, 2)
    ref = d.decode_nbest(base.to(DEV), A, lens)
    res = d.decode_nbest(base.repeat(10, 1, 1).to(DEV), A, lens.repeat(10))
    assert res.scores.shape[0] == 70
    for f in ("decoded_targets", "decoded_targets_lengths", "scores", "ctc_scores", "num_words", "num_hypotheses"):
        got, want = getattr(res, f), getattr(ref, f)
        assert torch.equal(got, want.repeat(*([10] + [1] * (want.dim() - 1)))), f


def test_empty_batch_and_limits():
    d = decoder(4, LETTERS, 2)
    res = d.decode_nbest(torch.zeros((0, 5, 29), device=DEV), None)
    assert res.decoded_targets.shape[:2] == (0, 4) and res.decoded_sentences == [] and res.num_hypotheses.numel() == 0
    from end2end_amd._runtime import _C
    assert _C.asg_beam_max_width(29) == 128
    with pytest.raises(ValueError):
        decoder(_C.asg_beam_max_width(29) + 1, LETTERS, 2)
    with pytest.raises(ValueError):
        decoder(4).decode_nbest(torch.zeros((1, 5, 129), device=DEV), None)
    with pytest.raises(Exception, match="exceeds e2e_asg_beam_max_width"):
        raw_call(torch.zeros((1, 5, 29), device=DEV), None, torch.tensor([5]), 2, 129, 0, 1, 5)
    with pytest.raises(Exception, match="e2e_asg_max_labels"):
        raw_call(torch.zeros((1, 5, 129), device=DEV), None, torch.tensor([5]), 0, 4, -1, 1, 5)


# ---- 7. beam_width = 1 is unchanged --------------------------------------------------------------------------------
def test_width_one_is_the_best_path_decoder():
    from end2end_amd import ASGDecoder
    x, A = U.pruned_case()
    xt, At, xl = torch.from_numpy(x).to(DEV), torch.from_numpy(A).to(DEV), torch.tensor(U.PRUNED_LENS)
    old = ASGDecoder(labels=LETTERS, num_replabels=2)
    new = ASGDecoder(labels=LETTERS, num_replabels=2).configure(beam_width=1, lmwt=0.5, wip=0.25, oov_penalty=-3, case_sensitive=False)
    a, b = old.decode(xt, At, xl), new.decode(xt, At, xl)
    assert torch.equal(a.decoded_targets, b.decoded_targets) and torch.equal(a.decoded_targets_lengths, b.decoded_targets_lengths)
    assert a.decoded_sentences == b.decoded_sentences
    pa, pb = old.decode_path(xt, At, xl), new.decode_path(xt, At, xl)
    assert torch.equal(pa.paths, pb.paths) and torch.equal(pa.scores, pb.scores)
