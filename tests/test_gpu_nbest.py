"""-m gpu: the n-best read-out of the beam search (e2e_ctc_beam_nbest) against the plain call, the oracle's beam search and
the oracle's CTC likelihood.  Every number is f64 against f64: atol = 1e-9 throughout (nbest_util.ATOL)."""
import os

import numpy as np
import pytest
import torch

import golden_util as G  # noqa: F401  (the brute-force goldens, through nbest_util)
import gpu_util as U
import nbest_util as NB
import oracle_lib as O
from end2end_amd.engines import LanguageModel

pytestmark = pytest.mark.gpu
ARPA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tiny_3gram.arpa")
ATOL = NB.ATOL
LABELS7 = ["_", "a", "b", "c", " ", "d", "'"]
XLEN5 = [40, 33, 17, 40, 1]


def rand_lp(seed, B, T, V, sharp=2.0, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    return torch.log_softmax(torch.randn(B, T, V, generator=g, dtype=torch.float64) * sharp, -1).to(dtype)


def check_timesteps(r, x_len):
    """As many frames as ids, strictly increasing, inside the utterance; -1 behind the sentence and for an empty winner's -1."""
    B, N, _ = r["ids"].shape
    for b in range(B):
        for h in range(N):
            n = int(r["lens"][b, h])
            ids, ts = r["ids"][b, h], r["ts"][b, h]
            assert (ts[n:] == -1).all() and (ids[n:] == 0).all(), (b, h)
            if h >= r["n_hyp"][b]:
                assert n == 0
                continue
            if n == 1 and ids[0] == -1:
                assert ts[0] == -1, (b, h)
                continue
            assert (ids[:n] >= 0).all()
            assert (ts[:n] >= 0).all() and (ts[:n] < x_len[b]).all() and (np.diff(ts[:n]) > 0).all(), (b, h, ts[:n])


def check_list(lp, x_len, blank, W, labels, nbest=None, lm=None, olm=None, **kw):
    """Item 1 of the suite for one call: hypothesis 0 is the plain call's and the oracle's result, the list is ranked and its
    members are distinct, empty slots are empty, timestamps are well formed and asking for them changes nothing else."""
    B, T, _ = lp.shape
    xl = [T] * B if x_len is None else list(x_len)
    gpu_kw = {k: v for k, v in kw.items() if k != "case_sensitive"}
    N = W if nbest is None else nbest
    r = NB.c_abi_beam_nbest(lp, x_len, blank, W, labels, lm, nbest=N, timesteps=True, **gpu_kw)
    r0 = NB.c_abi_beam_nbest(lp, x_len, blank, W, labels, lm, nbest=N, timesteps=False, **gpu_kw)
    for k in ("ids", "lens", "n_hyp", "scores", "counts"):
        assert np.array_equal(r[k], r0[k]), k                 # (-inf == -inf; no NaN is ever written)
    ids, lens = U.c_abi_beam(lp, x_len, blank, W, labels, lm, **gpu_kw)
    o_ids, o_lens, _ = O.ctc_beam(lp.double().numpy(), x_len, blank, W, labels, olm, **kw)
    assert r["lens"][:, 0].tolist() == lens.tolist() == o_lens.tolist()
    width = ids.shape[1]
    assert np.array_equal(r["ids"][:, 0, :width], ids) and (r["ids"][:, 0, width:] == 0).all()      # the row, zero fill included
    assert ids.tolist() == o_ids.tolist()
    for b in range(B):
        nh = int(r["n_hyp"][b])
        tot = r["scores"][b, :nh, 0]
        assert not np.isnan(r["scores"][b]).any()
        assert (tot[:-1] >= tot[1:]).all(), (b, tot)
        hyps = [NB.hypothesis(r, b, h) for h in range(nh)]
        assert len(set(hyps)) == nh, (b, "hypotheses repeat")
        assert (r["lens"][b, nh:] == 0).all() and (r["ids"][b, nh:] == 0).all()
        assert np.isneginf(r["scores"][b, nh:, :2]).all() and (r["scores"][b, nh:, 2] == 0).all()
        assert (r["counts"][b, nh:] == 0).all()
        if lm is None:
            assert (r["scores"][b, :, 2] == 0).all() and (r["counts"][b, :, 1] == 0).all()
    check_timesteps(r, xl)
    return r


# ---- 1. hypothesis 0 is decode ----
@pytest.mark.parametrize("W", [2, 3, 10, 100])
@pytest.mark.parametrize("wip", [0.0, 1.0])
def test_hypothesis_0_is_decode_random(W, wip):
    lp = rand_lp(100 + W, 5, 40, 7)
    check_list(lp, XLEN5, 0, W, LABELS7, wip=wip)
    check_list(lp, XLEN5, 6, W, LABELS7[::-1], wip=wip)                 # blank last, space elsewhere
    check_list(lp.float(), None, 0, W, None, wip=wip)                   # f32 input, no labels
    check_list(lp.bfloat16(), XLEN5, 0, W, LABELS7, wip=wip)            # 16-bit input, read as it is


def test_hypothesis_0_is_decode_empty_winner_and_time_major_view():
    lp = torch.log(torch.tensor([[[0.98, 0.01, 0.01]] * 4], dtype=torch.float64))
    r = check_list(lp, None, 0, 10, None)
    assert r["ids"][0, 0, :2].tolist() == [-1, 0] and r["lens"][0, 0] == 1 and r["ts"][0, 0, 0] == -1     # quirk Q6
    x = rand_lp(11, 4, 30, 6)
    tm = x.permute(1, 0, 2).contiguous().permute(1, 0, 2)
    a = check_list(x, None, 0, 8, None)
    b = check_list(tm, None, 0, 8, None)
    for k in ("ids", "lens", "n_hyp", "scores", "counts", "ts"):
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("W", [4, 70])
def test_hypothesis_0_is_decode_under_massive_ties(W):
    labels = ["_", "a", "b", "c", "d", "e", "f", "g", "h", " "]
    V = len(labels)
    flat = torch.full((2, 9, V), float(np.log(1.0 / V)), dtype=torch.float64)
    check_list(flat, [9, 6], 0, W, labels, wip=0.0)
    two = torch.log(torch.tensor([0.3] + [0.7 / (V - 1)] * (V - 1), dtype=torch.float64)).repeat(2, 9, 1)
    check_list(two, [9, 7], 0, W, labels, wip=1.0)
    holes = flat.clone(); holes[:, :, 3] = float("-inf"); holes[:, ::2, 5] = float("-inf")
    check_list(holes, [9, 9], 0, W, labels, wip=0.0)


# ---- 2. exhaustive beams: exact likelihoods in exact order ----
@pytest.mark.parametrize("name", NB.EXHAUSTIVE_NAMES)
def test_exhaustive_beam_lists_every_labelling_by_likelihood(name):
    """A beam as wide as the number of labellings never prunes: every hypothesis's CTC score is the labelling's likelihood,
    and the list is the labellings sorted by it (order compared between neighbours more than 1e-6 apart)."""
    c = next(c for c in NB.exhaustive_cases() if c["name"] == name)
    W, blank = c["beam_width"], c["blank"]
    lp = torch.from_numpy(c["lp"])[None]
    r = NB.c_abi_beam_nbest(lp, None, blank, W, c["labels"], wip=0.0, nbest=W)
    assert r["n_hyp"][0] == W
    want = dict(zip(c["seqs"], c["ll"]))
    got = [NB.hypothesis(r, 0, h) for h in range(W)]
    assert sorted(got) == sorted(want)                                   # every labelling exactly once
    place = {}
    for h, seq in enumerate(got):
        tot, ctc = r["scores"][0, h, 0], r["scores"][0, h, 1]
        assert tot == ctc, (seq, tot, ctc)
        assert np.isfinite(ctc) == np.isfinite(want[seq]), seq
        if np.isfinite(ctc):
            assert abs(ctc - want[seq]) <= ATOL, (seq, ctc, want[seq])
            place[seq] = h
    fin = [(s, l) for s, l in zip(c["seqs"], c["ll"]) if np.isfinite(l)]
    assert sorted(place.values()) == list(range(len(fin)))               # the finite ones come first
    for (s0, l0), (s1, l1) in zip(fin[:-1], fin[1:]):
        if l0 - l1 > 1e-6:
            assert place[s0] < place[s1], (s0, l0, s1, l1)
    if c["space_id"] >= 0:
        r1 = NB.c_abi_beam_nbest(lp, None, blank, W, c["labels"], wip=1.0, nbest=W)
        for h in range(W):
            seq = NB.hypothesis(r1, 0, h)
            nw = NB.num_words(seq, c["space_id"])
            assert r1["counts"][0, h].tolist() == [nw, 0]
            tot, ctc = r1["scores"][0, h, 0], r1["scores"][0, h, 1]
            if np.isfinite(ctc):
                assert abs(ctc - want[seq]) <= ATOL and abs(tot - (ctc - nw)) <= ATOL, (seq, tot, ctc, nw)
            else:
                assert np.isneginf(tot) and np.isneginf(ctc)


# ---- 3. pruned beams never gain mass ----
def never_gains_mass(lp, x_len, blank, r):
    B = lp.shape[0]
    for b in range(B):
        nh = int(r["n_hyp"][b])
        seqs = [NB.hypothesis(r, b, h) for h in range(nh)]
        ll = NB.loglik(lp[b].double().numpy(), seqs, blank, x_len[b])
        ctc = r["scores"][b, :nh, 1]
        fin = np.isfinite(ctc)
        assert (ctc[fin] <= ll[fin] + ATOL).all(), (b, (ctc - ll)[fin].max())


def test_pruned_beam_scores_are_lower_bounds_of_the_likelihood():
    labels = ["_"] + [chr(97 + i) for i in range(26)] + [" ", "'"]
    lp = rand_lp(7, 3, 120, 29, sharp=3.0)
    xl = [120, 90, 61]
    r = check_list(lp, xl, 0, 100, labels, wip=1.0)
    assert r["n_hyp"].tolist() == [100, 100, 100]
    never_gains_mass(lp, xl, 0, r)


# ---- 4. fewer members than asked ----
def test_fewer_members_than_asked():
    r = check_list(rand_lp(3, 2, 1, 3), None, 0, 10, None)
    assert r["n_hyp"].tolist() == [3, 3]                                 # the root and its two children
    lp = rand_lp(4, 2, 40, 7)
    r = check_list(lp, [1, 40], 0, 10, LABELS7, wip=1.0)
    assert r["n_hyp"].tolist() == [7, 10]
    r = check_list(lp, [40, 1], 0, 10, LABELS7, nbest=4)                 # ... and fewer asked than there are
    assert r["n_hyp"].tolist() == [4, 4] and r["ids"].shape[1] == 4


# ---- 5. both regimes of the general kernel ----
@pytest.mark.parametrize("V,W,T", [(100, 100, 40), (300, 256, 25)])
def test_general_kernel_member_sets_in_lds_and_in_the_workspace(V, W, T):
    labels = ["_"] + ["w%d" % i for i in range(V - 2)] + [" "]
    lp = rand_lp(500 + V, 3, T, V, sharp=3.0)
    xl = [T, T - 3, max(T // 2, 1)]
    r = check_list(lp, xl, 0, W, labels, wip=0.5)
    assert r["n_hyp"].tolist() == [W] * 3
    never_gains_mass(lp, xl, 0, r)


def test_item_1_through_the_general_kernel():
    """test_hypothesis_0_is_decode_* again with E2E_BEAM_GENERAL=1 (read once per process: a child pytest)."""
    import subprocess
    import sys
    if os.environ.get("E2E_BEAM_GENERAL"):
        pytest.skip("already inside the child run")
    env = dict(os.environ, E2E_BEAM_GENERAL="1")
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x",
                          "-k", "hypothesis_0_is_decode"],
                         env=env, capture_output=True, text=True, timeout=600,
                         cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]


# ---- 6. language model ----
@pytest.mark.parametrize("W,lmwt,wip,oov", [(10, 1.0, 0.0, -10.0), (30, 0.5, 1.0, -3.0), (100, 2.0, 0.0, -1000.0)])
def test_lm_scores_and_counts(W, lmwt, wip, oov):
    labels = ["_", "a", "b", " "]
    lm = LanguageModel(ARPA, labels, True)
    olm = O.OracleLM(ARPA)
    lp = rand_lp(31 + W, 4, 25, 4, sharp=1.5)
    r = check_list(lp, [25, 25, 18, 9], 0, W, labels, lm=lm, olm=olm, lmwt=lmwt, wip=wip, oov_penalty=oov,
                   case_sensitive=True)
    for b in range(4):
        for h in range(int(r["n_hyp"][b])):
            seq = NB.hypothesis(r, b, h)
            words = "".join(labels[k] for k in seq).split()
            tot, ctc, lms = r["scores"][b, h]
            nw, no = r["counts"][b, h]
            assert nw == len(words) == NB.num_words(seq, 3)
            assert no == sum(lm.word_index(w) == 0 for w in words), (b, h, words)       # the last, possibly partial, word included (Q8)
            if np.isfinite(tot):
                assert abs(tot - (ctc + lmwt * lms - wip * nw + oov * no)) <= ATOL * max(1.0, abs(tot)), (b, h)


# ---- 7. timestamps ----
RUNS = [[(5, 2, 0), (4, 1, 0), (4, 3, 1), (3, 4, 2), (5, 1, 0), (3, 2, 1), (3, 1, 1), (4, 3, 0), (5, 2, 3)],
        [(3, 1, 2), (3, 3, 1), (5, 4, 0), (4, 2, 0), (3, 1, 0), (5, 3, 2), (4, 4, 1), (4, 1, 0), (5, 2, 1)]]


def aligned_batch():
    """B=2, T=30, V=6: one-hot x 20 of a known alignment, log-softmax.  RUNS: (label, frames, blanks behind it) -- runs of 1 to 4
    frames, a blank between repeated labels."""
    T, V = 30, 6
    x = torch.zeros(2, T, V, dtype=torch.float64)
    starts, seqs = [], []
    for b, runs in enumerate(RUNS):
        al = []
        for lab, n, bl in runs:
            al += [lab] * n + [0] * bl
        al = (al + [0] * T)[:T]
        x[b, torch.arange(T), torch.tensor(al)] = 20.0
        st = [t for t in range(T) if al[t] != 0 and (t == 0 or al[t - 1] != al[t])]
        starts.append(st); seqs.append([al[t] for t in st])
    return torch.log_softmax(x, -1), seqs, starts


@pytest.mark.parametrize("W", [2, 3])
def test_timestamps_of_a_known_alignment_are_the_first_frames_of_its_runs(W):
    """A label's timestamp is the frame at which the prefix ending in it was created.  With one-hot emissions a prefix is also
    created -- as an improbable extension, all of them exactly tied at 20 nats below the best -- before its label's run begins if
    the beam has room for it, and then keeps that earlier frame.  Beams of 2 and 3 have no room: beside the best prefix they
    hold the first of the tied extensions by position, i.e. by label (1, then 2), and the alignments use the labels 3..5 only, so
    every label's prefix is created exactly at the first frame of its run."""
    lp, seqs, starts = aligned_batch()
    r = check_list(lp, None, 0, W, None)
    for b in range(2):
        n = int(r["lens"][b, 0])
        assert r["ids"][b, 0, :n].tolist() == seqs[b]
        assert r["ts"][b, 0, :n].tolist() == starts[b]


# ---- 8. truncation ----
def test_truncated_rows_report_the_needed_length():
    lp = rand_lp(110, 5, 40, 7)
    full = NB.c_abi_beam_nbest(lp, XLEN5, 0, 10, LABELS7, nbest=10, timesteps=True)
    cut = NB.c_abi_beam_nbest(lp, XLEN5, 0, 10, LABELS7, nbest=10, timesteps=True, max_out=2, check_status=False)   # (returned 0)
    assert np.array_equal(cut["lens"], full["lens"]) and (full["lens"] > 2).any() and (full["lens"] <= 2).any()
    assert np.array_equal(cut["n_hyp"], full["n_hyp"]) and np.array_equal(cut["scores"], full["scores"])
    assert np.array_equal(cut["ids"], full["ids"][:, :, :2]) and np.array_equal(cut["ts"], full["ts"][:, :, :2])


# ---- 9. module level ----
@pytest.mark.parametrize("keep", [False, True])
def test_module_decode_nbest(keep):
    from end2end_amd import CTCDecoder, NBestResults
    import cpp_ctc_decoder
    g = torch.Generator().manual_seed(5)
    logits = (torch.randn(30, 4, 7, generator=g) * 2).to(U.dev())                 # time-major, raw logits
    xl = torch.tensor([30, 22, 9, 30])
    dec = CTCDecoder(beam_width=8, labels=LABELS7, time_major=True, after_logsoftmax=False, wip=1.0, keep_on_device=keep)
    s = torch.cuda.Stream(device=U.dev())
    s.wait_stream(torch.cuda.current_stream(U.dev()))
    with torch.cuda.stream(s):
        res = dec.decode_nbest(logits, xl, nbest=5, timesteps=True)
        plain = dec.decode_nbest(logits, xl, nbest=5)
    s.synchronize()
    one = dec.decode(logits, xl)
    assert isinstance(res, NBestResults) and plain.timesteps is None
    for t in (res.decoded_targets, res.decoded_targets_lengths, res.scores, res.num_words, res.num_hypotheses, res.timesteps):
        assert t.is_cuda == keep
    ids, lens = res.decoded_targets.cpu(), res.decoded_targets_lengths.cpu()
    assert ids.shape == (4, 5, int(lens.max())) and res.timesteps.shape == ids.shape          # packed to the longest hypothesis
    assert res.scores.shape == res.ctc_scores.shape == res.lm_scores.shape == res.num_words.shape == res.num_oov_words.shape == (4, 5)
    assert res.num_hypotheses.tolist() == [5] * 4
    assert [row[0] for row in res.decoded_sentences] == one.decoded_sentences
    assert lens[:, 0].tolist() == one.decoded_targets_lengths.tolist()
    for b in range(4):
        assert len(res.decoded_sentences[b]) == 5
        for h in range(5):
            assert res.decoded_sentences[b][h] == "".join(LABELS7[k] for k in ids[b, h, : lens[b, h]].tolist() if k >= 0)
    assert torch.equal(plain.decoded_targets.cpu(), ids) and torch.equal(plain.scores.cpu(), res.scores.cpu())
    sc = res.scores.cpu()
    assert (sc[:, :-1] >= sc[:, 1:]).all()
    assert torch.allclose(sc, res.ctc_scores.cpu() - res.num_words.cpu().double(), rtol=0, atol=ATOL)
    # the engine under the reference's name: default nbest = beam_width, log-probabilities in
    eng = cpp_ctc_decoder.CTCDecoder(0, 8, LABELS7, wip_=1.0)
    out = eng.decode_nbest(torch.log_softmax(logits.transpose(0, 1), -1), xl)
    assert out[0].shape[:2] == (4, 8) and out[9] is None and torch.equal(out[0][:, :5, : ids.shape[2]], ids)


def _status_after(monkeypatch, name, at, count, value):
    """Let the C call `name` run, then write `value` over the first int64 word of its argument `at` (a buffer of `count`
    words): the status a search that ran out of room reports there."""
    from end2end_amd import engines
    real = getattr(engines._C, name)

    def call(*args, **kw):
        real(*args, **kw)
        torch.cuda.synchronize()
        torch.as_tensor(U.DeviceWords(args[at], count), device="cuda")[0] = value
    monkeypatch.setattr(engines._C, name, call)


@pytest.mark.parametrize("what", ["nodes", "max_out"])
def test_engine_raises_the_status_that_rides_on_the_results(monkeypatch, what):
    """n_hyp < 0 and a length beyond max_out are errors that name the utterance, in decode_nbest and in a stream's read-out."""
    from end2end_amd.engines import CTCDecoderEngine
    from end2end_amd._runtime import E2EError
    B, T, V, W = 2, 6, 4, 4
    x = rand_lp(3, B, T, V).to("cuda")
    e = CTCDecoderEngine(0, W, ["_", "a", "b", " "])
    text = {"nodes": "beam search: utterance 0 ran out of prefix-tree nodes",
            "max_out": "beam search: utterance 0 needs %d output ids, %d provided" % (T + 2, T + 1)}[what]
    # (x, dtype, sB, sT, sV, x_len, B, T, V, blank, W, space, lm, lmwt, wip, oov, N, out, max_out, out_len, n_hyp, ...)
    at, count, value = {"nodes": (20, B, -1), "max_out": (19, B * W, T + 2)}[what]
    _status_after(monkeypatch, "ctc_beam_nbest", at, count, value)
    with pytest.raises(E2EError, match=text):
        e.decode_nbest(x, torch.tensor([T, T]))
    # (..., oov, state, row_bytes, max_frames, with_timesteps, N, out, max_out, out_len, n_hyp, ...)
    _status_after(monkeypatch, "ctc_beam_stream", at + 4, count, value)
    with pytest.raises(E2EError, match=text):
        e.open_stream(B, T).feed_nbest(x)


def test_engine_stream_names_the_status_of_its_own(monkeypatch):
    """frames_done = -1: the CTC stream alone can run out of prefix-tree nodes; the other utterance has advanced."""
    from end2end_amd.engines import CTCDecoderEngine
    from end2end_amd._runtime import E2EError
    B, T, V, W = 2, 6, 4, 4
    st = CTCDecoderEngine(0, W, ["_", "a", "b", " "]).open_stream(B, T)
    # (..., N, out, max_out, out_len, n_hyp, scores, counts, timesteps, frames_done, ...)
    _status_after(monkeypatch, "ctc_beam_stream", 28, B, -1)
    with pytest.raises(E2EError, match="beam search stream: utterance 0 ran out of prefix-tree nodes"):
        st.feed_nbest(rand_lp(3, B, T, V).to("cuda"))
    assert st.frames == [0, T]
