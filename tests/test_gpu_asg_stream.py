"""GPU: the streaming ASG beam search (e2e_asg_beam_stream; ASGDecoder.open_stream) against the whole-utterance call
e2e_asg_beam_nbest_opt on the frames fed so far: np.array_equal on every output -- ids, lengths, n_hyp, scores, counts,
timesteps -- after every chunk (tests/asg_stream_util.py).  The stream does the same arithmetic in the same order, so there
is no tolerance.  One final read-out is also pinned to the plain-Python restatement, as test_gpu_asg_beam.py compares."""
import math
import os

import numpy as np
import pytest
import torch

import asg_beam_util as U
import asg_stream_util as S
from test_gpu_asg_beam import DEV, DTYPES, LETTERS, check_ranking, decoder

pytestmark = pytest.mark.gpu

_caches = {}


def cache(*key):
    """The whole-call references of one case, shared by its chunkings."""
    return _caches.setdefault(key, {})


def pruned(dt):
    x, A = U.pruned_case()
    return torch.from_numpy(x).to(DTYPES[dt]), torch.from_numpy(A).to(DTYPES[dt])


# some utterances get no frame in some calls; the sums are PRUNED_LENS
PER_UTTERANCE = [[5, 0, 3], [0, 4, 0], [10, 10, 10], [0, 0, 0], [0, 0, 7], [25, 9, 11]]
CHUNKINGS = {
    "every_frame": (lambda: S.regular(U.PRUNED_LENS, U.PRUNED_T, 1), None),
    "sevens": (lambda: S.regular(U.PRUNED_LENS, U.PRUNED_T, 7), "time_major"),
    "13_1_26": (lambda: S.cuts(U.PRUNED_LENS, [13, 1, 26]), "strided"),
    "per_utterance": (lambda: PER_UTTERANCE, None),
}


# ---- 1. plain ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("name", sorted(CHUNKINGS))
@pytest.mark.parametrize("W", [2, 7, 32, 100])
def test_plain(W, name, dt):
    x, A = pruned(dt)
    chunking, layout = CHUNKINGS[name]
    chunking = chunking()
    assert [sum(c[b] for c in chunking) for b in range(3)] == U.PRUNED_LENS
    r = S.check_stream(x, A, U.PRUNED_LENS, chunking, U.PRUNED_R, W, U.PRUNED_SPACE, cache=cache("plain", W, dt),
                       layout=layout)
    assert r["n_hyp"].tolist() == [W] * 3


def hyps_of(r, b):
    """The read-out of utterance b as the restatement lists its hypotheses."""
    out = []
    for k in range(int(r["n_hyp"][b])):
        m = int(r["lens"][b, k])
        out.append(dict(ids=tuple(r["ids"][b, k, :m].tolist()), total=float(r["scores"][b, k, 0]), ac=float(r["scores"][b, k, 1]),
                        lm=float(r["scores"][b, k, 2]), words=int(r["counts"][b, k, 0]), oov=int(r["counts"][b, k, 1])))
    return out


def test_final_read_out_equals_restatement():
    W = 7
    want, gap = U.pruned_ref(W)
    assert gap >= U.MIN_GAP
    x, A = pruned("f64")
    r = S.check_stream(x, A, U.PRUNED_LENS, S.regular(U.PRUNED_LENS, U.PRUNED_T, 7), U.PRUNED_R, W, U.PRUNED_SPACE,
                       cache=cache("plain", W, "f64"))
    for b in range(3):
        check_ranking(hyps_of(r, b), want[b])


def test_wide_alphabet():
    x, A = U.wide_case()
    S.check_stream(torch.from_numpy(x), torch.from_numpy(A), U.WIDE_LENS, S.regular(U.WIDE_LENS, U.WIDE_T, 1), 0, U.WIDE_W, -1)


# ---- 2. with a language model, and restricted ----------------------------------------------------------------------------
def model_case(model, case_sensitive):
    chars = U.LM_MODELS[model]["chars"] if case_sensitive else U.upper_chars(U.LM_MODELS[model]["chars"])
    x, A = U.lm_case(model)
    return chars, chars + ["<1>"], torch.from_numpy(x), torch.from_numpy(A)


@pytest.mark.parametrize("case_sensitive", [True, False])
@pytest.mark.parametrize("W", U.LM_WIDTHS)
@pytest.mark.parametrize("model", sorted(U.LM_MODELS))
def test_lm(model, W, case_sensitive):
    from end2end_amd.engines import LanguageModel
    chars, labels, x, A = model_case(model, case_sensitive)
    lm = LanguageModel(os.path.join(U.GOLDEN, model), labels, case_sensitive)
    r = S.check_stream(x, A, U.LM_LENS, S.regular(U.LM_LENS, U.LM_T, 1), U.LM_R, W, chars.index(" "), lm=lm, **U.LM_KNOBS)
    assert int(r["n_hyp"].min()) > 0


@pytest.mark.parametrize("vocabulary", ["model", "words"])
def test_restricted(vocabulary):
    from end2end_amd.engines import LanguageModel
    model = "lm_order4.arpa"
    chars, labels, x, A = model_case(model, True)
    if vocabulary == "model":
        lm, knobs = LanguageModel(os.path.join(U.GOLDEN, model), labels, True, lexicon=True), U.LM_KNOBS
    else:
        lm = LanguageModel(None, labels, True, words=["add", "bed", "a", "cab", "dead", "ace", "e'e"], lexicon=True)
        knobs = dict(wip=0.4)
    kw = dict(lm=lm, **knobs)
    space = chars.index(" ")
    r = S.check_stream(x, A, U.LM_LENS, S.regular(U.LM_LENS, U.LM_T, 1), U.LM_R, 7, space, restrict=True, **kw)
    # (the restriction bites: the unrestricted search over the same model ends elsewhere)
    free = S.reference(x, A, U.LM_LENS, U.LM_R, 7, space, **kw)
    assert not np.array_equal(r["ids"], free["ids"])


# ---- 3. the edges of the contract ----------------------------------------------------------------------------------------
def test_zero_transitions():
    x, _ = pruned("f32")
    S.check_stream(x, None, U.PRUNED_LENS, S.cuts(U.PRUNED_LENS, [13, 1, 26]), U.PRUNED_R, 7, U.PRUNED_SPACE)


def test_timesteps_are_frames_of_the_stream():
    x, A = pruned("f32")
    r = S.check_stream(x, A, U.PRUNED_LENS, S.regular(U.PRUNED_LENS, U.PRUNED_T, 7), U.PRUNED_R, 32, U.PRUNED_SPACE,
                       cache=cache("plain", 32, "f32"))
    late = 0
    for b in range(3):
        for k in range(32):
            n = int(r["lens"][b, k])
            ts = r["ts"][b, k, :n].tolist()
            assert ts[0] == 0 and all(p < q for p, q in zip(ts, ts[1:])) and ts[-1] < U.PRUNED_LENS[b]
            assert (r["ts"][b, k, n:] == -1).all()
            late += ts[-1] >= 7
    assert late                                                         # (frames beyond the first chunk: not the chunk's own count)


def test_a_dead_beam_stays_dead():
    x, A = pruned("f32")
    x = x[:2, :20].clone()
    x[0, 9, :] = -math.inf
    lens = [20, 20]
    c = {}
    for size in (1, 4):
        S.check_stream(x, A, lens, S.regular(lens, 20, size), U.PRUNED_R, 7, U.PRUNED_SPACE, cache=c)
    assert c[(8, 8)]["n_hyp"].tolist() == [7, 7] and c[(12, 12)]["n_hyp"].tolist() == [0, 7] and c[(20, 20)]["n_hyp"].tolist() == [0, 7]
    assert (c[(20, 20)]["scores"][0, :, 0] == -math.inf).all() and (c[(20, 20)]["lens"][0] == 0).all()


def test_short_max_out():
    x, A = pruned("f32")
    r = S.check_stream(x, A, U.PRUNED_LENS, S.regular(U.PRUNED_LENS, U.PRUNED_T, 7), U.PRUNED_R, 7, U.PRUNED_SPACE, max_out=5)
    assert int(r["lens"].max()) > 5 and r["ids"].shape[2] == 5


def test_feed_only():
    x, A = pruned("f32")
    W, lens = 7, U.PRUNED_LENS
    s = S.RawStream(3, U.PRUNED_T, U.PRUNED_V, U.PRUNED_R, W, U.PRUNED_SPACE, A)
    dx = x.to(DEV)
    o = S.garbage(3, 1, s.max_out, DEV)
    before = S.host(o)
    for chunk_no, (a, cl) in enumerate(zip(range(0, 40, 7), S.regular(lens, U.PRUNED_T, 7))):
        r = s.feed(dx[:, a:a + 7], cl, nbest=0, outputs=o)
        assert r["done"].tolist() == [min(n, a + 7) for n in lens]
        S.same(r, before, "feed only wrote an output")
    r = s.feed(dx[:, :1], [0, 0, 0])                                     # a read-out alone
    S.same(r, S.reference(x, A, lens, U.PRUNED_R, W, U.PRUNED_SPACE))
    assert r["done"].tolist() == lens


def test_rows_permuted_and_reset():
    x, A = pruned("f32")
    W, T = 7, U.PRUNED_T
    s = S.RawStream(3, T, U.PRUNED_V, U.PRUNED_R, W, U.PRUNED_SPACE, A)
    dx = x.to(DEV)
    ref = lambda lens, xx=x: S.reference(xx, A, lens, U.PRUNED_R, W, U.PRUNED_SPACE)   # noqa: E731
    S.same(s.feed(dx[:, :10], [10, 10, 10]), ref([10, 10, 10]))
    perm = [2, 0, 1]
    s.state = s.state[perm].contiguous()                                # the rows move, and the chunks with them
    r = s.feed(dx[perm, 10:23], [13, 13, 13])
    want = ref([23, 23, 23])
    S.same({k: (v[perm] if v is not None else None) for k, v in want.items()}, {k: r[k] for k in S.KEYS}, "permuted")
    # row 1 (utterance 0) starts anew, on utterance 1's frames; the others go on
    s.state[1, :S.HEADER] = 0
    chunk = torch.stack([dx[2, 23:31], dx[1, :8], dx[1, 23:31]])
    r = s.feed(chunk, [8, 8, 8])
    assert r["done"].tolist() == [31, 8, 31]
    a, fresh = ref([31, 31, 31]), ref([8, 8, 8])
    for k in S.KEYS:
        assert np.array_equal(r[k][0], a[k][2]) and np.array_equal(r[k][2], a[k][1]), k
        assert np.array_equal(r[k][1], fresh[k][1]), k


def test_statuses():
    from end2end_amd.engines import LanguageModel
    x, A = pruned("f32")
    W, V, R = 7, U.PRUNED_V, U.PRUNED_R
    s = S.RawStream(3, 20, V, R, W, U.PRUNED_SPACE, A)
    dx = x.to(DEV)
    ref = lambda lens: S.reference(x, A, lens, R, W, U.PRUNED_SPACE, max_out=20)   # noqa: E731
    S.same(s.feed(dx[:, :12], [12, 5, 12]), ref([12, 5, 12]))

    def refused(r, rows, status, want_lens, others=True):
        """The rows `rows` answer `status` and are left alone, outputs and state; the others advanced."""
        assert torch.equal(s.state[rows], before[rows])
        want = ref(want_lens) if want_lens else None
        for b in range(3):
            if b in rows:
                assert r["done"][b] == status and r["n_hyp"][b] == status
                assert (r["ids"][b] == -7).all() and (r["lens"][b] == -7).all() and (r["scores"][b] == 7.0).all()
                assert (r["counts"][b] == -7).all() and (r["ts"][b] == -7).all()
            elif others:
                assert r["done"][b] == want_lens[b]
                for k in S.KEYS:
                    assert np.array_equal(r[k][b], want[k][b]), (k, b)

    # -2: 12 + 9 > max_frames = 20 for utterances 0 and 2; utterance 1 advances
    before = s.state.clone()
    refused(s.feed(torch.stack([dx[0, 12:21], dx[1, 5:14], dx[2, 12:21]]), [9, 9, 9]), [0, 2], -2, [12, 14, 12])
    assert not torch.equal(s.state[1], before[1])
    # ... and what fits is taken afterwards
    S.same(s.feed(dx[:, 12:20], [8, 0, 8]), ref([20, 14, 20]))
    # -3: the rows were written at width 7, V = 29, without a model
    before = s.state.clone()
    refused(s.feed(dx[:, :1], [1, 1, 1], W=6), [0, 1, 2], -3, None)
    refused(s.feed(dx[:, :1, :28], [1, 1, 1], A=A[:28, :28]), [0, 1, 2], -3, None)
    refused(s.feed(dx[:, :1], [1, 1, 1], R=1), [0, 1, 2], -3, None)
    refused(s.feed(dx[:, :1], [1, 1, 1], max_frames=19), [0, 1, 2], -3, None)
    lm = LanguageModel(None, LETTERS + ["<1>", "<2>"], True, words=["a"])
    big = S.RawStream(3, 20, V, R, W, U.PRUNED_SPACE, A, lm=lm)         # (a model's row is longer: the same rows, widened)
    big.state[:, :s.row_bytes] = s.state
    s.state, s.row_bytes = big.state, big.row_bytes
    before = s.state.clone()
    refused(s.feed(dx[:, :1], [1, 1, 1], lm=lm), [0, 1, 2], -3, None)
    # a fresh row beside them is served
    s.state[1, :S.HEADER] = 0
    before = s.state.clone()
    r = s.feed(dx[:, :6], [6, 6, 6], W=6, lm=None)
    refused(r, [0, 2], -3, None, others=False)
    fresh = S.reference(x, A, [6, 6, 6], R, 6, U.PRUNED_SPACE, max_out=20)
    assert r["done"][1] == 6 and all(np.array_equal(r[k][1], fresh[k][1]) for k in S.KEYS)


# ---- 4. the module -------------------------------------------------------------------------------------------------------
FIELDS = ("decoded_targets", "decoded_targets_lengths", "scores", "ctc_scores", "lm_scores", "num_words", "num_oov_words",
          "num_hypotheses", "timesteps")


@pytest.mark.parametrize("keep_on_device,time_major", [(False, False), (True, True)])
def test_module(keep_on_device, time_major):
    from end2end_amd import ASGDecoder
    from end2end_amd._runtime import E2EError
    model = "lm_order4.arpa"
    chars, _, x, A = model_case(model, True)
    x, A = x.to(DEV), A.to(DEV)
    d = ASGDecoder(labels=chars, num_replabels=U.LM_R, time_major=time_major, keep_on_device=keep_on_device)
    d.configure(beam_width=7, lm_path=os.path.join(U.GOLDEN, model), **U.LM_KNOBS).restrict_to_vocabulary()
    shaped = (lambda t: t.transpose(0, 1)) if time_major else (lambda t: t)
    st = d.open_stream(A, 3, U.LM_T, timesteps=True)
    fed = [0, 0, 0]
    for a, cl in zip(range(0, U.LM_T, 5), S.regular(U.LM_LENS, U.LM_T, 5)):
        chunk, cl = shaped(x[:, a:a + 5]), torch.tensor(cl)
        fed = [f + int(n) for f, n in zip(fed, cl)]
        if a == 5:
            best = st.feed(chunk, cl)
            want = d.decode(shaped(x), A, torch.tensor(fed))
            assert torch.equal(best.decoded_targets, want.decoded_targets) and best.decoded_sentences == want.decoded_sentences
            assert torch.equal(best.decoded_targets_lengths, want.decoded_targets_lengths)
        else:
            got = st.feed_nbest(chunk, cl)
            want = d.decode_nbest(shaped(x), A, torch.tensor(fed), timesteps=True)
            for f in FIELDS:
                assert torch.equal(getattr(got, f), getattr(want, f)), (f, fed)
            assert got.decoded_sentences == want.decoded_sentences
            assert got.decoded_targets.is_cuda == keep_on_device
        assert st.frames == fed
    assert fed == U.LM_LENS and st.state.shape == (3, st.row_bytes)
    # a status surfaces as an error that names the utterance; the others have advanced
    with pytest.raises(E2EError, match="utterance 0 would pass max_frames=%d" % U.LM_T):
        st.feed(shaped(x[:, :2]), torch.tensor([1, 2, 0]))
    assert st.frames == [U.LM_LENS[0], U.LM_LENS[1] + 2, U.LM_LENS[2]]
    st.reset([0])
    assert st.frames[0] == 0
    got = st.feed_nbest(shaped(x[:, :4]), torch.tensor([4, 0, 0]), nbest=2)
    want = d.decode_nbest(shaped(x), A, torch.tensor([4, 1, 1]), nbest=2, timesteps=True)
    assert torch.equal(got.scores[0], want.scores[0]) and got.decoded_sentences[0] == want.decoded_sentences[0]
    assert st.feed_nbest(shaped(x[:, :1]), torch.tensor([1, 0, 0]), nbest=0) is None and st.frames[0] == 5


def test_module_zero_transitions_and_half():
    d = decoder(7, LETTERS, U.PRUNED_R, wip=0.0)
    x, _ = pruned("f32")
    xh = x.to(torch.bfloat16).to(DEV)
    st = d.open_stream(None, 3, U.PRUNED_T)
    for a in (0, 20):
        got = st.feed_nbest(xh[:, a:a + 20])
    want = d.decode_nbest(xh, None)
    assert got.timesteps is None
    for f in FIELDS[:-1]:
        assert torch.equal(getattr(got, f), getattr(want, f)), f
    assert got.decoded_sentences == want.decoded_sentences


# ---- 5. what the engine's host layer adds to the calls -----------------------------------------------------------------------
def _empty_slot(r, b, N):
    """Utterance b of an n-best tuple is the empty result: no hypothesis, length 0, -inf, an LM score of 0, timesteps -1."""
    assert int(r[8][b]) == 0 and r[2][b] == [] and r[1][b].tolist() == [0] * N and r[0][b].tolist() == [[0] * r[0].shape[2]] * N
    assert r[3][b].tolist() == [-math.inf] * N and r[4][b].tolist() == [-math.inf] * N and r[5][b].tolist() == [0.0] * N
    assert r[6][b].tolist() == [0] * N and r[7][b].tolist() == [0] * N
    assert r[9][b].tolist() == [[-1] * r[9].shape[2]] * N


def test_engine_leaves_an_utterance_without_frames_empty():
    """The call does not touch an utterance of length 0, nor a stream's utterance that has been fed no frame: the engine's
    buffers are the empty result beforehand.  No frames at all: no launch, the same empty result."""
    from end2end_amd.engines import ASGBeamEngine
    from gpu_util import poison_allocator
    e = ASGBeamEngine(["a", "b", " ", "c", "d"], 0, 4)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, 6, 5, generator=g).to(DEV)
    poison_allocator(DEV)
    r = e.decode_nbest(x, None, torch.tensor([6, 0, 3]), timesteps=True)
    _empty_slot(r, 1, 4)
    assert r[8].tolist() == [4, 0, 4]
    st = e.open_stream(None, 3, 12, timesteps=True)
    poison_allocator(DEV)
    s = st.feed_nbest(x[:, :5], torch.tensor([5, 0, 2]))
    _empty_slot(s, 1, 4)
    assert st.frames == [5, 0, 2] and s[8].tolist() == [4, 0, 4]
    want = e.decode_nbest(x[:, :5], None, torch.tensor([5, 0, 2]), timesteps=True)
    for i in (0, 1, 3, 4, 5, 6, 7, 8, 9):
        assert torch.equal(s[i], want[i]), i
    assert s[2] == want[2]
    z = e.decode_nbest(torch.zeros(2, 0, 5, device=DEV), None, torch.tensor([0, 0]), timesteps=True)
    assert z[0].shape == (2, 4, 0) and z[9].shape == (2, 4, 0)
    for b in range(2):
        _empty_slot(z, b, 4)


def test_engine_stream_keeps_its_transitions_per_dtype():
    """Chunks of either dtype in one stream: each reads the transitions in its own dtype (f32 values are exact in f64, so the
    result is the whole f32 call's)."""
    from end2end_amd.engines import ASGBeamEngine
    e = ASGBeamEngine(["a", "b", " ", "c", "d"], 0, 4)
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 10, 5, generator=g).to(DEV)
    A = torch.randn(5, 5, generator=g)
    want = e.decode_nbest(x, A, torch.tensor([10, 10]))
    st = e.open_stream(A, 2, 10)
    st.feed_nbest(x[:, :3].double(), nbest=0)
    st.feed_nbest(x[:, 3:6], nbest=0)
    st.feed_nbest(x[:, 6:8].double(), nbest=0)
    got = st.feed_nbest(x[:, 8:])
    for i in (0, 1, 3, 4, 5, 6, 7, 8):
        assert torch.equal(got[i], want[i]), i
    assert got[2] == want[2] and got[9] is None and st.frames == [10, 10]
