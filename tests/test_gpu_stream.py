"""-m gpu: the streaming beam search (e2e_ctc_beam_stream).  After every chunk every output -- ids, lengths, counts of
hypotheses, scores, word counts, timestamps -- is held to e2e_ctc_beam_nbest(_opt) on the frames fed so far with np.array_equal,
and hypothesis 0 to the oracle's beam search: a stream does the same arithmetic in the same order, so there is no tolerance."""
import os

import numpy as np
import pytest
import torch

import golden_util as G
import gpu_util as U
import oracle_lib as O
import stream_util as S
from end2end_amd.engines import LanguageModel

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ARPA = os.path.join(GOLD, "tiny_3gram.arpa")
LABELS7 = ["_", "a", "b", "c", " ", "d", "'"]
LABELS4 = ["_", "a", "b", " "]
XLEN5 = [40, 33, 17, 40, 1]
# per-utterance chunk lengths that sum to XLEN5: zeros in the middle and at the start, boundaries at frames 1, 2 and 3
IRREGULAR5 = [[1, 0, 2, 3, 0], [1, 1, 0, 0, 1], [1, 2, 1, 5, 0], [0, 0, 0, 0, 0], [7, 10, 14, 2, 0], [30, 20, 0, 30, 0]]


def rand_lp(seed, B, T, V, sharp=2.0, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    return torch.log_softmax(torch.randn(B, T, V, generator=g, dtype=torch.float64) * sharp, -1).to(dtype)


def every_frame(x_len, T):
    return S.regular(x_len, T, 1)


# ---- 1. plain beams at every boundary ----
@pytest.mark.parametrize("W", [2, 3, 10, 100])
@pytest.mark.parametrize("wip", [0.0, 1.0])
def test_plain_beams_at_every_boundary(W, wip):
    assert [sum(c[b] for c in IRREGULAR5) for b in range(5)] == XLEN5
    lp = rand_lp(100 + W, 5, 40, 7)
    cache = {}
    for chunking in (every_frame(XLEN5, 40), S.regular(XLEN5, 40, 7), S.regular(XLEN5, 40, 40), IRREGULAR5):
        r = S.check_stream(lp, XLEN5, chunking, 0, W, LABELS7, cache=cache, wip=wip)
    assert r["done"].tolist() == XLEN5
    # one chunk is the whole call: compared above with the reference at the full lengths
    S.check_stream(lp, XLEN5, S.regular(XLEN5, 40, 7), 6, W, LABELS7[::-1], wip=wip)                  # blank last, space elsewhere
    S.check_stream(lp.float(), None, S.regular([40] * 5, 40, 7), 0, W, None, wip=wip)                 # f32 chunks, no labels
    S.check_stream(lp.bfloat16(), XLEN5, IRREGULAR5, 0, W, LABELS7, wip=wip)                          # 16-bit chunks
    S.check_stream(lp, XLEN5, S.regular(XLEN5, 40, 7), 0, W, LABELS7, wip=wip, time_major=True)       # a time-major tensor's view


# ---- 2. ties: the order of the members survives a boundary ----
@pytest.mark.parametrize("W", [4, 70])
def test_massive_ties_one_frame_at_a_time(W):
    labels = ["_", "a", "b", "c", "d", "e", "f", "g", "h", " "]
    V = len(labels)
    flat = torch.full((2, 9, V), float(np.log(1.0 / V)), dtype=torch.float64)
    S.check_stream(flat, [9, 6], every_frame([9, 6], 9), 0, W, labels, wip=0.0)
    two = torch.log(torch.tensor([0.3] + [0.7 / (V - 1)] * (V - 1), dtype=torch.float64)).repeat(2, 9, 1)
    S.check_stream(two, [9, 7], every_frame([9, 7], 9), 0, W, labels, wip=1.0)
    holes = flat.clone(); holes[:, :, 3] = float("-inf"); holes[:, ::2, 5] = float("-inf")
    S.check_stream(holes, [9, 9], every_frame([9, 9], 9), 0, W, labels, wip=0.0)


# ---- 3. quirks ----
def test_empty_winner():
    lp = torch.log(torch.tensor([[[0.98, 0.01, 0.01]] * 4], dtype=torch.float64))
    r = S.check_stream(lp, None, every_frame([4], 4), 0, 10, None)
    assert r["ids"][0, 0, :2].tolist() == [-1, 0] and r["lens"][0, 0] == 1 and r["ts"][0, 0, 0] == -1         # quirk Q6


@pytest.mark.parametrize("case", G.beam_q7_cases(), ids=lambda c: c["name"])
def test_pruned_but_living_child_is_found_after_a_resume(case):
    """Quirk Q7 (tests/golden/make_beam_q7_golden.py): a pruned child that a descendant keeps alive is found, not re-created --
    at a resume through the guards and the child tables rebuilt from them."""
    lp = torch.tensor(case["log_probs"], dtype=torch.float64)[None]
    T = lp.shape[1]
    r = S.check_stream(lp, None, every_frame([T], T), case["blank"], case["beam_width"], case["labels"])
    got = r["ids"][0, 0, : r["lens"][0, 0]].tolist()
    assert got == case["expected"] and got != case["without_q7"]


# ---- 4. language model ----
XLEN_LM = [25, 25, 18, 9]


@pytest.mark.parametrize("W,lmwt,wip,oov", [(10, 1.0, 0.0, -10.0), (30, 0.5, 1.0, -3.0), (100, 2.0, 0.0, -1000.0)])
def test_language_model(W, lmwt, wip, oov):
    lm = LanguageModel(ARPA, LABELS4, True)
    olm = O.OracleLM(ARPA)
    lp = rand_lp(31 + W, 4, 25, 4, sharp=1.5)
    cache = {}
    for size in (1, 6):
        r = S.check_stream(lp, XLEN_LM, S.regular(XLEN_LM, 25, size), 0, W, LABELS4, lm=lm, olm=olm, cache=cache,
                           lmwt=lmwt, wip=wip, oov_penalty=oov, case_sensitive=True)
    assert (r["counts"][:, 0, 0] > 0).any() and (r["scores"][:, 0, 2] != 0).any()            # the model did score


def test_language_model_id_table_walk(tmp_path):
    """The model that lists a trigram without its context (tests/test_gpu_beam.py): served from the id-keyed tables."""
    src = open(ARPA).read()
    pruned = src.replace("-0.6\ta b\t-0.2\n", "").replace("ngram 2=5", "ngram 2=4")
    assert pruned != src
    path = str(tmp_path / "pruned.arpa")
    open(path, "w").write(pruned)
    lm = LanguageModel(path, LABELS4, True)
    olm = O.OracleLM(path)
    lp = rand_lp(6, 3, 20, 4, sharp=1.5)
    xl = [20, 14, 5]
    for size in (1, 6):
        S.check_stream(lp, xl, S.regular(xl, 20, size), 0, 40, LABELS4, lm=lm, olm=olm, lmwt=1.5, wip=0.5, oov_penalty=-5.0,
                       case_sensitive=True)


def test_language_model_order_4_walk():
    labels = ["_", "a", "b", "c", "d", "e", "'", " "]
    path = os.path.join(GOLD, "lm_order4.arpa")
    lm = LanguageModel(path, labels, True)
    olm = O.OracleLM(path)
    g = torch.Generator().manual_seed(77)
    x = torch.randn(3, 30, 8, generator=g, dtype=torch.float64) * 2.0
    x[:, :, 7] += 1.0
    lp = torch.log_softmax(x, -1)
    xl = [30, 21, 5]
    for size in (1, 7):
        S.check_stream(lp, xl, S.regular(xl, 30, size), 0, 30, labels, lm=lm, olm=olm, lmwt=1.0, wip=0.0, oov_penalty=-5.0,
                       case_sensitive=True)


# ---- 5. restricted search ----
@pytest.mark.parametrize("model", ["words", "lm"])
def test_restricted_search(model):
    tiny = ["a", "ab", "b", "ba"]
    if model == "words":
        lm, kw = LanguageModel(None, LABELS4, True, words=tiny, lexicon=True), dict(lmwt=0.0, wip=1.0, oov_penalty=0.0)
    else:
        lm, kw = LanguageModel(ARPA, LABELS4, True, lexicon=True), dict(lmwt=0.7, wip=0.5, oov_penalty=0.0)
    xl = [25, 22, 12]
    lp = rand_lp(4100, 3, 25, 4, sharp=1.5)
    differ = 0
    for W in (3, 30):
        r = S.check_stream(lp, xl, every_frame(xl, 25), 0, W, LABELS4, lm=lm, restrict=True, **kw)
        u = S.reference(lp, xl, 0, W, LABELS4, lm, False, **kw)
        differ += not np.array_equal(r["ids"], u["ids"])
    assert differ                                                                             # the restriction did restrict


# ---- 6. the general kernel ----
def test_items_1_to_5_through_the_general_kernel():
    """Everything above again with E2E_BEAM_GENERAL=1 (read once per process: a child pytest)."""
    import subprocess
    import sys
    if os.environ.get("E2E_BEAM_GENERAL"):
        pytest.skip("already inside the child run")
    env = dict(os.environ, E2E_BEAM_GENERAL="1")
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-k",
                          "plain_beams or massive_ties or empty_winner or pruned_but_living or language_model or restricted_search"],
                         env=env, capture_output=True, text=True, timeout=900,
                         cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]


@pytest.mark.parametrize("V,W,T", [(100, 100, 40), (300, 256, 25)])
def test_general_kernel_member_sets_in_lds_and_in_the_workspace(V, W, T):
    labels = ["_"] + ["w%d" % i for i in range(V - 2)] + [" "]
    lp = rand_lp(500 + V, 3, T, V, sharp=3.0)
    xl = [T, T - 3, max(T // 2, 1)]
    r = S.check_stream(lp, xl, S.regular(xl, T, 5), 0, W, labels, wip=0.5)
    assert r["n_hyp"].tolist() == [W] * 3


# ---- 7. timestamps are frames of the stream ----
@pytest.mark.parametrize("W", [2, 3])
def test_timestamps_are_global(W):
    from test_gpu_nbest import aligned_batch
    lp, seqs, starts = aligned_batch()
    r = S.check_stream(lp, None, S.regular([30, 30], 30, 4), 0, W, None)
    for b in range(2):
        n = int(r["lens"][b, 0])
        assert r["ids"][b, 0, :n].tolist() == seqs[b]
        assert r["ts"][b, 0, :n].tolist() == starts[b] and max(starts[b]) >= 4                # beyond the first chunk


# ---- 8. rows are self-contained ----
def test_rows_may_be_permuted_and_reset():
    B, T, V, W = 5, 40, 7, 10
    lp = rand_lp(7, B, T, V)
    dlp = lp.to(U.dev())
    s = S.RawStream(B, T, V, W, LABELS7, wip=1.0)
    s.feed(dlp[:, 0:6], [6] * B)
    s.feed(dlp[:, 6:13], [7, 7, 3, 7, 0])
    fed = [13, 13, 9, 13, 6]
    perm = [3, 0, 4, 2, 1]
    idx = torch.tensor(perm, device=U.dev())
    s.state = s.state.index_select(0, idx)                                  # a copy elsewhere: no address survives in a row
    nxt = torch.zeros((B, 8, V), dtype=lp.dtype, device=U.dev())
    for j, b in enumerate(perm):
        nxt[j] = dlp[b, fed[b]:fed[b] + 8]
    r = s.feed(nxt, [8] * B)
    total = [fed[b] + 8 for b in range(B)]
    ref = S.reference(lp, total, 0, W, LABELS7, wip=1.0)
    assert r["done"].tolist() == [total[b] for b in perm]
    for k in S.KEYS:
        assert np.array_equal(r[k], ref[k][perm]), k
    # a reset of one row restarts that utterance alone
    s.state[2, :S.HEADER] = 0
    lens = [5, 5, 9, 5, 5]
    nxt = torch.zeros((B, 9, V), dtype=lp.dtype, device=U.dev())
    for j, b in enumerate(perm):
        a = 0 if j == 2 else total[b]
        nxt[j, :lens[j]] = dlp[b, a:a + lens[j]]
    r = s.feed(nxt, lens)
    want = [9 if j == 2 else total[b] + 5 for j, b in enumerate(perm)]
    assert r["done"].tolist() == want
    for j, b in enumerate(perm):
        x_len = [1] * B
        x_len[b] = want[j]
        ref = S.reference(lp, x_len, 0, W, LABELS7, wip=1.0)
        for k in S.KEYS:
            assert np.array_equal(r[k][j], ref[k][b]), (j, k)


# ---- 9. statuses ----
def test_statuses_leave_the_row_alone():
    B, T, V, W = 3, 20, 7, 10
    lp = rand_lp(9, B, 30, V)
    dlp = lp.to(U.dev())
    s = S.RawStream(B, T, V, W, LABELS7, max_out=31)
    s.feed(dlp[:, :15], [15, 10, 15])
    before = s.state.clone()
    r = s.feed(dlp[:, 15:21], [6, 6, 5])                                     # utterance 0 would reach 21 > max_frames = 20
    assert r["done"].tolist() == [-2, 16, 20] and r["n_hyp"].tolist() == [-2, W, W]
    assert torch.equal(s.state[0], before[0]) and not torch.equal(s.state[1], before[1])
    assert (r["ids"][0] == -7).all() and (r["lens"][0] == -7).all()          # nothing else of the refused utterance is written
    ref = S.reference(lp, [15, 10, 20], 0, W, LABELS7)
    lp1 = lp.clone(); lp1[1, 10:16] = lp[1, 15:21]                           # utterance 1 was fed frames 0..9, then 15..20
    ref1 = S.reference(lp1, [15, 16, 20], 0, W, LABELS7)
    for k in S.KEYS:
        assert np.array_equal(r[k][2], ref[k][2]) and np.array_equal(r[k][1], ref1[k][1]), k
    r = s.feed(dlp[:, 15:20], [5, 0, 0])                                     # ... and fits exactly afterwards
    assert r["done"].tolist() == [20, 16, 20]
    # a row written with W = 10, fed with W = 8
    before = s.state.clone()
    r = s.feed(dlp[:, :1], [0, 0, 0], W=8)
    assert r["done"].tolist() == [-3] * 3 and r["n_hyp"].tolist() == [-3] * 3 and torch.equal(s.state, before)
    # nbest = 0 feeds without touching the outputs
    s2 = S.RawStream(B, T, V, W, LABELS7, max_out=31)
    r = s2.feed(dlp[:, :7], [7, 7, 2], nbest=0)
    assert r["done"].tolist() == [7, 7, 2]
    assert (r["ids"] == -7).all() and (r["lens"] == -7).all() and (r["n_hyp"] == -7).all() and (r["scores"] == 7.0).all()
    assert (r["counts"] == -7).all() and (r["ts"] == -7).all()
    r = s2.feed(dlp[:, 7:12], [5, 5, 5])
    ref = S.reference(lp, [12, 12, 7], 0, W, LABELS7)
    lp2 = lp.clone(); lp2[2, 2:7] = lp[2, 7:12]
    ref2 = S.reference(lp2, [12, 12, 7], 0, W, LABELS7)
    for k in S.KEYS:
        assert np.array_equal(r[k][:2], ref[k][:2]) and np.array_equal(r[k][2], ref2[k][2]), k


# ---- 10. module level ----
@pytest.mark.parametrize("keep", [False, True])
def test_module_stream(keep):
    from end2end_amd import CTCDecoder, DecoderResults, NBestResults
    from end2end_amd._runtime import E2EError
    import cpp_ctc_decoder
    g = torch.Generator().manual_seed(5)
    logits = (torch.randn(30, 4, 7, generator=g) * 2).to(U.dev())                 # time-major, raw logits
    xl = [30, 22, 9, 30]
    dec = CTCDecoder(beam_width=8, labels=LABELS7, time_major=True, after_logsoftmax=False, wip=1.0, keep_on_device=keep)
    whole = dec.decode_nbest(logits, torch.tensor(xl), nbest=5, timesteps=True)
    one = dec.decode(logits, torch.tensor(xl))
    st = dec.open_stream(4, 30, timesteps=True)
    plain = dec.open_stream(4, 30)
    side = torch.cuda.Stream(device=U.dev())
    side.wait_stream(torch.cuda.current_stream(U.dev()))
    with torch.cuda.stream(side):
        for a in range(0, 30, 8):
            n = min(8, 30 - a)
            lens = torch.tensor([max(0, min(x - a, n)) for x in xl])
            res = st.feed_nbest(logits[a:a + n], lens, nbest=5)
            first = plain.feed(logits[a:a + n], lens)
    side.synchronize()
    assert isinstance(res, NBestResults) and isinstance(first, DecoderResults)
    assert st.frames == xl and plain.frames == xl
    assert st.state.is_cuda and st.state.dtype == torch.uint8 and st.state.shape[0] == 4
    for t in (res.decoded_targets, res.decoded_targets_lengths, res.scores, res.num_hypotheses, res.timesteps, first.decoded_targets):
        assert t.is_cuda == keep
    for a, b in zip(res, whole):
        if torch.is_tensor(a):
            assert torch.equal(a.cpu(), b.cpu())
        else:
            assert a == b
    assert first.decoded_sentences == one.decoded_sentences == [row[0] for row in whole.decoded_sentences]
    assert torch.equal(first.decoded_targets.cpu(), one.decoded_targets.cpu())
    assert torch.equal(first.decoded_targets_lengths.cpu(), one.decoded_targets_lengths.cpu())
    # a reset row starts anew; the engine under the reference's name takes log-probabilities
    plain.reset([1])
    assert plain.frames == [30, 0, 9, 30]
    with pytest.raises(E2EError, match="utterance 0 would pass max_frames"):
        plain.feed(logits[:1], torch.tensor([1, 1, 0, 0]))                          # utterance 0 is full
    assert plain.frames == [30, 1, 9, 30]                                           # ... and the others advanced
    eng = cpp_ctc_decoder.CTCDecoder(0, 8, LABELS7, wip_=1.0).open_stream(4, 30)
    lp = torch.log_softmax(logits.transpose(0, 1), -1)
    out = None
    for a in (0, 15):
        out = eng.feed(lp[:, a:a + 15], torch.tensor([max(0, min(x - a, 15)) for x in xl]))
    assert out[2] == one.decoded_sentences and eng.frames == xl

