"""GPU: Gram-CTC decoding (e2e_gram_ctc_greedy, e2e_gram_ctc_beam_nbest through GramCTCDecoder) against enumeration of
all paths, against the test-side restatement of the search (tests/gram_decode_ref.py) and against the library's own
Gram-CTC loss."""
import math

import numpy as np
import pytest
import torch

import gram_decode_ref as DR
import gram_ref as GR

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def decoder(R, V, l2i, width, **kw):
    from end2end_amd.decoders import GramCTCDecoder
    return GramCTCDecoder(0, R, V, l2i, beam_width=width, after_logsoftmax=True, **kw)


def hyps_of(res, b):
    """[(sequence, score)] of utterance b of a GramNBestResults, and its lengths row."""
    n = int(res.num_hypotheses[b])
    lens = res.decoded_targets_lengths[b].tolist()
    ids = res.decoded_targets[b].tolist()
    return [(tuple(ids[j][:lens[j]]), float(res.scores[b, j])) for j in range(n)], lens


def check_empty_slots(res, b):
    n = int(res.num_hypotheses[b])
    assert (res.decoded_targets_lengths[b, n:] == 0).all() and (res.decoded_targets[b, n:] == 0).all()
    assert torch.isneginf(res.scores[b, n:]).all()
    for j in range(n):
        assert (res.decoded_targets[b, j, int(res.decoded_targets_lengths[b, j]):] == 0).all()


def gram_loss(R, V, l2i, lp, n_frames, seqs):
    """-log p(sequence) for every sequence, by the library's Gram-CTC loss on the GPU (reduce=False)."""
    from end2end_amd import GramCTCLoss
    S = max(max((len(s) for s in seqs), default=0), 1)
    tg = torch.ones((len(seqs), S), dtype=torch.long)
    for i, s in enumerate(seqs):
        tg[i, :len(s)] = torch.tensor(s, dtype=torch.long)
    tl = torch.tensor([len(s) for s in seqs])
    x = lp[None, :n_frames].expand(len(seqs), -1, -1).contiguous().to(DEV)
    loss = GramCTCLoss(0, R, V, l2i, reduce=False, after_logsoftmax=True)
    return loss(x, tg.to(DEV), torch.full((len(seqs),), n_frames).to(DEV), tl.to(DEV)).double().cpu().numpy()


# ---- 1. unpruned equals enumeration; 3b. and the loss -------------------------------------------------------------
@pytest.mark.parametrize("dt", [torch.float32, torch.float64])
def test_unpruned_beam_equals_enumeration_on_the_tiny_cases(dt):
    cases = DR.tiny_cases()
    ran = 0
    for i, (R, V, l2i, x) in enumerate(cases):
        lp = torch.log_softmax(torch.from_numpy(x).to(dt), -1)
        # (f64: the shared enumeration, whose log-softmax differs from torch's by rounding only; f32: the enumeration of
        #  the very f32 log-probabilities the search is given)
        enum = (DR.tiny_reference()[i] if dt == torch.float64
                else DR.enumerate_labellings(lp.double().numpy(), GR.grams_of(R, V, l2i)))
        want = {s: p for s, p in enum.items() if p > 0.0}
        if len(want) > 128:
            continue
        ran += 1
        res = decoder(R, V, l2i, 128).decode_nbest(lp[None].to(DEV), nbest=128)
        got, _ = hyps_of(res, 0)
        assert int(res.num_hypotheses[0]) == len(want)
        assert {s for s, _ in got} == set(want) and len(got) == len(want)
        for s, score in got:
            assert abs(math.exp(score) - want[s]) <= 1e-9 * want[s], (s, math.exp(score), want[s])
        best = max(want.values())
        assert want[got[0][0]] >= best * (1 - 1e-9)
        assert all(a[1] >= b[1] for a, b in zip(got, got[1:]))
        check_empty_slots(res, 0)
    assert ran >= 0.85 * len(cases)


def test_unpruned_scores_equal_the_loss_on_the_tiny_cases():
    """score = -GramCTCLoss(target = hypothesis).  Both sides are f64 sums of at most 4096 products of at most 6 factors:
    rounding leaves their logarithms some 1e-13 apart; the bound is the 1e-7 that the inequality of the pruned cases has."""
    for i, (R, V, l2i, x) in enumerate(DR.tiny_cases()):
        if len(DR.tiny_reference()[i]) > 128:                  # (the cases the unpruned test leaves out)
            continue
        lp = torch.log_softmax(torch.from_numpy(x), -1)
        res = decoder(R, V, l2i, 128).decode_nbest(lp[None].to(DEV), nbest=128)
        got, _ = hyps_of(res, 0)
        loss = gram_loss(R, V, l2i, lp, x.shape[0], [s for s, _ in got])
        for (s, score), l in zip(got, loss):
            assert abs(score + l) <= 1e-7, (s, score, -l)


# ---- 2. pruned equals the restatement; 3a. and never exceeds the loss ---------------------------------------------
def check_against_restatement(res, want_rows):
    for b, (want, _) in enumerate(want_rows):
        got, lens = hyps_of(res, b)
        assert int(res.num_hypotheses[b]) == len(want)
        assert [s for s, _ in got] == [s for s, _ in want], b
        assert lens[:len(want)] == [len(s) for s, _ in want]
        for (_, a), (_, w) in zip(got, want):
            assert abs(a - w) <= 1e-9 * max(1.0, abs(w)), (b, a, w)
        check_empty_slots(res, b)


@pytest.mark.parametrize("width", DR.PRUNED_WIDTHS)
def test_pruned_beam_equals_the_restatement(width):
    R, V, l2i, batches = DR.pruned_cases()
    ref = DR.pruned_reference()
    dec = decoder(R, V, l2i, width)
    for scale in DR.PRUNED_SCALES:
        x, xl = batches[(width, scale)]
        lp = torch.from_numpy(DR.log_softmax(x))
        if scale == DR.PRUNED_SCALES[0]:                       # one batch through a time-major view, one contiguous
            tm = lp.transpose(0, 1).contiguous().to(DEV)       # (T, B, V) in memory
            res = decoder(R, V, l2i, width, time_major=True).decode_nbest(tm, torch.from_numpy(xl).to(DEV))
        else:
            res = dec.decode_nbest(lp.to(DEV), torch.from_numpy(xl).to(DEV))
        check_against_restatement(res, ref[(width, scale)])
        # consistency with the loss: a pruned search can only have lost mass
        for b in range(len(xl)):
            got, _ = hyps_of(res, b)
            loss = gram_loss(R, V, l2i, lp[b], int(xl[b]), [s for s, _ in got])
            for (s, score), l in zip(got, loss):
                assert score <= -l + 1e-7, (width, scale, b, s, score, -l)


def test_pruned_beam_at_the_headline_table():
    R, V, l2i, x, xl, width = DR.headline_case()
    lp = torch.from_numpy(DR.log_softmax(x))
    res = decoder(R, V, l2i, width).decode_nbest(lp.to(DEV), torch.from_numpy(xl).to(DEV))
    check_against_restatement(res, DR.pruned_reference()["headline"])
    for b in range(2):
        got, _ = hyps_of(res, b)
        loss = gram_loss(R, V, l2i, lp[b], int(xl[b]), [s for s, _ in got])
        for (s, score), l in zip(got, loss):
            assert score <= -l + 1e-7, (b, s, score, -l)


# ---- 4. ties ------------------------------------------------------------------------------------------------------
def test_single_frame_ties_are_cut_by_key():
    R, V = 5, 9
    l2i = {5: [1, 2], 6: [2, 1], 7: [3, 3, 4], 8: [4, 1]}
    grams = GR.grams_of(R, V, l2i)
    lp = torch.log_softmax(torch.zeros(1, 1, V, dtype=torch.float64), -1)
    res = decoder(R, V, l2i, 4).decode_nbest(lp.to(DEV))
    got, _ = hyps_of(res, 0)
    want = sorted([()] + [grams[c] for c in range(1, V)], key=DR.key_of)[:4]
    assert [s for s, _ in got] == want
    assert all(abs(score - math.log(1.0 / V)) <= 1e-12 for _, score in got)


def test_all_equal_logits_decode_the_same_bits_twice():
    R, V, l2i, _ = DR.pruned_cases()[:4]
    lp = torch.log_softmax(torch.zeros(2, 12, V), -1).to(DEV)
    dec = decoder(R, V, l2i, 16, keep_on_device=True)
    a, b = dec.decode_nbest(lp), dec.decode_nbest(lp)
    for u, v in zip(a, b):
        if torch.is_tensor(u):
            assert u.shape == v.shape and torch.equal(u.cpu().view(torch.uint8), v.cpu().view(torch.uint8))
        else:
            assert u == v
    assert int(a.num_hypotheses[0]) == 16


@pytest.mark.parametrize("T", [2, 3])
def test_multi_frame_ties_equal_the_restatement(T):
    """All-equal log-probabilities at width 16: the cut of every frame is decided by keys.  Frame 0 cuts the equal
    single-share candidates of a beam that is not full (the key select with the floor filter off), the later frames cut
    those of a full beam (with it on); at T = 2 the restatement keeps 8 hypotheses at -4.990432586779 and 8 at
    -5.395897694887."""
    R, V, l2i, _ = DR.pruned_cases()
    lp = torch.log_softmax(torch.zeros(1, T, V, dtype=torch.float64), -1)
    want = DR.beam_search(lp[0].numpy(), GR.grams_of(R, V, l2i), 16)
    assert len(want[0]) == 16
    res = decoder(R, V, l2i, 16).decode_nbest(lp.to(DEV))
    check_against_restatement(res, [want])


# ---- 5. edges -----------------------------------------------------------------------------------------------------
def _edge_inputs(B, T, seed):
    R, V, l2i, _ = DR.pruned_cases()
    x = torch.from_numpy(np.random.default_rng(seed).normal(size=(B, T, V)) * 2.0)
    return R, V, l2i, x


def test_a_column_of_probability_zero_is_in_no_hypothesis():
    R, V, l2i, x = _edge_inputs(3, 20, 11)
    banned = 3                                                 # the unigram 3; no other gram may then supply a 3 either
    x[:, :, [c for c in range(1, V) if banned in GR.grams_of(R, V, l2i)[c]]] = -math.inf
    lp = torch.log_softmax(x, -1)
    res = decoder(R, V, l2i, 32).decode_nbest(lp.to(DEV))
    for b in range(3):
        got, _ = hyps_of(res, b)
        assert len(got) == 32 and all(banned not in s for s, _ in got)
        want, _ = DR.beam_search(lp[b].numpy(), GR.grams_of(R, V, l2i), 32)
        assert [s for s, _ in got] == [s for s, _ in want]


def test_lengths_of_zero_one_and_all_frames():
    R, V, l2i, x = _edge_inputs(3, 25, 12)
    lp = torch.log_softmax(x, -1)
    xl = torch.tensor([0, 1, 25])
    res = decoder(R, V, l2i, 8).decode_nbest(lp.to(DEV), xl.to(DEV))
    got, lens = hyps_of(res, 0)
    assert got == [((), 0.0)] and lens == [0] * 8
    check_empty_slots(res, 0)
    grams = GR.grams_of(R, V, l2i)
    for b in (1, 2):
        want, _ = DR.beam_search(lp[b, :int(xl[b])].numpy(), grams, 8)
        got, _ = hyps_of(res, b)
        assert [s for s, _ in got] == [s for s, _ in want]
        assert all(abs(a[1] - w[1]) <= 1e-9 * max(1.0, abs(w[1])) for a, w in zip(got, want))


def test_nbest_below_the_width_is_the_head_of_the_list():
    R, V, l2i, x = _edge_inputs(2, 30, 13)
    lp = torch.log_softmax(x, -1).to(DEV)
    dec = decoder(R, V, l2i, 32)
    full, head = dec.decode_nbest(lp), dec.decode_nbest(lp, nbest=5)
    assert head.decoded_targets.shape[1] == 5 and head.num_hypotheses.tolist() == [5, 5]
    for b in range(2):
        assert hyps_of(head, b)[0] == hyps_of(full, b)[0][:5]
    one = dec.decode(lp)
    for b in range(2):
        n = int(one.decoded_targets_lengths[b])
        assert tuple(one.decoded_targets[b, :n].tolist()) == hyps_of(full, b)[0][0][0]


def test_max_out_too_small_reports_the_needed_length():
    from end2end_amd import _C
    from end2end_amd.engines import GramCTCDecoderEngine
    R, V, l2i, x = _edge_inputs(2, 30, 14)
    lp = torch.log_softmax(x, -1).to(DEV)
    eng = GramCTCDecoderEngine(0, R, V, l2i, 8)
    full = eng.decode_nbest(lp, torch.tensor([30, 30]))
    ids, lens = eng._table(DEV)
    B, T, N, max_out = 2, 30, 8, 3
    assert int(full[1].max()) > max_out
    out = torch.full((B, N, max_out), -7, dtype=torch.long, device=DEV)
    out_len = torch.empty((B, N), dtype=torch.long, device=DEV)
    n_hyp = torch.empty(B, dtype=torch.long, device=DEV)
    scores = torch.empty((B, N), dtype=torch.float64, device=DEV)
    ws = torch.empty(_C.gram_beam_workspace_bytes(B, T, V, eng.max_order, 8), dtype=torch.uint8, device=DEV)
    xl = torch.tensor([30, 30], device=DEV)
    _C.gram_ctc_beam_nbest(lp.data_ptr(), _C.F64, *lp.stride(), xl.data_ptr(), B, T, V, ids.data_ptr(), lens.data_ptr(),
                           eng.max_order, 8, N, out.data_ptr(), max_out, out_len.data_ptr(), n_hyp.data_ptr(),
                           scores.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream(DEV).cuda_stream)
    assert torch.equal(out_len.cpu(), full[1]) and torch.equal(scores.cpu(), full[3])
    want = torch.zeros((B, N, max_out), dtype=torch.long)
    w = min(max_out, full[0].shape[2])
    want[:, :, :w] = full[0][:, :, :w]
    assert torch.equal(out.cpu(), want)


def test_a_width_above_the_limit_raises_before_any_launch():
    from end2end_amd import _C
    cap = _C.gram_beam_max_width(21, 8)
    z = torch.zeros(8, dtype=torch.long, device=DEV)
    with pytest.raises(_C.E2EError, match="beam_width"):       # (addresses that no kernel may touch: the host refuses first)
        _C.gram_ctc_beam_nbest(z.data_ptr(), _C.F32, 0, 0, 0, z.data_ptr(), 1, 1, 21, z.data_ptr(), z.data_ptr(), 8,
                               cap + 1, 1, z.data_ptr(), 1, z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), 0, 0)
    with pytest.raises(ValueError, match="beam_width"):
        decoder(6, 21, DR.pruned_cases()[2], cap + 1)


def test_a_batch_of_seventy_utterances_keeps_its_workspaces_apart():
    R, V, l2i, x = _edge_inputs(5, 16, 15)
    lp = torch.log_softmax(x, -1)
    idx = [i % 5 for i in range(70)]
    xl = torch.tensor([16 - (i // 5) % 4 for i in range(70)])
    res = decoder(R, V, l2i, 16).decode_nbest(lp[idx].to(DEV), xl.to(DEV))
    grams = GR.grams_of(R, V, l2i)
    seen = {}
    for b in range(70):
        k = (idx[b], int(xl[b]))
        if k not in seen:
            seen[k] = DR.beam_search(lp[idx[b], :int(xl[b])].numpy(), grams, 16)[0]
        got, _ = hyps_of(res, b)
        assert [s for s, _ in got] == [s for s, _ in seen[k]], b
        assert all(abs(a[1] - w[1]) <= 1e-9 * max(1.0, abs(w[1])) for a, w in zip(got, seen[k]))


# ---- 6. greedy ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [torch.float32, torch.float64, torch.bfloat16])
def test_greedy_equals_its_definition(dt):
    R, V, l2i, _ = DR.pruned_cases()
    grams = GR.grams_of(R, V, l2i)
    g = torch.Generator().manual_seed(21)
    B, T = 8, 200
    x = (torch.randn(B, T, V, generator=g) * 2).to(dt)
    xl = torch.randint(100, T + 1, (B,), generator=g)
    xl[0], xl[1] = T, 1
    from end2end_amd.decoders import GramCTCDecoder
    dec = GramCTCDecoder(0, R, V, l2i, beam_width=1, labels=["_", "a", "b", "c", "d", "e"])
    res = dec.decode_greedy(x.to(DEV), xl.to(DEV), return_columns=True)
    assert res.decoded_targets.shape == (B, T * 8) and res.columns.shape == (B, T)
    assert dec.decode(x.to(DEV), xl.to(DEV)).decoded_sentences == res.decoded_sentences
    xs = x.float().numpy() if dt == torch.bfloat16 else x.numpy()      # (bf16 -> f32 is exact: the same arg-max)
    for b in range(B):
        ids, cols = DR.greedy(xs[b], int(xl[b]), grams)
        n, m = int(res.decoded_targets_lengths[b]), int(res.columns_lengths[b])
        assert res.decoded_targets[b, :n].tolist() == ids and (res.decoded_targets[b, n:] == 0).all()
        assert res.columns[b, :m].tolist() == cols and (res.columns[b, m:] == 0).all()
        # the returned segmentation expands to the ids
        assert [i for c in res.columns[b, :m].tolist() for i in grams[c]] == res.decoded_targets[b, :n].tolist()
        assert res.decoded_sentences[b] == "".join("_abcde"[i] for i in ids)


def test_greedy_with_unigrams_only_is_the_ctc_greedy_decode():
    from end2end_amd.decoders import GramCTCDecoder
    from end2end_amd.engines import CTCDecoderEngine
    g = torch.Generator().manual_seed(22)
    B, T, V = 6, 300, 29
    x = torch.randn(B, T, V, generator=g).to(DEV)
    xl = torch.randint(150, T + 1, (B,), generator=g).to(DEV)
    a = GramCTCDecoder(0, V, V, {}, beam_width=1).decode_greedy(x, xl)
    b = CTCDecoderEngine(0, 1).decode_greedy(x, xl)
    assert torch.equal(a.decoded_targets, b[0]) and torch.equal(a.decoded_targets_lengths, b[1])
