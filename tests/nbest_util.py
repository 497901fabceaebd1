"""Helpers of the n-best tests: the raw C-ABI call e2e_ctc_beam_nbest on device tensors, and -- oracle only, no GPU -- the
likelihood of every labelling of a tiny utterance."""
import itertools

import numpy as np
import torch

import golden_util as G
import oracle_lib as O

ATOL = 1e-9      # f64 against f64: a few thousand log-sum-exps of relative error ~1e-16 on magnitudes below 1e4


def c_abi_beam_nbest(lp, x_len=None, blank=0, beam_width=100, labels=None, lm=None, lmwt=1.0, wip=0.0, oov_penalty=-1000.0,
                     nbest=None, timesteps=False, max_out=None, check_status=True):
    """Raw C-ABI n-best read-out on log-probs -> dict of numpy arrays: ids (B,N,max_out), lens (B,N), n_hyp (B), scores (B,N,3),
    counts (B,N,2), ts (B,N,max_out) or None.  Every output starts as garbage, so what the call leaves unwritten shows."""
    from end2end_amd import _lib
    import gpu_util as U
    L = _lib.load()
    d = U.dev()
    if not lp.is_cuda:
        base = lp
        lp = torch.empty_strided(base.shape, base.stride(), dtype=base.dtype, device=d)
        lp.copy_(base)
    B, T, V = lp.shape
    if x_len is None:
        x_len = [T] * B
    xl = torch.as_tensor(np.asarray(x_len)).to(d, torch.long)
    labels = list(labels or [])
    space_id = labels.index(" ") if " " in labels else -1
    N = beam_width if nbest is None else nbest
    max_out = T + 1 if max_out is None else max_out
    out = torch.full((B, N, max_out), -7, dtype=torch.long, device=d)
    out_len = torch.full((B, N), -7, dtype=torch.long, device=d)
    n_hyp = torch.full((B,), -7, dtype=torch.long, device=d)
    scores = torch.full((B, N, 3), 7.0, dtype=torch.float64, device=d)
    counts = torch.full((B, N, 2), -7, dtype=torch.int32, device=d)
    ts = torch.full((B, N, max_out), -7, dtype=torch.long, device=d) if timesteps else None
    n = L.e2e_ctc_beam_nbest_workspace_bytes(B, T, V, beam_width, 1 if lm is not None else 0, 1 if timesteps else 0)
    ws = torch.empty(n, dtype=torch.uint8, device=d)
    sB, sT, sV = lp.stride()
    _lib.check(L.e2e_ctc_beam_nbest(lp.data_ptr(), _lib.dtype_code(lp.dtype), sB, sT, sV, xl.data_ptr(), B, T, V, blank,
                                    beam_width, space_id, lm.on(d).handle if lm is not None else None, lmwt, wip, oov_penalty,
                                    N, out.data_ptr(), max_out, out_len.data_ptr(), n_hyp.data_ptr(), scores.data_ptr(),
                                    counts.data_ptr(), ts.data_ptr() if timesteps else None,
                                    ws.data_ptr(), ws.numel(), _lib.stream_ptr(d)))
    torch.cuda.synchronize()
    r = dict(ids=out.cpu().numpy(), lens=out_len.cpu().numpy(), n_hyp=n_hyp.cpu().numpy(), scores=scores.cpu().numpy(),
             counts=counts.cpu().numpy(), ts=ts.cpu().numpy() if timesteps else None)
    if check_status:
        assert (r["n_hyp"] >= 1).all() and (r["n_hyp"] <= N).all(), r["n_hyp"]
        assert ((r["lens"] >= 0) & (r["lens"] <= max_out)).all(), r["lens"]
    return r


def hypothesis(r, b, h):
    """The label sequence of hypothesis h of utterance b as a tuple; the empty winner's single -1 (quirk Q6) is ()."""
    seq = tuple(int(k) for k in r["ids"][b, h, : r["lens"][b, h]])
    return () if seq == (-1,) else seq


def loglik(lp, seqs, blank, x_len=None):
    """log P(labelling | lp) for every labelling of `seqs`, by the oracle's CTC loss.  lp: (T,V) f64."""
    lp = np.asarray(lp, dtype=np.float64)
    T = lp.shape[0] if x_len is None else int(x_len)
    n = len(seqs)
    width = max(1, max(len(s) for s in seqs))
    tg = np.zeros((n, width), dtype=np.int64)
    for i, s in enumerate(seqs):
        tg[i, : len(s)] = s
    losses, _ = O.ctc_loss(np.broadcast_to(lp, (n,) + lp.shape), tg, [T] * n, [len(s) for s in seqs], blank)
    return -losses


def all_labellings(T, V, blank):
    syms = [c for c in range(V) if c != blank]
    return [s for n in range(T + 1) for s in itertools.product(syms, repeat=n)]


_exhaustive = None


def exhaustive_cases():
    """The brute-force goldens that a one-launch n-best can be held to exactly (T <= 7, V <= 4, width = number of labellings in
    63..255: nothing is ever pruned), each with `seqs` / `ll`: its labellings and their oracle likelihoods, most likely first.
    The order of two neighbours is only checkable when their likelihoods differ by more than 1e-6 (`gap_ok`); a case in which
    fewer than 90 % of the neighbouring finite pairs do -- the flat-emission goldens -- gets seeded random emissions of the same size
    instead (`replaced`)."""
    global _exhaustive
    if _exhaustive is not None:
        return _exhaustive
    cases = []
    for c in G.beam_bruteforce_cases():
        if not (c["T"] <= 7 and c["V"] <= 4 and 63 <= c["beam_width"] <= 255):
            continue
        c = dict(c)
        c["lp"] = np.array(c["log_probs"], dtype=np.float64)
        c["replaced"] = False
        for attempt in range(2):
            seqs = all_labellings(c["T"], c["V"], c["blank"])
            assert len(seqs) == c["beam_width"]
            ll = loglik(c["lp"], seqs, c["blank"])
            order = sorted(range(len(seqs)), key=lambda i: -ll[i])
            c["seqs"] = [seqs[i] for i in order]
            c["ll"] = ll[order]
            fin = c["ll"][np.isfinite(c["ll"])]
            c["gap_fraction"] = float((fin[:-1] - fin[1:] > 1e-6).mean())
            if c["gap_fraction"] >= 0.9:
                break
            assert attempt == 0, (c["name"], c["gap_fraction"])
            g = torch.Generator().manual_seed(1000 + len(cases))
            c["lp"] = torch.log_softmax(torch.randn(c["T"], c["V"], generator=g, dtype=torch.float64) * 2.0, -1).numpy()
            c["replaced"] = True
        cases.append(c)
    _exhaustive = cases
    return cases


EXHAUSTIVE_NAMES = [c["name"] for c in G.beam_bruteforce_cases() if c["T"] <= 7 and c["V"] <= 4 and 63 <= c["beam_width"] <= 255]


def num_words(seq, space_id):
    """Words of a label sequence: maximal runs of non-space labels."""
    n, inside = 0, False
    for k in seq:
        if k == space_id:
            inside = False
        elif not inside:
            n, inside = n + 1, True
    return n
