"""-m gpu: ASGDecoder's per-frame label pruning (cutoff_top_n; e2e_asg_beam_nbest_cut and e2e_asg_beam_stream_cut, the
definition in include/e2e_ctc.h).

1. A pruned call equals, bit for bit in every output, the unpruned call on emissions whose non-kept columns the HOST set to
   -inf (asg_cut_ref.masked: a stable descending sort, the lower id on ties, NaN as -inf).  Both calls go through the C ABI,
   the pruned one with a garbage-filled workspace of exactly the queried size.
2. cutoff_top_n >= V is the unpruned call.
3. The beam dies: n_hyp = 0, the stream's header says dead and stays so.
4. Streams: after every chunk of any chunking the read-out is the whole pruned call's, bit for bit; reset(rows).
5. Time-major and strided views give the contiguous result.
6. Refusals before any launch.
7. The kept-loop restatement (tests/asg_cut_ref.py), for the utterances whose margin allows it.
8. ASGDecoder.prune: decode, decode_nbest, streams equal the C-ABI results; prune(None) and configure() give the unpruned ones.
The cases, the restatement and what is left out of 7 are tests/asg_cut_ref.py's; tests/test_asg_cut_cpu.py checks them."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import asg_cut_ref as CR
import asg_stream_util as S
import gpu_util as U

pytestmark = pytest.mark.gpu

TOL = 1e-9                                       # tests/test_gpu_asg_beam.py's, against the restatement
DTYPES = {"f32": torch.float32, "f64": torch.float64}
MODEL_PATH = os.path.join(CR.BU.GOLDEN, CR.MODEL)
ERR_ARG, ERR_UNSUPPORTED, ERR_WORKSPACE = -1, -2, -3
GUARD, FILL = 4096, 0xAB


@functools.lru_cache(maxsize=None)
def model(shape, kind):
    from end2end_amd.engines import LanguageModel
    labels = CR.labels_of(shape)
    if kind == "words":
        return LanguageModel(None, labels, True, words=CR.WORDS, lexicon=True)
    lm = LanguageModel(MODEL_PATH, labels, True)
    if kind == "lexicon":
        lm.enable_lexicon()
    return lm


def search(shape, inst):
    """The C arguments of an instance -> dict(R, W, space, lm, restrict, lmwt, wip, oov_penalty, timesteps)."""
    B, T, V, R, W, K = CR.SHAPES[shape]
    s = dict(R=R, W=W, space=CR.chars_of(shape).index(" "), lm=None, restrict=inst in ("lex_lm", "lex_words"), lmwt=0.0, wip=0.0,
             oov_penalty=0.0, timesteps=inst in ("wip", "lex_lm", "timesteps"))
    if inst in ("wip", "lex_words"):
        s["wip"] = 0.4
    if inst in ("lm", "lex_lm", "timesteps"):
        s.update(lm=model(shape, "lexicon" if inst == "lex_lm" else "arpa"), **CR.KNOBS)
    if inst == "lex_words":
        s["lm"] = model(shape, "words")
    return s


def whole(x, A, x_len, s, top_n=None, nbest=None, expect_rc=0, outputs=None, short=0):
    """The whole call through the C ABI -> dict of numpy arrays (outputs start as garbage).  top_n None:
    e2e_asg_beam_nbest_opt (asg_stream_util.reference); else e2e_asg_beam_nbest_cut with a garbage-filled workspace of exactly
    the queried size between two guards (short: that many bytes less than the call needs at the pointer's alignment)."""
    if top_n is None:
        return S.reference(x, A, x_len, s["R"], s["W"], s["space"], s["lm"], s["restrict"], s["lmwt"], s["wip"], s["oov_penalty"],
                           nbest=nbest, timesteps=s["timesteps"])
    from end2end_amd import _lib
    L, d = _lib.load(), U.dev()
    if not x.is_cuda:
        x = x.to(d)
    B, T, V = x.shape
    xl = torch.as_tensor(np.asarray(x_len)).to(d, torch.long)
    N = s["W"] if nbest is None else nbest
    o = S.garbage(B, N, T, d, s["timesteps"]) if outputs is None else outputs
    At = S.transitions(A, x.dtype, d)
    need = L.e2e_asg_beam_cut_workspace_bytes(B, T, V, s["W"], 1 if s["lm"] is not None else 0, top_n)
    buf = torch.full((GUARD + max(need, 256) + GUARD,), FILL, dtype=torch.uint8, device=d)
    assert buf.data_ptr() % 256 == 0
    opts = _lib.AsgBeamOpts(1 if s["restrict"] else 0, o["ts"].data_ptr() if s["timesteps"] else None)
    given = need - 257 - short + 1 if short else need            # (the query's 256 bytes of slack are for the pointer's alignment)
    rc = L.e2e_asg_beam_nbest_cut(x.data_ptr(), _lib.dtype_code(x.dtype), *x.stride(), At.data_ptr() if At is not None else None,
                                  xl.data_ptr(), B, T, V, s["R"], s["W"], s["space"],
                                  s["lm"].on(d).handle if s["lm"] is not None else None, s["lmwt"], s["wip"], s["oov_penalty"],
                                  N, o["out"].data_ptr(), T, o["out_len"].data_ptr(), o["n_hyp"].data_ptr(), o["scores"].data_ptr(),
                                  o["counts"].data_ptr(), buf.data_ptr() + GUARD, given, _lib.stream_ptr(d), C.byref(opts), top_n)
    assert rc == expect_rc, (rc, L.e2e_last_error())
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == FILL).all()) and bool((buf[GUARD + max(need, 256):] == FILL).all())
    r = S.host(o)
    r["need"] = need
    return r


def tensors(shape, kind, dtype):
    x, A, lens = CR.case(shape, kind)
    K = CR.SHAPES[shape][5]
    xd = torch.from_numpy(x).to(DTYPES[dtype]).to(U.dev())
    xm = torch.from_numpy(CR.masked(x, K)).to(DTYPES[dtype]).to(U.dev())
    return xd, xm, (torch.from_numpy(A) if A is not None else None), lens


def untouched(r, b):
    return r["n_hyp"][b] == 0 and (r["lens"][b] == -7).all() and (r["ids"][b] == -7).all()


# ---- 1. masked equivalence, bit for bit ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("inst", CR.INSTANCES)
@pytest.mark.parametrize("shape", range(len(CR.SHAPES)))
def test_pruned_call_equals_the_unpruned_call_on_masked_emissions(shape, inst, dtype):
    B, T, V, R, W, K = CR.SHAPES[shape]
    s = search(shape, inst)
    alive = 0
    for kind in CR.KINDS:
        x, xm, A, lens = tensors(shape, kind, dtype)
        got = whole(x, A, lens, s, top_n=K)
        want = whole(xm, A, lens, s)
        S.same(got, want, (shape, inst, dtype, kind))
        for b, n in enumerate(lens):
            if not 1 <= n <= T:                      # lengths 0 and T + 1: n_hyp = 0 and nothing else is written
                assert untouched(got, b), (shape, kind, b)
            else:
                alive += int(got["n_hyp"][b] > 0)
    # (a restricted search may die in every utterance: a frame whose kept labels continue no word of the vocabulary ends it)
    assert alive > 0 or s["restrict"]


# ---- 2. no pruning is the unpruned call -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("inst", ["plain", "lex_lm"])
def test_no_pruning_is_the_unpruned_call(inst):
    from end2end_amd import _lib
    L = _lib.load()
    shape = 0
    B, T, V, R, W, K = CR.SHAPES[shape]
    s = search(shape, inst)
    x, _, A, lens = tensors(shape, "randn", "f64")
    want = whole(x, A, lens, s)
    for top_n in (V, V + 5):
        got = whole(x, A, lens, s, top_n=top_n)
        S.same(got, want, (inst, top_n))
        with_lm = 1 if s["lm"] is not None else 0
        assert got["need"] == L.e2e_asg_beam_workspace_bytes(B, T, V, W, with_lm)
        assert L.e2e_asg_beam_cut_stream_workspace_bytes(B, T, V, W, with_lm, top_n) == L.e2e_asg_beam_stream_workspace_bytes(B, V, W, with_lm)
        st = CutStream(B, T, V, s, top_n, A)
        S.same(st.feed(x, [min(n, T) for n in lens]), whole(x, A, [min(n, T) for n in lens], s), (inst, top_n, "stream"))


# ---- 4 (the raw stream; 3 uses it) ------------------------------------------------------------------------------------------------
class CutStream:
    """B state rows and the raw call e2e_asg_beam_stream_cut (asg_stream_util.RawStream with the knob); the workspace is
    garbage of exactly the queried size."""

    def __init__(self, B, max_frames, V, s, top_n, A=None):
        from end2end_amd import _lib
        self._lib, self.L, self.d = _lib, _lib.load(), U.dev()
        self.B, self.max_frames, self.V, self.s, self.top_n, self.A = B, max_frames, V, s, top_n, A
        self.row_bytes = self.L.e2e_asg_beam_stream_row_bytes(max_frames, V, s["W"], 1 if s["lm"] is not None else 0)
        assert self.row_bytes > 0 and self.row_bytes % 256 == 0
        g = torch.Generator().manual_seed(12345)
        self.state = torch.randint(0, 256, (B, self.row_bytes), generator=g, dtype=torch.uint8).to(self.d)
        self.state[:, :S.HEADER] = 0

    def header(self, b):
        """(n, frames, dead) of row b's header."""
        h = self.state[b, :S.HEADER].cpu().numpy().view(np.int32)
        return int(h[6]), int(h[7]), int(h[8])

    def feed(self, chunk, chunk_len):
        _lib, L, d, s = self._lib, self.L, self.d, self.s
        if not chunk.is_cuda:
            chunk = chunk.to(d)
        B, Tc, V = chunk.shape
        cl = torch.as_tensor(np.asarray(chunk_len)).to(d, torch.long)
        o = S.garbage(B, s["W"], self.max_frames, d, s["timesteps"])
        done = torch.full((B,), -77, dtype=torch.long, device=d)
        At = S.transitions(self.A, chunk.dtype, d)
        need = L.e2e_asg_beam_cut_stream_workspace_bytes(B, Tc, V, s["W"], 1 if s["lm"] is not None else 0, self.top_n)
        assert need > 0
        ws = torch.full((need,), FILL, dtype=torch.uint8, device=d)
        opts = _lib.AsgBeamOpts(1 if s["restrict"] else 0, o["ts"].data_ptr() if s["timesteps"] else None)
        rc = L.e2e_asg_beam_stream_cut(chunk.data_ptr(), _lib.dtype_code(chunk.dtype), *chunk.stride(),
                                       At.data_ptr() if At is not None else None, cl.data_ptr(), B, Tc, V, s["R"], s["W"], s["space"],
                                       s["lm"].on(d).handle if s["lm"] is not None else None, s["lmwt"], s["wip"], s["oov_penalty"],
                                       self.state.data_ptr(), self.row_bytes, self.max_frames, s["W"], o["out"].data_ptr(),
                                       self.max_frames, o["out_len"].data_ptr(), o["n_hyp"].data_ptr(), o["scores"].data_ptr(),
                                       o["counts"].data_ptr(), done.data_ptr(), ws.data_ptr(), need, _lib.stream_ptr(d),
                                       C.byref(opts), self.top_n)
        assert rc == 0, (rc, L.e2e_last_error())
        torch.cuda.synchronize()
        r = S.host(o)
        r["done"] = done.cpu().numpy()
        return r


# ---- 3. the beam dies ---------------------------------------------------------------------------------------------------------------
def test_the_beam_dies():
    # V = 3: a, the space, one repeat label; K = 1
    s = dict(R=1, W=4, space=1, lm=None, restrict=False, lmwt=0.0, wip=0.0, oov_penalty=0.0, timesteps=True)
    d = U.dev()
    T = 6
    # utterance 0: the repeat label is the top of frame 0 -- nothing can begin with it.  Utterance 1: frame 0 keeps the space,
    # frame 2 the repeat label alone, which may not follow a space, and the space itself is dropped: no stay.  Utterance 2 lives.
    x = torch.zeros((3, T, 3), dtype=torch.float64)
    x[0, :, 2] = 3.0
    x[1, :, 1] = 3.0
    x[1, 2, 2] = 5.0
    x[2, :, 0] = 3.0
    x[2, 3, 1] = 4.0
    x = x.to(d)
    lens = [T, T, T]
    got = whole(x, None, lens, s, top_n=1)
    xm = torch.from_numpy(CR.masked(x.cpu().numpy(), 1)).to(d)
    S.same(got, whole(xm, None, lens, s), "dies")
    assert got["n_hyp"].tolist() == [0, 0, 1]
    assert got["ids"][2, 0, :got["lens"][2, 0]].tolist() == [0, 1, 0]
    # the stream: dead after the chunk with frame 2, and later chunks leave it so
    st, ref = CutStream(3, T, 3, s, 1), S.RawStream(3, T, 3, 1, 4, 1, timesteps=True)
    for a, b in ((0, 2), (2, 4), (4, 6)):
        r = st.feed(x[:, a:b], [b - a] * 3)
        S.same(r, ref.feed(xm[:, a:b], [b - a] * 3), ("dies, stream", a))
        assert r["done"].tolist() == [b] * 3
        assert st.header(0) == (0, b, 1)
        assert st.header(1) == ((1, b, 0) if b <= 2 else (0, b, 1))
        assert st.header(2)[2] == 0 and r["n_hyp"][2] == 1
        S.same(r, whole(x, None, [b] * 3, s, top_n=1), ("dies, whole", b))


# ---- 4. streams -----------------------------------------------------------------------------------------------------------------------
def chunkings(x_len, T):
    x_len = [min(max(n, 0), T) for n in x_len]
    one = S.regular(x_len, T, 1)
    uneven = S.cuts(x_len, [5, 1, 7, 3] + [T])
    first = [min(4, n) for n in x_len]
    rest = [n - f for n, f in zip(x_len, first)]
    with_empty = [first, [0] * len(x_len), [0] + rest[1:], [rest[0]] + [0] * (len(x_len) - 1)]   # a zero-frame chunk for one utterance
    return x_len, (one, uneven, with_empty)


def feed_and_compare(x, A, x_len, chunking, s, top_n, cache):
    B, T, V = x.shape
    st = CutStream(B, T, V, s, top_n, A)
    fed = [0] * B
    for lens in chunking:
        Tc = max(max(lens), 1)
        chunk = torch.zeros((B, Tc, V), dtype=x.dtype, device=x.device)
        for b in range(B):
            chunk[b, :lens[b]] = x[b, fed[b]:fed[b] + lens[b]]
        r = st.feed(chunk, lens)
        fed = [fed[b] + lens[b] for b in range(B)]
        assert r["done"].tolist() == fed
        key = tuple(fed)
        if key not in cache:
            cache[key] = whole(x, A, fed, s, top_n=top_n)
        for b in range(B):
            if fed[b] == 0:                          # fed nothing yet: the row and the outputs are not touched (as the whole call)
                assert r["n_hyp"][b] == 0
        S.same(r, cache[key], (key, top_n))


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("inst", ["plain", "lm", "lex_lm", "lex_words"])
def test_stream_equals_the_whole_pruned_call_after_every_chunk(inst, dtype):
    for shape in (0, 1):
        B, T, V, R, W, K = CR.SHAPES[shape]
        x, _, A, lens = tensors(shape, "randn", dtype)
        s, cache = search(shape, inst), {}
        lens, cks = chunkings(lens, T)
        for chunking in cks:
            assert [sum(c[b] for c in chunking) for b in range(B)] == lens
            feed_and_compare(x, A, lens, chunking, s, K, cache)


# ---- 5. views -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["time_major", "strided"])
@pytest.mark.parametrize("inst", ["plain", "lex_lm"])
def test_views_give_the_contiguous_result(inst, layout):
    for shape, dtype in ((1, "f32"), (4, "f64")):
        B, T, V, R, W, K = CR.SHAPES[shape]
        x, _, A, lens = tensors(shape, "half", dtype)
        s = search(shape, inst)
        want = whole(x, A, lens, s, top_n=K)
        v = S.view_of(x, layout)
        assert v.stride() != x.stride()
        S.same(whole(v, A, lens, s, top_n=K), want, (inst, layout, shape))
        inside = [min(n, T) for n in lens]
        st = CutStream(B, T, V, s, K, A)
        S.same(st.feed(v, inside), whole(x, A, inside, s, top_n=K), (inst, layout, shape, "stream"))


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch():
    shape = 1
    B, T, V, R, W, K = CR.SHAPES[shape]
    s = search(shape, "lm")
    x, _, A, lens = tensors(shape, "randn", "f32")

    def refused(x, top_n, rc, **kw):
        o = S.garbage(B, W, T, U.dev(), s["timesteps"])
        before = {k: v.clone() for k, v in o.items() if v is not None}
        whole(x, A, lens, s, top_n=top_n, expect_rc=rc, outputs=o, **kw)
        assert all(torch.equal(o[k], v) for k, v in before.items())          # the outputs are still garbage
    refused(x, 0, ERR_ARG)
    refused(x, -1, ERR_ARG)
    refused(x, K, ERR_WORKSPACE, short=1)                                    # one byte less than the call needs
    big = torch.zeros((B, T, 129), device=U.dev())
    refused(big, K, ERR_UNSUPPORTED)
    refused(big, 200, ERR_UNSUPPORTED)
    want = whole(x, A, lens, s, top_n=K)                                     # ... and the exact size is enough (whole() passes it)
    assert (want["n_hyp"] >= 1).all()


# ---- 7. the restatement -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,inst", CR.ORACLE)
def test_pruned_call_equals_the_kept_loop_restatement(shape, inst):
    B, T, V, R, W, K = CR.SHAPES[shape]
    x, _, A, lens = tensors(shape, "randn", "f64")
    s = search(shape, inst)
    got = whole(x, A, lens, s, top_n=K)
    ranking, gaps = CR.oracle_reference(shape, inst)
    compared = 0
    for b, n in enumerate(lens):
        if not 1 <= n <= T:
            assert untouched(got, b)
            continue
        if (shape, inst, b) in CR.LEFT_OUT:
            continue
        assert gaps[b] >= CR.MIN_GAP
        compared += 1
        want = ranking[b]
        assert got["n_hyp"][b] == len(want), (shape, inst, b)
        for j, r in enumerate(want):
            m = int(got["lens"][b, j])
            assert tuple(got["ids"][b, j, :m].tolist()) == r["ids"], (shape, inst, b, j)
            for g, k in zip(got["scores"][b, j], ("total", "ac", "lm")):
                assert abs(float(g) - r[k]) <= TOL * max(1.0, abs(r[k])), (shape, inst, b, j, k, float(g), r[k])
            assert tuple(got["counts"][b, j].tolist()) == (r["words"], r["oov"]), (shape, inst, b, j)
    assert compared >= 2


# ---- 8. the Python surface --------------------------------------------------------------------------------------------------------------
def decoder(shape, inst):
    from end2end_amd import ASGDecoder
    B, T, V, R, W, K = CR.SHAPES[shape]
    d = ASGDecoder(labels=CR.chars_of(shape), num_replabels=R)
    if inst == "lm":
        return d.configure(beam_width=W, lm_path=MODEL_PATH, **CR.KNOBS)
    return d.configure(beam_width=W, wip=0.0)


@pytest.mark.parametrize("inst", ["plain", "lm"])
def test_decoder_prune(inst, monkeypatch):
    shape = 1
    B, T, V, R, W, _ = CR.SHAPES[shape]
    K = 3                                            # (the shape's own 10 of 29 leaves these utterances' 16 best as they are)
    x, _, A, lens = tensors(shape, "randn", "f32")
    xm = torch.from_numpy(CR.masked(CR.case(shape, "randn")[0], K)).to(U.dev())
    xl = torch.tensor(lens)
    s = dict(search(shape, inst), timesteps=True)
    raw = whole(x, A, lens, s, top_n=K)

    def holds(res, raw, what):
        n = res.decoded_targets.shape[-1]
        assert res.num_hypotheses.tolist() == raw["n_hyp"].tolist(), what
        assert np.array_equal(res.decoded_targets_lengths.numpy(), raw["lens"]), what
        assert np.array_equal(res.decoded_targets.numpy(), raw["ids"][:, :, :n]) and not raw["ids"][:, :, n:].any(), what
        assert np.array_equal(res.scores.numpy(), raw["scores"][:, :, 0]) and np.array_equal(res.ctc_scores.numpy(), raw["scores"][:, :, 1])
        assert np.array_equal(res.num_words.numpy(), raw["counts"][:, :, 0]), what
        assert np.array_equal(res.timesteps.numpy(), raw["ts"][:, :, :n]), what
    dec = decoder(shape, inst)
    assert dec.prune(K) is dec
    holds(dec.decode_nbest(x, A, xl, timesteps=True), raw, "decode_nbest")
    one = dec.decode(x, A, xl)
    assert one.decoded_targets_lengths.tolist() == raw["lens"][:, 0].tolist()
    n = one.decoded_targets.shape[-1]
    assert np.array_equal(one.decoded_targets.numpy(), raw["ids"][:, 0, :n])
    st = dec.open_stream(A, B, T, timesteps=True)
    st.feed_nbest(x[:, :7], torch.tensor([min(7, k) for k in lens]))
    res = st.feed_nbest(x[:, 7:], torch.tensor([max(0, k - 7) for k in lens]))
    holds(res, raw, "stream")
    st.reset([1])                                                            # row 1 starts afresh: frames 3 .. 9, counted from 0
    again = st.feed_nbest(x[:, 3:10], torch.tensor([0, 7, 0]))
    fresh = whole(x[:, 3:10].contiguous(), A, [7, 7, 7], s, top_n=K)
    m = again.decoded_targets.shape[-1]
    assert np.array_equal(again.decoded_targets[1].numpy(), np.pad(fresh["ids"][1], ((0, 0), (0, max(0, m - 7))))[:, :m])
    assert np.array_equal(again.scores[1].numpy(), fresh["scores"][1, :, 0])
    assert np.array_equal(again.decoded_targets[0].numpy(), res.decoded_targets[0].numpy()[:, :m])   # the others: as they were
    # prune(None) and a later configure() give the unpruned results; a search that prunes nothing never reaches a *_cut entry
    plain = whole(x, A, lens, s)
    assert not np.array_equal(plain["scores"], raw["scores"])
    pruned_on_masked = decoder(shape, inst).decode_nbest(xm, A, xl, timesteps=True)
    holds(pruned_on_masked, raw, "the unpruned decoder on masked emissions")
    from end2end_amd import engines

    def refuse(*a, **k):
        raise AssertionError("a search that prunes nothing went to a *_cut entry")
    monkeypatch.setattr(engines._AsgCut, "call", staticmethod(refuse))
    monkeypatch.setattr(engines._AsgCut, "query", staticmethod(refuse))
    holds(dec.prune(None).decode_nbest(x, A, xl, timesteps=True), plain, "prune(None)")
    holds(dec.prune(V).decode_nbest(x, A, xl, timesteps=True), plain, "prune(V)")
    dec.prune(K)
    redo = decoder(shape, inst).prune(K)
    redo.configure(beam_width=W, **(dict(lm_path=MODEL_PATH, **CR.KNOBS) if inst == "lm" else dict(wip=0.0)))
    holds(redo.decode_nbest(x, A, xl, timesteps=True), plain, "configure() drops the setting")
