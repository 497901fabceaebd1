"""Helpers of the streaming Gram-CTC beam-search tests (TEST INFRASTRUCTURE ONLY): the raw C-ABI call
e2e_gram_ctc_beam_stream on device tensors, the whole-utterance reference (e2e_gram_ctc_beam_nbest for scored = 0,
e2e_gram_ctc_beam_nbest_opt for scored = 1, on the concatenated frames) and the checker that feeds a chunking and compares
after every chunk.  Equality throughout (np.array_equal): a stream does the same arithmetic in the same order.  Modelled on
tests/asg_stream_util.py."""
import ctypes as C

import numpy as np
import torch

import gpu_util as U

KEYS = ("ids", "lens", "n_hyp", "scores", "counts", "ts")
HEADER = 256
# the header's fields (include/e2e_ctc.h): byte offsets of the 4-byte ones, esum's 8 bytes at 56
H_N, H_FRAMES, H_OVERFLOW, H_DEAD, H_ESUM = 36, 40, 44, 48, 56


class Search:
    """One configuration of the search: the table, the width, and -- scored -- the model, the knobs and the restriction."""

    def __init__(self, R, V, l2i, W, scored=False, labels=None, lm=None, restrict=False, lmwt=0.0, wip=0.0, oov_penalty=0.0):
        from end2end_amd.engines import GramCTCDecoderEngine
        self.eng = GramCTCDecoderEngine(0, R, V, l2i, W, labels)
        self.R, self.V, self.W, self.K = R, V, W, self.eng.max_order
        self.scored, self.lm, self.restrict = scored, lm, restrict
        self.space = list(labels).index(" ") if labels and " " in labels else -1
        self.lmwt, self.wip, self.oov = lmwt, wip, oov_penalty
        assert scored or (lm is None and not restrict)

    def table(self, d):
        return self.eng._table(d)


def garbage(B, N, max_out, d, scored, timesteps):
    """The outputs of one call, pre-filled so that what the call leaves unwritten shows."""
    return dict(out=torch.full((B, N, max_out), -7, dtype=torch.long, device=d),
                out_len=torch.full((B, N), -7, dtype=torch.long, device=d),
                n_hyp=torch.full((B,), -7, dtype=torch.long, device=d),
                scores=torch.full((B, N, 3) if scored else (B, N), 7.0, dtype=torch.float64, device=d),
                counts=torch.full((B, N, 2), -7, dtype=torch.int32, device=d) if scored else None,
                ts=torch.full((B, N, max_out), -7, dtype=torch.long, device=d) if scored and timesteps else None)


def host(o):
    opt = lambda t: t.cpu().numpy() if t is not None else None   # noqa: E731
    return dict(ids=o["out"].cpu().numpy(), lens=o["out_len"].cpu().numpy(), n_hyp=o["n_hyp"].cpu().numpy(),
                scores=o["scores"].cpu().numpy(), counts=opt(o["counts"]), ts=opt(o["ts"]))


def reference(x, x_len, s, nbest=None, max_out=None, timesteps=True):
    """The whole call on the whole tensor with x_len -> dict of numpy arrays (outputs start as garbage)."""
    from end2end_amd import _lib
    L = _lib.load()
    d = U.dev()
    x = x.to(d)
    B, T, V = x.shape
    xl = torch.as_tensor(np.asarray(x_len)).to(d, torch.long)
    N = s.W if nbest is None else nbest
    max_out = T * s.K if max_out is None else max_out
    o = garbage(B, N, max_out, d, s.scored, timesteps)
    ids, lens = s.table(d)
    sB, sT, sV = x.stride()
    head = (x.data_ptr(), _lib.dtype_code(x.dtype), sB, sT, sV, xl.data_ptr(), B, T, V, ids.data_ptr(), lens.data_ptr(), s.K)
    tail = (N, o["out"].data_ptr(), max_out, o["out_len"].data_ptr(), o["n_hyp"].data_ptr(), o["scores"].data_ptr())
    if s.scored:
        ws = torch.empty(L.e2e_gram_beam_workspace_bytes_lm(B, T, V, s.K, s.W, 1 if s.lm is not None else 0), dtype=torch.uint8, device=d)
        opts = _lib.GramBeamOpts(1 if s.restrict else 0, o["ts"].data_ptr() if o["ts"] is not None else None)
        _lib.check(L.e2e_gram_ctc_beam_nbest_opt(*head, s.R, s.W, s.space, s.lm.on(d).handle if s.lm is not None else None,
                                                 s.lmwt, s.wip, s.oov, *tail, o["counts"].data_ptr(), ws.data_ptr(), ws.numel(),
                                                 _lib.stream_ptr(d), C.byref(opts)))
    else:
        ws = torch.empty(L.e2e_gram_beam_workspace_bytes(B, T, V, s.K, s.W), dtype=torch.uint8, device=d)
        _lib.check(L.e2e_gram_ctc_beam_nbest(*head, s.W, *tail, ws.data_ptr(), ws.numel(), _lib.stream_ptr(d)))
    torch.cuda.synchronize()
    return host(o)


class RawStream:
    """B state rows and the raw call.  The state starts as garbage except for zeroed headers; every output of every call
    starts as garbage, so what a call leaves unwritten shows."""

    def __init__(self, B, max_frames, s, timesteps=True, max_out=None):
        from end2end_amd import _lib
        self._lib, self.L, self.d = _lib, _lib.load(), U.dev()
        self.B, self.max_frames, self.s = B, max_frames, s
        self.timesteps = timesteps
        self.max_out = max_frames * s.K if max_out is None else max_out
        self.row_bytes = self.L.e2e_gram_beam_stream_row_bytes(max_frames, s.V, s.K, s.W, 1 if s.scored else 0,
                                                               1 if s.lm is not None else 0)
        assert self.row_bytes > 0 and self.row_bytes % 256 == 0
        g = torch.Generator().manual_seed(12345)
        self.state = torch.randint(0, 256, (B, self.row_bytes), generator=g, dtype=torch.uint8).to(self.d)
        self.state[:, :HEADER] = 0

    def field(self, b, offset, size=4):
        """A header field of row b, little endian."""
        return int.from_bytes(bytes(self.state[b, offset:offset + size].cpu().tolist()), "little", signed=True)

    def feed(self, chunk, chunk_len, nbest=None, expect_rc=0, outputs=None, s=None, max_frames=None):
        """One call.  chunk: (B,Tc,V) on any device, any strides.  s, max_frames: of this call alone (a call under another
        configuration).  -> dict with the read-out (the garbage where nothing was written) and frames_done."""
        _lib, L, d = self._lib, self.L, self.d
        s = self.s if s is None else s
        max_frames = self.max_frames if max_frames is None else max_frames
        if not chunk.is_cuda:
            base = chunk
            chunk = torch.empty_strided(base.shape, base.stride(), dtype=base.dtype, device=d)
            chunk.copy_(base)
        B, Tc, V = chunk.shape
        N = s.W if nbest is None else nbest
        cl = torch.as_tensor(np.asarray(chunk_len)).to(d, torch.long)
        mo = self.max_out
        o = garbage(B, max(N, 1), mo, d, s.scored, self.timesteps) if outputs is None else outputs
        done = torch.full((B,), -77, dtype=torch.long, device=d)
        # (the workspace carries nothing from call to call: it starts as garbage every time, the answer cache with it)
        ws = torch.full((L.e2e_gram_beam_stream_workspace_bytes(B, V, s.K, s.W, 1 if s.scored else 0, 1 if s.lm is not None else 0),),
                        0xAB, dtype=torch.uint8, device=d)
        opts = _lib.GramBeamOpts(1 if s.restrict else 0, o["ts"].data_ptr() if o["ts"] is not None else None) if s.scored else None
        ids, lens = s.table(d)
        sB, sT, sV = chunk.stride()
        rc = L.e2e_gram_ctc_beam_stream(chunk.data_ptr(), _lib.dtype_code(chunk.dtype), sB, sT, sV, cl.data_ptr(), B, Tc, V,
                                        ids.data_ptr(), lens.data_ptr(), s.K, s.R, s.W, 1 if s.scored else 0, s.space,
                                        s.lm.on(d).handle if s.lm is not None else None, s.lmwt, s.wip, s.oov,
                                        self.state.data_ptr(), self.row_bytes, max_frames, N, o["out"].data_ptr(), mo,
                                        o["out_len"].data_ptr(), o["n_hyp"].data_ptr(), o["scores"].data_ptr(),
                                        o["counts"].data_ptr() if o["counts"] is not None else None,
                                        done.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr(d),
                                        C.byref(opts) if opts is not None else None)
        assert rc == expect_rc, (rc, L.e2e_last_error())
        torch.cuda.synchronize()
        r = host(o)
        r["done"] = done.cpu().numpy()
        return r


def regular(x_len, T, size):
    """Chunks of `size` frames cut from the common time axis: utterance b gets what is left of its x_len[b] frames."""
    return [[max(0, min(int(n) - a, min(size, T - a))) for n in x_len] for a in range(0, T, size)]


def cuts(x_len, sizes):
    """Chunks of the given sizes cut from the common time axis."""
    out, a = [], 0
    for s in sizes:
        out.append([max(0, min(int(n) - a, s)) for n in x_len])
        a += s
    return out


def same(r, ref, what=""):
    for k in KEYS:
        if ref[k] is None:
            continue
        assert np.array_equal(r[k], ref[k]), (what, k)


def view_of(x, layout):
    """x (B,T,V) on the GPU as it is, as a (B,T,V) view of a time-major tensor, or as a view with gaps."""
    if layout == "time_major":
        return x.permute(1, 0, 2).contiguous().permute(1, 0, 2)
    if layout == "strided":
        B, T, V = x.shape
        buf = torch.full((B, T + 3, 2 * V + 1), 7.0, dtype=x.dtype, device=x.device)
        v = buf[:, 2:2 + T, 1:1 + 2 * V:2]
        v.copy_(x)
        return v
    return x


def check_stream(x, x_len, chunking, s, cache=None, layout=None, check_after=None, nbest=None, **kw):
    """Feed `chunking` (a list of per-utterance chunk lengths) and, after every chunk (check_after: after these chunks only),
    hold every output to the whole call on the frames fed so far -- before the first chunk too: a fresh row read out at
    f_b = 0.  cache: results per tuple of lengths, shared by the chunkings of one case.  Chunks are views of the whole tensor
    where the utterances' frames line up.  Returns the last read-out."""
    B, T, V = x.shape
    x_len = [T] * B if x_len is None else list(x_len)
    cache = {} if cache is None else cache
    st = RawStream(B, T, s, **kw)
    dx = view_of(x.to(U.dev()), layout)
    fed = [0] * B
    r = None
    for i, lens in enumerate(chunking):
        Tc = max(max(lens), 1)
        starts = {fed[b] for b in range(B) if lens[b] > 0}
        if len(starts) <= 1 and (not starts or min(starts) + Tc <= T):
            a = min(starts) if starts else 0
            chunk = dx[:, a:a + Tc]                                        # a view: the strides of the whole tensor
        else:
            chunk = torch.zeros((B, Tc, V), dtype=x.dtype, device=U.dev())
            for b in range(B):
                chunk[b, :lens[b]] = dx[b, fed[b]:fed[b] + lens[b]]
        r = st.feed(chunk, lens, nbest=nbest)
        fed = [fed[b] + lens[b] for b in range(B)]
        assert max(fed[b] - x_len[b] for b in range(B)) <= 0
        assert r["done"].tolist() == fed, (r["done"], fed)
        if check_after is not None and i not in check_after:
            continue
        key = tuple(fed)
        if key not in cache:
            cache[key] = reference(x, fed, s, nbest=nbest, **kw)
        same(r, cache[key], key)
    return r
