"""Helpers of the streaming ASG beam-search tests (TEST INFRASTRUCTURE ONLY): the raw C-ABI call e2e_asg_beam_stream on device
tensors, the whole-utterance reference (e2e_asg_beam_nbest_opt on the concatenated frames) and the checker that feeds a
chunking and compares after every chunk.  Equality throughout (np.array_equal): a stream does the same arithmetic in the same
order.  Modelled on tests/stream_util.py."""
import ctypes as C

import numpy as np
import torch

import gpu_util as U

KEYS = ("ids", "lens", "n_hyp", "scores", "counts", "ts")
HEADER = 256


def space_of(chars):
    chars = list(chars or [])
    return chars.index(" ") if " " in chars else -1


def garbage(B, N, max_out, d, timesteps=True):
    """The outputs of one call, pre-filled so that what the call leaves unwritten shows."""
    return dict(out=torch.full((B, N, max_out), -7, dtype=torch.long, device=d),
                out_len=torch.full((B, N), -7, dtype=torch.long, device=d),
                n_hyp=torch.full((B,), -7, dtype=torch.long, device=d),
                scores=torch.full((B, N, 3), 7.0, dtype=torch.float64, device=d),
                counts=torch.full((B, N, 2), -7, dtype=torch.int32, device=d),
                ts=torch.full((B, N, max_out), -7, dtype=torch.long, device=d) if timesteps else None)


def host(o):
    return dict(ids=o["out"].cpu().numpy(), lens=o["out_len"].cpu().numpy(), n_hyp=o["n_hyp"].cpu().numpy(),
                scores=o["scores"].cpu().numpy(), counts=o["counts"].cpu().numpy(),
                ts=o["ts"].cpu().numpy() if o["ts"] is not None else None)


def transitions(A, dtype, d):
    return None if A is None else A.to(device=d, dtype=dtype).contiguous()


def reference(x, A, x_len, R, W, space, lm=None, restrict=False, lmwt=0.0, wip=0.0, oov_penalty=0.0, nbest=None,
              max_out=None, timesteps=True):
    """e2e_asg_beam_nbest_opt on the whole tensor with x_len -> dict of numpy arrays (outputs start as garbage)."""
    from end2end_amd import _lib
    L = _lib.load()
    d = U.dev()
    x = x.to(d)
    B, T, V = x.shape
    xl = torch.as_tensor(np.asarray(x_len)).to(d, torch.long)
    N = W if nbest is None else nbest
    max_out = T if max_out is None else max_out
    o = garbage(B, N, max_out, d, timesteps)
    At = transitions(A, x.dtype, d)
    ws = torch.empty(L.e2e_asg_beam_workspace_bytes(B, T, V, W, 1 if lm is not None else 0), dtype=torch.uint8, device=d)
    opts = _lib.AsgBeamOpts(1 if restrict else 0, o["ts"].data_ptr() if timesteps else None)
    sB, sT, sV = x.stride()
    _lib.check(L.e2e_asg_beam_nbest_opt(x.data_ptr(), _lib.dtype_code(x.dtype), sB, sT, sV, At.data_ptr() if At is not None else None,
                                        xl.data_ptr(), B, T, V, R, W, space, lm.on(d).handle if lm is not None else None,
                                        lmwt, wip, oov_penalty, N, o["out"].data_ptr(), max_out, o["out_len"].data_ptr(),
                                        o["n_hyp"].data_ptr(), o["scores"].data_ptr(), o["counts"].data_ptr(),
                                        ws.data_ptr(), ws.numel(), _lib.stream_ptr(d), C.byref(opts)))
    torch.cuda.synchronize()
    return host(o)


class RawStream:
    """B state rows and the raw call.  The state starts as garbage except for zeroed headers; every output of every call
    starts as garbage, so what a call leaves unwritten shows."""

    def __init__(self, B, max_frames, V, R, W, space, A=None, lm=None, restrict=False, lmwt=0.0, wip=0.0, oov_penalty=0.0,
                 timesteps=True, max_out=None):
        from end2end_amd import _lib
        self._lib, self.L, self.d = _lib, _lib.load(), U.dev()
        self.B, self.max_frames, self.V, self.R, self.W, self.space = B, max_frames, V, R, W, space
        self.A, self.lm, self.restrict = A, lm, restrict
        self.lmwt, self.wip, self.oov = lmwt, wip, oov_penalty
        self.timesteps = timesteps
        self.max_out = max_frames if max_out is None else max_out
        self.row_bytes = self.L.e2e_asg_beam_stream_row_bytes(max_frames, V, W, 1 if lm is not None else 0)
        assert self.row_bytes > 0 and self.row_bytes % 256 == 0
        g = torch.Generator().manual_seed(12345)
        self.state = torch.randint(0, 256, (B, self.row_bytes), generator=g, dtype=torch.uint8).to(self.d)
        self.state[:, :HEADER] = 0

    def feed(self, chunk, chunk_len, nbest=None, expect_rc=0, outputs=None, **other):
        """One call.  chunk: (B,Tc,V) on any device, any strides.  other: W, R, A, lm, max_frames of this call alone (a call
        under another configuration).  -> dict with the read-out (the garbage where nothing was written) and frames_done."""
        _lib, L, d = self._lib, self.L, self.d
        if not chunk.is_cuda:
            base = chunk
            chunk = torch.empty_strided(base.shape, base.stride(), dtype=base.dtype, device=d)
            chunk.copy_(base)
        B, Tc, V = chunk.shape
        W, R = other.get("W", self.W), other.get("R", self.R)
        lm, A = other.get("lm", self.lm), other.get("A", self.A)
        max_frames = other.get("max_frames", self.max_frames)
        N = W if nbest is None else nbest
        cl = torch.as_tensor(np.asarray(chunk_len)).to(d, torch.long)
        mo = self.max_out
        o = garbage(B, max(N, 1), mo, d, self.timesteps) if outputs is None else outputs
        done = torch.full((B,), -77, dtype=torch.long, device=d)
        At = transitions(A, chunk.dtype, d)
        ws = torch.empty(L.e2e_asg_beam_stream_workspace_bytes(B, V, W, 1 if lm is not None else 0), dtype=torch.uint8, device=d)
        opts = _lib.AsgBeamOpts(1 if self.restrict else 0, o["ts"].data_ptr() if self.timesteps else None)
        sB, sT, sV = chunk.stride()
        rc = L.e2e_asg_beam_stream(chunk.data_ptr(), _lib.dtype_code(chunk.dtype), sB, sT, sV,
                                   At.data_ptr() if At is not None else None, cl.data_ptr(), B, Tc, V, R, W, self.space,
                                   lm.on(d).handle if lm is not None else None, self.lmwt, self.wip, self.oov,
                                   self.state.data_ptr(), self.row_bytes, max_frames, N, o["out"].data_ptr(), mo,
                                   o["out_len"].data_ptr(), o["n_hyp"].data_ptr(), o["scores"].data_ptr(), o["counts"].data_ptr(),
                                   done.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr(d), C.byref(opts))
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


def check_stream(x, A, x_len, chunking, R, W, space, lm=None, restrict=False, cache=None, layout=None, check_after=None,
                 nbest=None, **kw):
    """Feed `chunking` (a list of per-utterance chunk lengths) and, after every chunk (check_after: after these chunks only),
    hold every output to the whole-utterance call on the frames fed so far.  cache: results per tuple of lengths, shared by the
    chunkings of one case.  Chunks are views of the whole tensor where the utterances' frames line up.  Returns the last
    read-out."""
    B, T, V = x.shape
    x_len = [T] * B if x_len is None else list(x_len)
    cache = {} if cache is None else cache
    s = RawStream(B, T, V, R, W, space, A, lm, restrict, **kw)
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
        r = s.feed(chunk, lens, nbest=nbest)
        fed = [fed[b] + lens[b] for b in range(B)]
        assert max(fed[b] - x_len[b] for b in range(B)) <= 0
        assert r["done"].tolist() == fed, (r["done"], fed)
        if check_after is not None and i not in check_after:
            continue
        key = tuple(fed)
        if key not in cache:
            cache[key] = reference(x, A, fed, R, W, space, lm, restrict, nbest=nbest, **kw)
        same(r, cache[key], key)
    return r
