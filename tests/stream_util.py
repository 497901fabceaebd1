"""Helpers of the streaming beam-search tests: the raw C-ABI call e2e_ctc_beam_stream on device tensors, the whole-utterance
reference (e2e_ctc_beam_nbest_opt on the concatenated frames) and the checker that feeds a chunking and compares after
every chunk.  Equality throughout (np.array_equal): a stream does the same arithmetic in the same order."""
import ctypes as C

import numpy as np
import torch

import gpu_util as U
import oracle_lib as O

KEYS = ("ids", "lens", "n_hyp", "scores", "counts", "ts")
HEADER = 256


def _space(labels):
    labels = list(labels or [])
    return labels.index(" ") if " " in labels else -1


def reference(lp, x_len, blank, W, labels, lm=None, restrict=False, lmwt=1.0, wip=0.0, oov_penalty=-1000.0, nbest=None,
              timesteps=True):
    """e2e_ctc_beam_nbest_opt on the whole tensor with x_len -> dict of numpy arrays (outputs start as garbage)."""
    from end2end_amd import _lib
    L = _lib.load()
    d = U.dev()
    lp = lp.to(d)
    B, T, V = lp.shape
    xl = torch.as_tensor(np.asarray(x_len)).to(d, torch.long)
    N = W if nbest is None else nbest
    max_out = T + 1
    out = torch.full((B, N, max_out), -7, dtype=torch.long, device=d)
    out_len = torch.full((B, N), -7, dtype=torch.long, device=d)
    n_hyp = torch.full((B,), -7, dtype=torch.long, device=d)
    scores = torch.full((B, N, 3), 7.0, dtype=torch.float64, device=d)
    counts = torch.full((B, N, 2), -7, dtype=torch.int32, device=d)
    ts = torch.full((B, N, max_out), -7, dtype=torch.long, device=d) if timesteps else None
    ws = torch.empty(L.e2e_ctc_beam_nbest_workspace_bytes(B, T, V, W, 1 if lm is not None else 0, 1 if timesteps else 0),
                     dtype=torch.uint8, device=d)
    opts = _lib.BeamOpts(1)
    sB, sT, sV = lp.stride()
    _lib.check(L.e2e_ctc_beam_nbest_opt(lp.data_ptr(), _lib.dtype_code(lp.dtype), sB, sT, sV, xl.data_ptr(), B, T, V, blank,
                                        W, _space(labels), lm.on(d).handle if lm is not None else None, lmwt, wip, oov_penalty,
                                        N, out.data_ptr(), max_out, out_len.data_ptr(), n_hyp.data_ptr(), scores.data_ptr(),
                                        counts.data_ptr(), ts.data_ptr() if timesteps else None,
                                        ws.data_ptr(), ws.numel(), _lib.stream_ptr(d), C.byref(opts) if restrict else None))
    torch.cuda.synchronize()
    return dict(ids=out.cpu().numpy(), lens=out_len.cpu().numpy(), n_hyp=n_hyp.cpu().numpy(), scores=scores.cpu().numpy(),
                counts=counts.cpu().numpy(), ts=ts.cpu().numpy() if timesteps else None)


class RawStream:
    """B state rows and the raw call.  The state starts as garbage except for zeroed headers; every output of every call
    starts as garbage, so what a call leaves unwritten shows."""

    def __init__(self, B, max_frames, V, W, labels=None, blank=0, lm=None, restrict=False, lmwt=1.0, wip=0.0,
                 oov_penalty=-1000.0, timesteps=True, max_out=None):
        from end2end_amd import _lib
        self._lib, self.L, self.d = _lib, _lib.load(), U.dev()
        self.B, self.max_frames, self.V, self.W, self.blank = B, max_frames, V, W, blank
        self.labels, self.lm, self.restrict = labels, lm, restrict
        self.lmwt, self.wip, self.oov = lmwt, wip, oov_penalty
        self.timesteps = timesteps
        self.max_out = max_frames + 1 if max_out is None else max_out
        self.row_bytes = self.L.e2e_ctc_beam_stream_row_bytes(max_frames, V, W, 1 if lm is not None else 0, 1 if timesteps else 0)
        assert self.row_bytes > 0 and self.row_bytes % 256 == 0
        g = torch.Generator().manual_seed(12345)
        self.state = torch.randint(0, 256, (B, self.row_bytes), generator=g, dtype=torch.uint8).to(self.d)
        self.state[:, :HEADER] = 0
        n = self.L.e2e_ctc_beam_stream_workspace_bytes(B, V, W, 1 if lm is not None else 0)
        self.ws = torch.empty(n, dtype=torch.uint8, device=self.d) if n else None

    def feed(self, chunk, chunk_len, nbest=None, W=None, expect_rc=0, outputs=None):
        """One call.  chunk: (B,Tc,V) on any device, any strides.  -> dict with the read-out and frames_done."""
        _lib, L, d = self._lib, self.L, self.d
        if not chunk.is_cuda:
            base = chunk
            chunk = torch.empty_strided(base.shape, base.stride(), dtype=base.dtype, device=d)
            chunk.copy_(base)
        B, Tc, V = chunk.shape
        W = self.W if W is None else W
        N = W if nbest is None else nbest
        cl = torch.as_tensor(np.asarray(chunk_len)).to(d, torch.long)
        mo = self.max_out
        if outputs is None:
            M = max(N, 1)
            outputs = dict(out=torch.full((B, M, mo), -7, dtype=torch.long, device=d),
                           out_len=torch.full((B, M), -7, dtype=torch.long, device=d),
                           n_hyp=torch.full((B,), -7, dtype=torch.long, device=d),
                           scores=torch.full((B, M, 3), 7.0, dtype=torch.float64, device=d),
                           counts=torch.full((B, M, 2), -7, dtype=torch.int32, device=d),
                           ts=torch.full((B, M, mo), -7, dtype=torch.long, device=d) if self.timesteps else None)
        o = outputs
        done = torch.full((B,), -77, dtype=torch.long, device=d)
        opts = _lib.BeamOpts(1)
        sB, sT, sV = chunk.stride()
        rc = L.e2e_ctc_beam_stream(chunk.data_ptr(), _lib.dtype_code(chunk.dtype), sB, sT, sV, cl.data_ptr(), B, Tc, V,
                                   self.blank, W, _space(self.labels), self.lm.on(d).handle if self.lm is not None else None,
                                   self.lmwt, self.wip, self.oov, self.state.data_ptr(), self.row_bytes, self.max_frames,
                                   1 if self.timesteps else 0, N, o["out"].data_ptr(), mo, o["out_len"].data_ptr(),
                                   o["n_hyp"].data_ptr(), o["scores"].data_ptr(), o["counts"].data_ptr(),
                                   o["ts"].data_ptr() if self.timesteps else None, done.data_ptr(),
                                   self.ws.data_ptr() if self.ws is not None else None,
                                   self.ws.numel() if self.ws is not None else 0, _lib.stream_ptr(d),
                                   C.byref(opts) if self.restrict else None)
        assert rc == expect_rc, (rc, L.e2e_last_error())
        torch.cuda.synchronize()
        return dict(ids=o["out"].cpu().numpy(), lens=o["out_len"].cpu().numpy(), n_hyp=o["n_hyp"].cpu().numpy(),
                    scores=o["scores"].cpu().numpy(), counts=o["counts"].cpu().numpy(),
                    ts=o["ts"].cpu().numpy() if self.timesteps else None, done=done.cpu().numpy())


def regular(x_len, T, size):
    """Chunks of `size` frames cut from the common time axis: utterance b gets what is left of its x_len[b] frames."""
    return [[max(0, min(int(n) - a, min(size, T - a))) for n in x_len] for a in range(0, T, size)]


def same(r, ref, what=""):
    for k in KEYS:
        if ref[k] is None:
            continue
        assert np.array_equal(r[k], ref[k]), (what, k)


def check_stream(lp, x_len, chunking, blank, W, labels, lm=None, olm=None, restrict=False, cache=None, oracle=True,
                 time_major=False, **kw):
    """Feed `chunking` (a list of per-utterance chunk lengths) and, after every chunk, hold every output to the whole-utterance
    call on the frames fed so far and hypothesis 0 to the oracle's beam search.  cache: results per tuple of lengths, shared by
    the chunkings of one case.  Returns the last read-out."""
    B, T, V = lp.shape
    x_len = [T] * B if x_len is None else list(x_len)
    cache = {} if cache is None else cache
    gpu_kw = {k: v for k, v in kw.items() if k != "case_sensitive"}
    s = RawStream(B, T, V, W, labels, blank, lm, restrict, **gpu_kw)
    dlp = lp.to(U.dev())
    if time_major:
        dlp = dlp.permute(1, 0, 2).contiguous().permute(1, 0, 2)          # (B,T,V) view of a time-major tensor
    fed = [0] * B
    r = None
    for lens in chunking:
        Tc = max(max(lens), 1)
        starts = {fed[b] for b in range(B) if lens[b] > 0}
        if len(starts) <= 1 and (not starts or min(starts) + Tc <= T):
            a = min(starts) if starts else 0
            chunk = dlp[:, a:a + Tc]                                       # a view: the strides of the whole tensor
        else:
            chunk = torch.zeros((B, Tc, V), dtype=lp.dtype, device=U.dev())
            for b in range(B):
                chunk[b, :lens[b]] = dlp[b, fed[b]:fed[b] + lens[b]]
        r = s.feed(chunk, lens)
        fed = [fed[b] + lens[b] for b in range(B)]
        assert max(fed[b] - x_len[b] for b in range(B)) <= 0
        assert r["done"].tolist() == fed, (r["done"], fed)
        key = tuple(fed)
        if key not in cache:
            ref = reference(lp, fed, blank, W, labels, lm, restrict, **gpu_kw)
            orc = O.ctc_beam(lp.double().numpy(), fed, blank, W, labels, olm, **kw) if oracle and not restrict else None
            cache[key] = (ref, orc)
        ref, orc = cache[key]
        same(r, ref, key)
        if orc is not None:
            o_ids, o_lens, _ = orc
            assert r["lens"][:, 0].tolist() == o_lens.tolist(), key
            assert r["ids"][:, 0, :o_ids.shape[1]].tolist() == o_ids.tolist(), key
    return r
