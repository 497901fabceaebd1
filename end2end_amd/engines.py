"""The two engines of the reference's pybind modules, computed on the MI355X.

CTCLossEngine    <-> cpp_ctc_loss.CTCLossEngine     (src/losses/ctc_loss_py.cpp:8-16)
CTCDecoderEngine <-> cpp_ctc_decoder.CTCDecoder     (src/decoders/ctc_decoder_py.cpp:8-38)

and, with the same compute() contract, CTCWithoutBlankLossEngine for the blank-free loss (a numba function upstream,
pytorch_end2end/functions/ctc_without_blank.py) and GramCTCLossEngine <-> cpp_gram_ctc_loss.GramCTCLossEngine
(src/losses/gram_ctc_loss_py.cpp; its compute_2d is empty upstream).

Same constructor arguments, keyword names, defaults and results.  The top-level modules `cpp_ctc_loss` and
`cpp_ctc_decoder` of this repository export them under the reference's names, so that the reference's own callers
(`import_module("cpp_ctc_loss")`, pytorch_end2end/modules/ctc_loss.py:74; `import cpp_ctc_decoder`,
pytorch_end2end/decoders/ctc_decoder.py:13) find them.

Unlike the reference (which copies GPU tensors to the host and computes in C++ threads,
src/losses/forward_backward.cpp:12-19) tensors stay on the GPU: the engines hand device addresses, strides and sizes
to the C ABI (include/e2e_ctc.h) through the pybind11 layer `end2end_amd._C`.  CPU tensors are moved to the current GPU
and the loss results moved back to the source device and dtype (forward_backward.cpp:55-56); decode results are CPU
tensors as upstream (ctc_decoder.cpp:157,449) unless `keep_on_device` is set.
"""
import os
import threading
import warnings

import numpy as np
import torch

from . import _runtime as R
from ._runtime import _C


def _as_long(t, device):
    if not torch.is_tensor(t):
        t = torch.as_tensor(t)
    elif t.dtype == torch.long and t.device == device and t.is_contiguous():
        return t                         # (the usual case on a training step: nothing to convert, no dispatcher round trips)
    return t.to(device=device, dtype=torch.long).contiguous()


_F32_F64 = (torch.float32, torch.float64)
_16BIT = (torch.float16, torch.bfloat16)
_REDUCTIONS = {None: _C.REDUCE_NONE, "sum": _C.REDUCE_SUM, "mean": _C.REDUCE_MEAN}
_ws_bytes = {}                           # (B, T, V, Smax, dtype code, algo) -> e2e_ctc_loss_workspace_bytes


class _GramCut:
    """The pruned Gram-CTC entries (e2e_gram_beam_cut_*, e2e_gram_ctc_beam_*_cut; include/e2e_ctc.h), reached through the
    ctypes view: end2end_amd._C's set of functions is held to a recording by tests/test_bindings_cpu.py, and _lib types every
    symbol of _C.SIGNATURES -- these included -- from the header.  A query returns its value; a call takes addresses as
    integers (0: NULL), `opts` as None or (restrict_to_lexicon, timesteps), and raises E2EError as _C's wrappers do."""

    @staticmethod
    def query(name, *args):
        from . import _lib
        return getattr(_lib.load(), "e2e_gram_beam_cut_" + name)(*args)

    @staticmethod
    def call(name, *args):
        """args: the C parameters in order, `opts` in its place; cutoff_top_n and cutoff_prob last."""
        import ctypes
        from . import _lib
        L = _lib.load()
        at = len(args) - 3
        opts = None if args[at] is None else _lib.GramBeamOpts(1 if args[at][0] else 0, args[at][1] or None)
        rc = getattr(L, name)(*args[:at], None if opts is None else ctypes.byref(opts), *args[at + 1:])
        if rc:
            raise R.E2EError("libe2e_ctc: %s (code %d)" % (L.e2e_last_error().decode(errors="replace"), rc))


class _AsgCut:
    """The pruned ASG entries (e2e_asg_beam_cut_*, e2e_asg_beam_*_cut; include/e2e_ctc.h), reached through the ctypes view as
    _GramCut's are, and for the same reason.  A call takes addresses as integers (0: NULL), `opts` as (restrict_to_lexicon,
    timesteps), cutoff_top_n last."""

    @staticmethod
    def query(name, *args):
        from . import _lib
        return getattr(_lib.load(), "e2e_asg_beam_cut_" + name)(*args)

    @staticmethod
    def call(name, *args):
        import ctypes
        from . import _lib
        L = _lib.load()
        at = len(args) - 2
        opts = _lib.AsgBeamOpts(1 if args[at][0] else 0, args[at][1] or None)
        rc = getattr(L, name)(*args[:at], ctypes.byref(opts), args[at + 1])
        if rc:
            raise R.E2EError("libe2e_ctc: %s (code %d)" % (L.e2e_last_error().decode(errors="replace"), rc))


def _on_device(dev):
    """A context that makes `dev` the current GPU -- none at all when it already is (the context manager costs ~10 us of host time
    per entry, which on a 130 us step is what decides whether the host stays ahead of the GPU)."""
    if torch.cuda.current_device() == dev.index:
        return _NULL_CTX
    return torch.cuda.device(dev)


def _pack_nbest(out, lens, nh, strings, keep_on_device):
    """The tail of an n-best read-out: out (B,N,max_out) on the device, lens [B][N] and nh [B] on the host, strings(rows, lens)
    the engine's spelling -> (ids (B,N,width) packed to the longest hypothesis of the batch, on the device or the host as
    keep_on_device says; sentences [B][nh[b]]; width)."""
    B, N = out.shape[:2]
    width = max((max(row) for row in lens), default=0)
    ids = out[:, :, :width].contiguous()
    ids_host = ids.cpu()
    flat = strings(ids_host.reshape(B * N, width), [n for row in lens for n in row])   # one lookup per batch
    sentences = [flat[b * N: b * N + nh[b]] for b in range(B)]
    return ids if keep_on_device else ids_host, sentences, width


def _nbest_buffers(B, N, max_out, dev, scored=True, timesteps=False, prefill=None):
    """The buffers an n-best read-out fills -> (out (B,N,max_out) int64, out_len (B,N), n_hyp (B), scores (B,N,3) f64, counts
    (B,N,2) int32, ts (B,N,max_out) int64 or None); not scored (Gram-CTC's search on the masses): scores (B,N) and no counts.
    `prefill` None: nothing (the call writes every slot); "ts": the timesteps with -1; "all": every buffer with the empty
    result -- length 0, -inf, an LM score of 0, timesteps -1 -- for a call that leaves some utterances untouched."""
    new = torch.zeros if prefill == "all" else torch.empty
    out = new((B, N, max_out), dtype=torch.long, device=dev)
    out_len = new((B, N), dtype=torch.long, device=dev)
    n_hyp = new(B, dtype=torch.long, device=dev)
    if prefill == "all":
        scores = torch.full((B, N, 3) if scored else (B, N), float("-inf"), dtype=torch.float64, device=dev)
        if scored:
            scores[:, :, 2] = 0.0
    else:
        scores = torch.empty((B, N, 3) if scored else (B, N), dtype=torch.float64, device=dev)
    counts = new((B, N, 2), dtype=torch.int32, device=dev) if scored else None
    ts = None
    if timesteps:
        ts = (torch.full((B, N, max_out), -1, dtype=torch.long, device=dev) if prefill
              else torch.empty((B, N, max_out), dtype=torch.long, device=dev))
    return out, out_len, n_hyp, scores, counts, ts


def _nbest_result(engine, out, out_len, n_hyp, scores, counts, ts):
    """What decode_nbest and a stream's feed_nbest return, from the buffers the read-out has filled: (ids, lengths, sentences,
    scores, acoustic scores, lm_scores, num_words, num_oov, num_hypotheses, timesteps or None) -- without counts (not scored):
    (ids, lengths, sentences, scores, num_hypotheses).  The status that rides on the counts and lengths is the engine's to
    read (`_check_nbest`), its spelling `_strings`."""
    nh, lens = n_hyp.tolist(), out_len.tolist()
    engine._check_nbest(nh, lens, out.shape[2])
    ids, sentences, width = _pack_nbest(out, lens, nh, engine._strings, engine.keep_on_device)
    r = (lambda t: t) if engine.keep_on_device else (lambda t: t.cpu())
    if counts is None:
        return (ids, r(out_len), sentences, r(scores), r(n_hyp))
    if ts is not None:
        ts = r(ts[:, :, :width].contiguous())
    return (ids, r(out_len), sentences, r(scores[:, :, 0].contiguous()),
            r(scores[:, :, 1].contiguous()), r(scores[:, :, 2].contiguous()), r(counts[:, :, 0].contiguous()),
            r(counts[:, :, 1].contiguous()), r(n_hyp), ts)


def _first_hypothesis(r):
    """Hypothesis 0 of an n-best result -> (ids (B,maxlen) int64, lengths (B), sentences), what decode / feed return."""
    return r[0][:, 0, :].contiguous(), r[1][:, 0].contiguous(), [s[0] if s else "" for s in r[2]]


def _lexicon_words(lexicon):
    """The words of a lexicon given as an iterable of words or as the path of a text file of them (white space between the
    words) -> a list; a ValueError for a file that is not there and for no words at all."""
    if isinstance(lexicon, (str, bytes, os.PathLike)):
        path = os.fsdecode(lexicon)
        if not os.path.isfile(path):
            raise ValueError("Can't find a lexicon: {}".format(path))
        with open(path, encoding="utf-8") as f:
            words = f.read().split()
    else:
        words = [str(w) for w in lexicon]
    if not words:
        raise ValueError("the lexicon is empty")
    return words


class _NullCtx:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


_NULL_CTX = _NullCtx()


class _BeamStream:
    """The beams of `batch_size` utterances, kept on the GPU between chunks: what the engines' open_stream return.  Owns the
    (batch_size, row_bytes) uint8 state tensor `state`: one self-contained row per utterance, allocated at the first chunk
    (on `device`, else on the chunk's GPU, else on the current one).  Rows may be reordered or copied by the caller; a row
    whose first 256 bytes are zero starts a new utterance.  A family says how large a row is (`_row_bytes`), how a chunk is
    checked and converted (`_prepare`), how many ids a hypothesis of so many frames can have (`_max_out`), makes its one C
    call (`_launch`) and names the statuses that are its own (`_STATUS`)."""

    HEADER_BYTES = 256
    _INPUT = "logits"                    # what check_chunk calls a chunk
    _PREFILL = None                      # _nbest_buffers' prefill
    _STATUS = {}                         # frames_done < 0, beside -2 and -3: what it says of the utterance
    _scored = True

    def __init__(self, engine, batch_size, max_frames, device=None, timesteps=False):
        if int(batch_size) < 1 or int(max_frames) < 1:
            raise ValueError("batch_size and max_frames must be at least 1")
        self.engine = engine
        self.batch_size, self.max_frames = int(batch_size), int(max_frames)
        self.timesteps = bool(timesteps)
        self.device = None if device is None else torch.device(device)
        self.state = None
        self.row_bytes = 0
        self._frames = [0] * self.batch_size

    @property
    def frames(self):
        """Frames consumed so far, per utterance."""
        return list(self._frames)

    def check_chunk(self, shape):
        """The chunk's shape (batch, frames, alphabet) against the stream: a ValueError before any device work."""
        if len(shape) != 3:
            raise ValueError("%s must be (batch, time, alphabet)" % self._INPUT)
        if shape[0] != self.batch_size:
            raise ValueError("the chunk has %d utterances, the stream was opened for %d" % (shape[0], self.batch_size))
        if not 1 <= shape[1] <= self.max_frames:
            raise ValueError("a chunk of %d frames: the stream takes 1 .. max_frames = %d" % (shape[1], self.max_frames))

    def reset(self, rows=None):
        """Start the given utterances (all: None) anew: their headers are zeroed, nothing else is touched."""
        idx = range(self.batch_size) if rows is None else [int(r) for r in (rows.tolist() if torch.is_tensor(rows) else rows)]
        for b in idx:
            if not 0 <= b < self.batch_size:
                raise ValueError("row %d outside the stream's %d utterances" % (b, self.batch_size))
        if self.state is not None:
            if rows is None:
                self.state[:, : self.HEADER_BYTES].zero_()
            else:
                self.state[torch.as_tensor(list(idx), dtype=torch.long, device=self.state.device), : self.HEADER_BYTES] = 0
        for b in idx:
            self._frames[b] = 0

    def _state_for(self, V, dev):
        if self.state is None:
            self.row_bytes = self._row_bytes(V)
            if not self.row_bytes:
                raise ValueError("a stream of max_frames=%d at beam_width=%d is not supported"
                                 % (self.max_frames, self.engine.beam_width))
            self.state = torch.empty((self.batch_size, self.row_bytes), dtype=torch.uint8, device=dev)
            self.state[:, : self.HEADER_BYTES].zero_()
            self.device = dev
        return self.state

    def feed_nbest(self, logits_, logits_lengths_=None, nbest=None):
        """Feed a chunk (batch, frames, alphabet) -- of LOG-PROBABILITIES; an ASG stream: of emissions -- and read the beams out:
        what the engine's decode_nbest returns for everything fed so far (timesteps if the stream was opened with them).
        logits_lengths_: the frames of this chunk per utterance, 0 allowed, all of them by default.  nbest=0 feeds only and
        returns None."""
        return self._feed_nbest(logits_, logits_lengths_, nbest, self.timesteps)

    def _feed_nbest(self, chunk, lengths, nbest, timesteps):
        e = self.engine
        N = e.beam_width if nbest is None else int(nbest)
        if not 0 <= N <= e.beam_width:
            raise ValueError("nbest=%d outside [0, beam_width=%d]" % (N, e.beam_width))
        self.check_chunk(tuple(chunk.shape))
        B, Tc = chunk.shape[0], chunk.shape[1]
        if lengths is None:
            lengths = torch.full((B,), Tc, dtype=torch.long)
        if self.device is not None and chunk.device != self.device:
            chunk = chunk.to(self.device)
        x, xl, dev = self._prepare(chunk, lengths)
        state = self._state_for(x.shape[2], dev)
        if dev != state.device:
            raise ValueError("the chunk is on %s, the stream's state on %s" % (dev, state.device))
        max_out = self._max_out(max(self._frames) + Tc)
        frames_done = torch.empty(B, dtype=torch.long, device=dev)
        # (a buffer the read-out does not fill -- none at all with nbest=0 -- goes to the call as a null pointer)
        bufs = _nbest_buffers(B, N, max_out, dev, self._scored, timesteps, self._PREFILL) if N else (None,) * 6
        stream = R.stream_handle(dev)
        with _on_device(dev):
            self._launch(x, xl, state, N, max_out, [t.data_ptr() if t is not None else 0 for t in bufs],
                         frames_done.data_ptr(), stream)
        # what only the device knows rides on frames_done (include/e2e_ctc.h); the other utterances have advanced
        bad = None
        for b, f in enumerate(frames_done.tolist()):
            if f >= 0:
                self._frames[b] = f
            elif bad is None:
                bad = (b, f)
        if bad is not None:
            why = {-2: "would pass max_frames=%d with this chunk" % self.max_frames,
                   -3: "has a state row that was written under another configuration", **self._STATUS}
            raise R.E2EError("beam search stream: utterance %d %s" % (bad[0], why.get(bad[1], "status %d" % bad[1])))
        return _nbest_result(e, *bufs) if N else None

    def feed(self, logits_, logits_lengths_=None):
        """Feed a chunk and return what the engine's decode returns for everything fed so far: (ids, lengths, sentences)."""
        return _first_hypothesis(self.feed_nbest(logits_, logits_lengths_, nbest=1))


class _ForwardBackwardEngine:
    """compute() of the loss engines: one (B,T,V) tensor of logits or log-probabilities, padded targets and the two
    lengths in; (losses[B], grads[B,T,V]) out, on the device and in the dtype the logits came in.  A subclass says
    whether its kernels read 16-bit logits (`_takes_16bit`), what else it checks (`_check`), how large a workspace it needs
    (`_workspace_bytes`) and makes its one C call (`_launch`)."""

    _redo_flags = None                   # name of the e2e_debug_*_redo_flags entry point, if the kernels keep such flags
    _last = None                         # then: (workspace, B, T, Smax) of the last launch

    def _check(self, V):
        pass

    def _takes_16bit(self, x, targets):
        """Do the kernels read these f16 / bf16 logits as they are?  If not they are up-cast to f32, as every dtype but f32
        and f64 is."""
        return False

    def compute(self, logits, targets, logits_lengths, targets_lengths, input_is_logprobs=True,
                grad_scale=1.0, reduction=None):
        """`logits` is batch-major (B,T,V) (any strides).  With input_is_logprobs=True this is the
        reference engine: log-probabilities in, grads = exp(lp) - posterior.  With False the
        log-softmax is fused in and grads are d loss / d logits.

        Extensions (e2e_ctc_loss_opts): `grad_scale` multiplies every gradient element as the kernel writes it;
        `reduction` = "sum" / "mean" makes the call also return the reduced loss, written by the tail of its last
        kernel: the result is then (losses, grads, reduced)."""
        if logits.dim() != 3:
            raise ValueError("logits must be (batch, time, alphabet)")
        self._check(logits.shape[2])
        src_device, src_dtype = logits.device, logits.dtype
        dev = R.compute_device(logits)
        targets = _as_long(targets, dev)
        x = logits.detach().to(dev)
        if x.dtype not in _F32_F64 and not (x.dtype in _16BIT and self._takes_16bit(x, targets)):
            x = x.to(torch.float32)
        B, T, V = x.shape
        if targets.dim() != 2 or targets.shape[0] != B:
            raise ValueError("targets must be (batch, max_target_length)")
        xl = _as_long(logits_lengths, dev)
        tl = _as_long(targets_lengths, dev)
        if xl.numel() != B or tl.numel() != B:
            raise ValueError("lengths must have one entry per utterance")
        if reduction not in (None, "sum", "mean"):
            raise ValueError("reduction must be None, 'sum' or 'mean'")
        Smax = targets.shape[1]
        if Smax == 0:
            targets = torch.zeros((B, 1), dtype=torch.long, device=dev)    # (an address to hand over; never read)
        loss_dtype = torch.float32 if x.dtype in _16BIT else x.dtype       # (16-bit I/O: the library keeps losses in f32)
        losses = torch.empty(B, dtype=loss_dtype, device=dev)
        grads = torch.empty((B, T, V), dtype=x.dtype, device=dev)
        if B == 0:
            out = (losses.to(src_device, src_dtype), grads.to(src_device, src_dtype))
            return out if reduction is None else out + (getattr(out[0], reduction)(),)
        code = R.dtype_code(x.dtype)
        nbytes = self._workspace_bytes(B, T, V, Smax, code)
        reduced = torch.empty((), dtype=loss_dtype, device=dev) if reduction else None
        stream = R.stream_handle(dev)
        with _on_device(dev):
            ws = R.workspace(dev, nbytes, stream)
            sB, sT, sV = x.stride()
            self._launch(dev,
                         (x.data_ptr(), code, bool(input_is_logprobs), sB, sT, sV, targets.data_ptr(), targets.stride(0),
                          xl.data_ptr(), tl.data_ptr(), B, T, V, Smax),
                         (losses.data_ptr(), grads.data_ptr(), ws.data_ptr(), ws.numel()),
                         (stream, float(grad_scale), reduced.data_ptr() if reduction else 0,
                          _REDUCTIONS[reduction]))
        if self._redo_flags:
            self._last = (ws, B, T, Smax)
        if src_device != dev or src_dtype != losses.dtype:
            losses = losses.to(src_device, src_dtype)
            if reduction:
                reduced = reduced.to(src_device, src_dtype)
        if src_device != dev or src_dtype != grads.dtype:
            grads = grads.to(src_device, src_dtype)
        return (losses, grads) if reduction is None else (losses, grads, reduced)

    @staticmethod
    def scale_grads_(grads, scale):
        """grads[b] *= scale[b] in place on the GPU (the multiply of functions/forward_backward.py:33 upstream,
        without a second (B,T,V) tensor; rows whose factor is exactly 1 are not touched).  `grads` must be a contiguous
        CUDA tensor, `scale` a (B,) tensor -- or a single element, which then scales the whole tensor."""
        if not (grads.is_cuda and grads.is_contiguous()):
            raise ValueError("scale_grads_ needs a contiguous GPU tensor")
        if scale.device != grads.device or scale.dtype != grads.dtype or not scale.is_contiguous():
            scale = scale.detach().to(device=grads.device, dtype=grads.dtype).contiguous()
        B = grads.shape[0] if scale.numel() != 1 else 1
        if scale.numel() != B:
            raise ValueError("scale must have one entry per utterance (or a single one)")
        if grads.numel():
            with _on_device(grads.device):
                _C.ctc_scale_grads(grads.data_ptr(), R.dtype_code(grads.dtype), scale.data_ptr(), B,
                                   grads.numel() // B, R.stream_handle(grads.device))
        return grads


class CTCLossEngine(_ForwardBackwardEngine):
    """blank_idx -> .compute(logits, targets, logits_lengths, targets_lengths) -> (losses[B], grads[B,T,V])."""

    def __init__(self, blank_idx, algo=R.ALGO_AUTO, f32_chains=False):
        """`f32_chains` (extension, e2e_ctc_loss_opts.chains): let the lattice chains run in packed f32 where that is
        faster (long targets, small alphabets): gradient elements within 2e-5 absolute of the reference instead of 2e-6."""
        self.blank_idx = int(blank_idx)
        self.algo = algo
        self.f32_chains = bool(f32_chains)

    def _takes_16bit(self, x, targets):
        # 16-bit logits (raw autocast outputs): the fast and wide paths read them as they are and write the gradient in
        # the same dtype -- no f32 copy of the (B,T,V) tensors (the reference converts once to double,
        # src/losses/forward_backward.cpp:15,55-56).  Shapes those paths do not take (the library says which:
        # e2e_ctc_loss_takes_dtype) are up-cast.  The gradient of a fresh allocation is 256-byte aligned.
        if self.algo == R.ALGO_EXACT:
            return False
        B, T, V = x.shape
        Smax = targets.shape[1] if targets.dim() == 2 else 0
        sB, sT, sV = x.stride()
        return _C.ctc_loss_takes_dtype(R.dtype_code(x.dtype), self.algo, T, V, Smax, sB, sT, sV, x.data_ptr(), 0)

    def _workspace_bytes(self, B, T, V, Smax, code):
        key = (B, T, V, Smax, code, self.algo)
        nbytes = _ws_bytes.get(key)
        if nbytes is None:
            nbytes = _ws_bytes[key] = _C.ctc_loss_workspace_bytes(B, T, V, Smax, code, self.algo)
        return nbytes

    def _launch(self, dev, call, out, opts):
        _C.ctc_loss_fwd_bwd(*call, self.blank_idx, *out, self.algo, *opts,
                            _C.CHAINS_F32 if self.f32_chains else _C.CHAINS_F64)


class _LatticeLossEngine(_ForwardBackwardEngine):
    """The engines of the one-workgroup-per-utterance lattice kernels (csrc/lattice_common.h): f32 and f64 only, and a
    probability-domain f32 pass that redoes in the f64 log domain the utterances it cannot settle."""

    def _redo_args(self):
        return ()

    def redo_flags(self):
        """Diagnostics (synchronises): per utterance of the last compute(), why it was redone in the f64 log domain -- 0 not
        (or f64 input, or no lattice to run: bad lengths or labels, more labels than frames without blank), 1 the
        probability-domain forward could not settle it (Gram-CTC: infeasible utterances included), 2 the backward found a
        frame whose posteriors do not sum to 1.  Read before another call on the stream reuses the workspace."""
        import ctypes
        from . import _lib
        ws, B, T, Smax = self._last
        out = (ctypes.c_int * B)()
        _lib.check(getattr(_lib.load(), self._redo_flags)(ctypes.c_void_p(ws.data_ptr()), B, T, Smax, *self._redo_args(), out))
        return np.array(out[:], dtype=np.int32)


class CTCWithoutBlankLossEngine(_LatticeLossEngine):
    """space_idx -> .compute(logits, targets, logits_lengths, targets_lengths) -> (losses[B], grads[B,T,V]) for the
    blank-free (ASG-style) lattice of pytorch_end2end/functions/ctc_without_blank.py:13-138 upstream, computed by
    e2e_ctc_noblank_fwd_bwd.  The contract of CTCLossEngine.compute (devices, dtypes, `input_is_logprobs`, `grad_scale`,
    `reduction`), so that ForwardBackwardLossFunction serves it unchanged; 16-bit inputs are up-cast to f32."""

    _redo_flags = "e2e_debug_noblank_redo_flags"

    def __init__(self, space_idx=-1):
        self.space_idx = int(space_idx)

    def _check(self, V):
        if self.space_idx != -1 and not 0 <= self.space_idx < V:
            raise ValueError("space_idx %d is neither -1 nor a label of the %d-column alphabet" % (self.space_idx, V))

    def _workspace_bytes(self, B, T, V, Smax, code):
        return _C.ctc_noblank_workspace_bytes(B, T, V, Smax, code)

    def _launch(self, dev, call, out, opts):
        _C.ctc_noblank_fwd_bwd(*call, self.space_idx, *out, *opts)


def _asg_check(V, Smax=0):
    """The limits of the ASG kernels (e2e_asg_max_labels, e2e_asg_max_target_length), as a ValueError that states them."""
    max_v, max_s = _C.asg_max_labels(), _C.asg_max_target_length()
    if not 1 <= V <= max_v:
        raise ValueError("ASG: an alphabet of %d columns is not supported: 1 to %d (exp(transitions) lives in one "
                         "workgroup's LDS)" % (V, max_v))
    if Smax > max_s:
        raise ValueError("ASG: targets of %d labels are not supported: at most %d" % (Smax, max_s))


def _asg_transitions(transitions, V, dev, dtype):
    if transitions.dim() != 2 or transitions.shape[0] != V or transitions.shape[1] != V:
        raise ValueError("transitions must be (%d, %d) for emissions of %d columns, not %s"
                         % (V, V, V, tuple(transitions.shape)))
    return transitions.detach().to(device=dev, dtype=dtype).contiguous()


_asg_call = threading.local()           # the transitions of the compute() in flight on this thread, and its slab buffer


class ASGLossEngine(_LatticeLossEngine):
    """.compute(emissions, transitions, targets, logits_lengths, targets_lengths) -> (losses[B], grads[B,T,V],
    tgrads[B,V,V]) for ASG with learned transitions, computed by e2e_asg_fwd_bwd (the definition: include/e2e_ctc.h).
    `transitions[j, i]` scores label j after label i; `tgrads[b]` is the utterance's own transition gradient.  The device
    and dtype contract is _ForwardBackwardEngine.compute's: any strides, CPU tensors in give CPU tensors out, losses and
    grads come back in the emissions' dtype; 16-bit inputs are up-cast to f32, and `tgrads` then stays f32 (a sum over the
    frames has no place in 16 bits).  The kernels keep every cell in f64 and have no
    redo route, so there are no redo flags to read."""

    def __init__(self, num_labels=None):
        self.num_labels = None if num_labels is None else int(num_labels)
        if self.num_labels is not None:
            _asg_check(self.num_labels)

    def _check(self, V):
        if self.num_labels is not None and V != self.num_labels:
            raise ValueError("emissions have %d columns; this ASG engine was made for %d" % (V, self.num_labels))
        _asg_check(V)

    def _workspace_bytes(self, B, T, V, Smax, code):
        _asg_check(V, Smax)
        return _C.asg_workspace_bytes(B, T, V, Smax, code)

    def _launch(self, dev, call, out, opts):
        x, code, _, sB, sT, sV, targets, tgt_stride, xl, tl, B, T, V, Smax = call
        A = _asg_call.transitions
        tgrads = _asg_call.tgrads = torch.empty((B, V, V), dtype=A.dtype, device=dev)
        _C.asg_fwd_bwd(x, code, sB, sT, sV, A.data_ptr(), targets, tgt_stride, xl, tl, B, T, V, Smax,
                       out[0], out[1], tgrads.data_ptr(), out[2], out[3], opts[0], opts[1])

    def compute(self, emissions, transitions, targets, logits_lengths, targets_lengths, grad_scale=1.0):
        """`emissions` is batch-major (B,T,V) unnormalised scores (any strides), `transitions` (V,V).  `grad_scale`
        multiplies both gradients as the kernels write them."""
        if emissions.dim() != 3:
            raise ValueError("emissions must be (batch, time, alphabet)")
        B, _, V = emissions.shape
        self._check(V)
        dev = R.compute_device(emissions)
        dtype = emissions.dtype if emissions.dtype in _F32_F64 else torch.float32
        _asg_call.transitions = _asg_transitions(transitions, V, dev, dtype)
        _asg_call.tgrads = None
        try:
            losses, grads = super().compute(emissions, targets, logits_lengths, targets_lengths, True, grad_scale)
            tgrads = _asg_call.tgrads
        finally:
            _asg_call.transitions = _asg_call.tgrads = None
        if tgrads is None:                   # an empty batch: nothing was launched
            tgrads = torch.zeros((B, V, V), dtype=dtype, device=dev)
        if tgrads.device != emissions.device:
            tgrads = tgrads.to(emissions.device)
        return losses, grads, tgrads


class ASGViterbiEngine:
    """.compute(emissions, transitions, logits_lengths) -> (paths (B,T) int64 padded with `pad_value`, scores (B) f64,
    collapsed (B,T) int64 zero padded, lengths (B) int64): the best path of e2e_asg_viterbi (include/e2e_ctc.h).
    Results are CPU tensors, as the other decoders' are, unless `keep_on_device`."""

    def __init__(self, pad_value=-100, keep_on_device=False):
        self.pad_value = int(pad_value)
        self.keep_on_device = bool(keep_on_device)

    def compute(self, emissions, transitions, logits_lengths):
        if emissions.dim() != 3:
            raise ValueError("emissions must be (batch, time, alphabet)")
        B, T, V = emissions.shape
        _asg_check(V)
        dev = R.compute_device(emissions)
        x = emissions.detach().to(dev)
        if x.dtype not in _F32_F64:
            x = x.to(torch.float32)
        A = _asg_transitions(transitions, V, dev, x.dtype)
        xl = _as_long(logits_lengths, dev)
        if xl.numel() != B:
            raise ValueError("logits_lengths must have one entry per utterance")
        path = torch.empty((B, T), dtype=torch.long, device=dev)
        coll = torch.empty((B, T), dtype=torch.long, device=dev)
        scores = torch.empty(B, dtype=torch.float64, device=dev)
        lengths = torch.empty(B, dtype=torch.long, device=dev)
        if B and T:
            stream = R.stream_handle(dev)
            with _on_device(dev):
                ws = R.workspace(dev, _C.asg_viterbi_workspace_bytes(B, T, V), stream)
                sB, sT, sV = x.stride()
                _C.asg_viterbi(x.data_ptr(), R.dtype_code(x.dtype), sB, sT, sV, A.data_ptr(), xl.data_ptr(), B, T, V,
                               path.data_ptr(), self.pad_value, scores.data_ptr(), coll.data_ptr(), lengths.data_ptr(),
                               ws.data_ptr(), ws.numel(), stream)
        else:
            lengths.zero_()
            scores.fill_(float("nan"))
        out = (path, scores, coll, lengths)
        return out if self.keep_on_device else tuple(t.cpu() for t in out)


class ASGBeamEngine:
    """(labels, num_replabels, beam_width_, lm_path, lmwt_, wip_, oov_penalty_, case_sensitive) -> decode_nbest / decode: the
    ASG prefix beam search with transitions and a word language model (e2e_asg_beam_nbest; the definition:
    include/e2e_ctc.h).  `labels`: the character strings of the columns 0 .. V - R - 1 (a list of all V columns is taken
    too; None: no sentences, no space, no model).  The model is loaded once per device through LanguageModel, with the
    labels of all V columns (the repeat columns' strings are never read), at the first call: only the emissions tell
    whether `labels` lists the characters or all columns.  The width limit is checked here when the
    alphabet is known, else at the first call -- before any launch either way.  `restrict()` restricts the search to a
    vocabulary (e2e_asg_beam_nbest_opt); `prune()` sets per-frame label pruning (e2e_asg_beam_nbest_cut).  Results are CPU
    tensors unless `keep_on_device`."""

    def __init__(self, labels=None, num_replabels=0, beam_width_=100, lm_path="", lmwt_=1.0, wip_=0.0,
                 oov_penalty_=-1000.0, case_sensitive=False, keep_on_device=False):
        self.num_replabels = int(num_replabels)
        if self.num_replabels < 0:
            raise ValueError("num_replabels must be >= 0")
        self.beam_width = int(beam_width_)
        self.labels = None if labels is None else list(labels)
        self.lmwt = float(lmwt_) if lm_path else 0.0
        self.wip = float(wip_)
        self.oov_penalty = float(oov_penalty_)
        self.case_sensitive = bool(case_sensitive)
        self.keep_on_device = bool(keep_on_device)
        self.num_labels = None                       # V, once it is known
        self.lm = None
        self.restricted = False
        self._words = None                           # restrict(lexicon=...): the word list of the model that scores nothing
        self.cutoff_top_n = None                     # prune(): per-frame label pruning, off
        if self.beam_width < 1 or self.beam_width > _C.asg_beam_max_width(1):
            raise ValueError("beam_width %d is not supported: 1 to %d" % (self.beam_width, _C.asg_beam_max_width(1)))
        self._lm_path = lm_path or ""
        if self._lm_path:
            if self.labels is None:
                raise ValueError("a language model needs the labels: the alphabet spells its words")
            R.require_gpu()

    def restrict(self, lexicon=None):
        """Restrict the search to a vocabulary (the definition: e2e_asg_beam_nbest_opt); returns self.  `lexicon` None: the
        words of the language model of `lm_path`.  `lexicon` an iterable of words: the model that scores nothing is built
        from them (e2e_lm_load_words) -- `lmwt` and `oov_penalty` then count as 0, `wip` applies; not together with `lm_path`.
        The model is loaded, and its lexicon built, when the number of columns is known."""
        if self.labels is None:
            raise ValueError("restrict needs the labels: the alphabet spells the vocabulary's words")
        if lexicon is not None and self._lm_path:
            raise ValueError("lm_path and lexicon exclude each other (a lexicon together with a language model is not supported)")
        if lexicon is None and not self._lm_path and self._words is None:
            raise ValueError("restrict needs a vocabulary: lm_path or lexicon")
        if lexicon is not None:
            words = _lexicon_words(lexicon)
            R.require_gpu()
            self._words = words
            self.lmwt = 0.0
            self.oov_penalty = 0.0
            self.lm = None
        self.restricted = True
        if self.num_labels is not None:
            self._load_model(self.num_labels)
        return self

    def prune(self, cutoff_top_n):
        """Per-frame label pruning (the definition: e2e_asg_beam_nbest_cut, include/e2e_ctc.h); returns self.  A frame expands
        its `cutoff_top_n` highest-scoring labels alone, and a member whose last label is not among them does not stay.
        None: not pruned, as is a `cutoff_top_n` that is no less than the alphabet.  decode, decode_nbest and the streams
        opened afterwards use it.  There is no cutoff_prob: ASG emissions are scores, not probabilities."""
        if cutoff_top_n is not None and (isinstance(cutoff_top_n, bool) or not isinstance(cutoff_top_n, (int, np.integer))
                                         or cutoff_top_n < 1):
            raise ValueError("cutoff_top_n=%r: at least 1" % (cutoff_top_n,))
        self.cutoff_top_n = None if cutoff_top_n is None else int(cutoff_top_n)
        return self

    def _cut(self, V):
        """cutoff_top_n as the C calls take it if the search prunes an alphabet of V columns, else None: the unpruned entries."""
        return self.cutoff_top_n if self.cutoff_top_n is not None and self.cutoff_top_n < V else None

    def _load_model(self, V):
        """The model over all V columns (the repeat columns' strings are never spelled), with its lexicon if restricted."""
        labels = self.labels[: V - self.num_replabels] + ["<%d>" % (r + 1) for r in range(self.num_replabels)]
        if self.lm is None:
            if self._words is not None:
                self.lm = LanguageModel(None, labels, self.case_sensitive, words=self._words, lexicon=True)
            elif self._lm_path:
                self.lm = LanguageModel(self._lm_path, labels, self.case_sensitive)
        if self.restricted and not self.lm.has_lexicon():
            self.lm.enable_lexicon()

    def _chars(self):
        return self.labels if self.num_labels is None else self.labels[: self.num_labels - self.num_replabels]

    def _bind(self, V):
        """The alphabet's size is known: the limits, the labels' count, the space."""
        if self.num_labels == V:
            return
        if self.num_labels is not None:
            raise ValueError("emissions have %d columns; this decoder was used with %d before" % (V, self.num_labels))
        _asg_check(V)
        num_chars = V - self.num_replabels
        if num_chars < 1:
            raise ValueError("%d columns leave no characters beside %d repeat labels" % (V, self.num_replabels))
        if self.labels is not None and len(self.labels) not in (num_chars, V):
            raise ValueError("the decoder has %d labels but the emissions have %d columns, %d of them repeat labels"
                             % (len(self.labels), V, self.num_replabels))
        cap = _C.asg_beam_max_width(V)
        if self.beam_width > cap:
            raise ValueError("beam_width %d is not supported for an ASG alphabet of %d columns: 1 to %d"
                             % (self.beam_width, V, cap))
        chars = self.labels[:num_chars] if self.labels is not None else []
        self.space_id = chars.index(" ") if " " in chars else -1
        if self._lm_path or self._words is not None:  # loaded once, now that the number of columns is known
            self._load_model(V)
        self.num_labels = V

    def _strings(self, rows, lens):
        if self.labels is None:
            return ["" for _ in lens]
        chars, out = self._chars(), []
        for row, n in zip(rows.tolist(), lens):
            s = []
            for i in row[:n]:
                if i < len(chars):
                    s.append(chars[i])
                elif s:
                    s.extend([s[-1]] * (i - len(chars) + 1))
            out.append("".join(s))
        return out

    def decode_nbest(self, emissions, transitions, logits_lengths, nbest=None, timesteps=False):
        """-> (ids (B,N,maxlen) int64 -- the merged labels, repeat labels as they are --, lengths (B,N), sentences [B][n_hyp]
        with the repeat labels expanded, scores (B,N) f64, acoustic scores, lm_scores, num_words (B,N) int32, num_oov (B,N),
        num_hypotheses (B), timesteps): CTCDecoderEngine.decode_nbest's tuple.  `transitions` None: all zero.  `timesteps`:
        (B,N,maxlen) int64, the frame at which each label's sequence last entered the beam, -1 behind a sequence, cut to the
        longest result as `ids` is; None unless asked for."""
        N = self.beam_width if nbest is None else int(nbest)
        if not 1 <= N <= self.beam_width:
            raise ValueError("nbest=%d outside [1, beam_width=%d]" % (N, self.beam_width))
        if emissions.dim() != 3:
            raise ValueError("emissions must be (batch, time, alphabet)")
        B, T, V = emissions.shape
        self._bind(V)
        dev = R.compute_device(emissions)
        x = emissions.detach().to(dev)
        if x.dtype not in _F32_F64:
            x = x.to(torch.float32)
        A = None if transitions is None else _asg_transitions(transitions, V, dev, x.dtype)
        xl = _as_long(logits_lengths, dev)
        if xl.numel() != B:
            raise ValueError("logits_lengths must have one entry per utterance")
        max_out = max(T, 1)
        # (an utterance whose length is outside [1, T] is not touched by the call: its slots are the empty ones from here)
        bufs = out, out_len, n_hyp, scores, counts, ts = _nbest_buffers(B, N, max_out, dev, timesteps=timesteps, prefill="all")
        if B and T:
            stream = R.stream_handle(dev)
            with _on_device(dev):
                lm = self.lm.on(dev).handle if self.lm is not None else 0
                cut = self._cut(V)
                if cut:
                    nbytes = _AsgCut.query("workspace_bytes", B, T, V, self.beam_width, self.lm is not None, cut)
                else:
                    nbytes = _C.asg_beam_workspace_bytes(B, T, V, self.beam_width, self.lm is not None)
                if not nbytes:
                    raise ValueError("ASG beam search: %d frames at beam_width %d are not supported" % (T, self.beam_width))
                ws = R.workspace(dev, nbytes, stream)
                sB, sT, sV = x.stride()
                args = (x.data_ptr(), R.dtype_code(x.dtype), sB, sT, sV, A.data_ptr() if A is not None else 0,
                        xl.data_ptr(), B, T, V, self.num_replabels, self.beam_width, self.space_id, lm,
                        self.lmwt, self.wip, self.oov_penalty, N, out.data_ptr(), max_out, out_len.data_ptr(),
                        n_hyp.data_ptr(), scores.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel(), stream)
                opts = (self.restricted, ts.data_ptr() if ts is not None else 0)
                if cut:
                    _AsgCut.call("e2e_asg_beam_nbest_cut", *args, opts, cut)
                else:
                    _C.asg_beam_nbest(*args, *opts)
        return _nbest_result(self, *bufs)

    def _check_nbest(self, nh, lens, max_out):
        pass                                         # (no status rides on the results: the search cannot run out of anything)

    def decode(self, emissions, transitions, logits_lengths):
        """Hypothesis 0 of decode_nbest -> (ids (B,maxlen) int64, lengths (B), sentences)."""
        return _first_hypothesis(self.decode_nbest(emissions, transitions, logits_lengths, nbest=1))

    def open_stream(self, transitions, batch_size, max_frames, device=None, timesteps=False):
        """Streaming beam search (e2e_asg_beam_stream, include/e2e_ctc.h): an ASGBeamStream that is fed emissions in chunks
        and keeps the beams of `batch_size` utterances of up to `max_frames` frames on the GPU between the chunks.
        `transitions` (None: all zero) are given once, here.  After every chunk the result is, bit for bit, that of
        decode / decode_nbest on all the frames fed so far."""
        return ASGBeamStream(self, transitions, batch_size, max_frames, device=device, timesteps=timesteps)


class ASGBeamStream(_BeamStream):
    """The ASG beams of `batch_size` utterances, kept on the GPU between chunks (ASGBeamEngine.open_stream): _BeamStream, fed
    emissions.  The transitions are the stream's: converted to a chunk's dtype on first use and kept."""

    _INPUT = "emissions"
    _PREFILL = "all"                     # (an utterance that has been fed no frame is not touched by the call)

    def __init__(self, engine, transitions, batch_size, max_frames, device=None, timesteps=False):
        super().__init__(engine, batch_size, max_frames, device=device, timesteps=timesteps)
        self.cutoff_top_n = engine.cutoff_top_n   # (the engine's setting when the stream was opened: the same for every chunk)
        self.transitions = None if transitions is None else transitions.detach()
        self._A = {}                              # dtype -> the transitions on the stream's device

    def _row_bytes(self, V):
        e = self.engine
        return _C.asg_beam_stream_row_bytes(self.max_frames, V, e.beam_width, e.lm is not None)

    def _transitions_for(self, V, dev, dtype):
        if self.transitions is None:
            return None
        A = self._A.get(dtype)
        if A is None:
            A = self._A[dtype] = _asg_transitions(self.transitions, V, dev, dtype)
        return A

    def _prepare(self, emissions, lengths):
        self.engine._bind(emissions.shape[2])
        dev = R.compute_device(emissions)
        x = emissions.detach().to(dev)
        if x.dtype not in _F32_F64:
            x = x.to(torch.float32)
        xl = _as_long(lengths, dev)
        if xl.numel() != x.shape[0]:
            raise ValueError("lengths must have one entry per utterance")
        return x, xl, dev

    def _max_out(self, frames):
        return frames

    def _launch(self, x, xl, state, N, max_out, bufs, frames_done, stream):
        e, dev = self.engine, x.device
        B, Tc, V = x.shape
        out, out_len, n_hyp, scores, counts, ts = bufs
        A = self._transitions_for(V, dev, x.dtype)
        lm = e.lm.on(dev).handle if e.lm is not None else 0
        cut = self.cutoff_top_n if self.cutoff_top_n is not None and self.cutoff_top_n < V else None
        if cut:
            nbytes = _AsgCut.query("stream_workspace_bytes", B, Tc, V, e.beam_width, e.lm is not None, cut)
        else:
            nbytes = _C.asg_beam_stream_workspace_bytes(B, V, e.beam_width, e.lm is not None)
        ws = R.workspace(dev, nbytes, stream)
        sB, sT, sV = x.stride()
        args = (x.data_ptr(), R.dtype_code(x.dtype), sB, sT, sV, A.data_ptr() if A is not None else 0,
                xl.data_ptr(), B, Tc, V, e.num_replabels, e.beam_width, e.space_id, lm,
                e.lmwt, e.wip, e.oov_penalty, state.data_ptr(), self.row_bytes, self.max_frames, N,
                out, max_out, out_len, n_hyp, scores, counts, frames_done, ws.data_ptr(), ws.numel(), stream)
        if cut:
            _AsgCut.call("e2e_asg_beam_stream_cut", *args, (e.restricted, ts), cut)
        else:
            _C.asg_beam_stream(*args, e.restricted, ts)


GRAM_MAX_ORDER = 8


def gram_columns(num_base_labels, total_labels, label2ids):
    """Check upstream's (num_base_labels, total_labels, label2ids) and return ({column: base-id tuple} for the columns
    1 .. V-1, max_order, {key: column}).  Column 0 is the blank, columns 1 .. R-1 the unigrams, every column R .. V-1 a
    gram of label2ids (a sequence of 1..8 base ids in [1, R)); the key of a gram is its sequence read as a number in radix
    R (upstream's get_hash, src/losses/gram_ctc_loss.cpp:22-28), and keys must be distinct."""
    R, V = int(num_base_labels), int(total_labels)
    if not 1 <= R <= V:
        raise ValueError("num_base_labels %d and total_labels %d: need 1 <= num_base_labels <= total_labels" % (R, V))
    grams = {c: (c,) for c in range(1, R)}
    for key, ids in dict(label2ids).items():
        c = int(key)
        if c != key or not 1 <= c < V:
            raise ValueError("label2ids key %r is not a column in [1, %d)" % (key, V))
        seq = tuple(int(i) for i in ids)
        if not 1 <= len(seq) <= GRAM_MAX_ORDER:
            raise ValueError("column %d: a gram has 1 to %d base labels, not %d" % (c, GRAM_MAX_ORDER, len(seq)))
        if any(not 1 <= i < R for i in seq):
            raise ValueError("column %d: base label ids must be in [1, %d): %r" % (c, R, list(ids)))
        if c < R and seq != (c,):
            raise ValueError("column %d is the unigram [%d], not %r" % (c, c, list(ids)))
        grams[c] = seq
    missing = [c for c in range(R, V) if c not in grams]
    if missing:
        raise ValueError("label2ids has no entry for the gram columns %s" % missing[:10])
    order = max((len(g) for g in grams.values()), default=1)
    if R ** order > 2 ** 63 - 1:
        raise ValueError("num_base_labels %d ** max_order %d overflows int64 keys" % (R, order))
    keys = {}
    for c in sorted(grams):
        k = 0
        for i in grams[c]:
            k = k * R + i
        if k in keys:
            raise ValueError("columns %d and %d spell the same gram %r" % (keys[k], c, list(grams[c])))
        keys[k] = c
    return grams, order, keys


def gram_table(num_base_labels, total_labels, label2ids):
    """The gram table of e2e_gram_ctc_fwd_bwd from upstream's (num_base_labels, total_labels, label2ids), checked by
    gram_columns: (keys int64 sorted ascending, their columns int32, max_order), host arrays."""
    _, order, keys = gram_columns(num_base_labels, total_labels, label2ids)
    ks = sorted(keys)
    return np.array(ks, dtype=np.int64), np.array([keys[k] for k in ks], dtype=np.int32), order


class GramCTCLossEngine(_LatticeLossEngine):
    """(blank_idx, num_base_labels, total_labels, label2ids) -> .compute(logits, targets, logits_lengths,
    targets_lengths) -> (losses[B], grads[B,T,V]) for Gram-CTC, computed by e2e_gram_ctc_fwd_bwd (the definition:
    include/e2e_ctc.h).  The contract of CTCLossEngine.compute, so that ForwardBackwardLossFunction serves it unchanged;
    16-bit inputs are up-cast to f32.  Construction checks the table on the host; the device copy is made on first use
    and kept per device."""

    _redo_flags = "e2e_debug_gram_redo_flags"

    def __init__(self, blank_idx, num_base_labels, total_labels, label2ids):
        if int(blank_idx) != 0:
            raise NotImplementedError("Gram-CTC supports blank_idx=0 only (as upstream)")
        self.blank_idx = 0
        self.num_base_labels = int(num_base_labels)
        self.total_labels = int(total_labels)
        self._keys, self._cols, self.max_order = gram_table(num_base_labels, total_labels, label2ids)
        self._per_device = {}

    def _redo_args(self):
        return (self.max_order,)

    def _table(self, dev):
        t = self._per_device.get(dev.index)
        if t is None:
            t = (torch.from_numpy(self._keys).to(dev), torch.from_numpy(self._cols).to(dev))
            self._per_device[dev.index] = t
        return t

    def max_target_length(self):
        """The longest target the kernel serves at this table's max_order (its rows live in one workgroup's LDS)."""
        lo, hi = 0, 1 << 16
        while lo < hi:
            mid = (lo + hi + 1) // 2
            if _C.gram_ctc_workspace_bytes(1, 1, self.total_labels, mid, self.max_order, _C.F32) > 0:
                lo = mid
            else:
                hi = mid - 1
        return lo

    def _check(self, V):
        if V != self.total_labels:
            raise ValueError("logits have %d columns; this Gram-CTC table has total_labels=%d" % (V, self.total_labels))

    def _workspace_bytes(self, B, T, V, Smax, code):
        nbytes = _C.gram_ctc_workspace_bytes(B, T, V, Smax, self.max_order, code)
        if nbytes == 0:
            raise ValueError("Gram-CTC: targets of %d labels exceed the %d the kernel serves at max_order %d"
                             % (Smax, self.max_target_length(), self.max_order))
        return nbytes

    def _launch(self, dev, call, out, opts):
        keys, cols = self._table(dev)
        _C.gram_ctc_fwd_bwd(*call, keys.data_ptr(), cols.data_ptr(), keys.numel(), self.num_base_labels, self.max_order,
                            *out, *opts)


class GramCTCDecoderEngine:
    """(blank_idx, num_base_labels, total_labels, label2ids, beam_width_=100, labels=None) -> decode_greedy /
    decode_nbest for Gram-CTC (e2e_gram_ctc_greedy, e2e_gram_ctc_beam_nbest; the definition: include/e2e_ctc.h).  The table
    check is GramCTCLossEngine's (gram_columns); the decoders take the table spelled out -- (V,8) base ids and (V) lengths
    -- copied to a device on first use and kept per device.  `labels`: the R base-label strings (index 0 the blank's).
    The width limit is checked here, not at the first decode.  `configure()` sets up the search with a word language
    model (e2e_gram_ctc_beam_nbest_lm); an engine that was never configured is the search on the masses alone.  `restrict()`,
    after `configure()`, restricts the search to a vocabulary (e2e_gram_ctc_beam_nbest_opt).  `cutoff_top_n`, `cutoff_prob`:
    per-frame label pruning, CTCDecoderEngine's knobs -- decode, decode_nbest and open_stream then go to the *_cut entries
    (e2e_gram_ctc_beam_nbest_cut, e2e_gram_ctc_beam_stream_cut), a search that prunes nothing to the entries above; the width
    limit is then e2e_gram_beam_cut_max_width's.  Results are CPU tensors unless `keep_on_device`."""

    def __init__(self, blank_idx, num_base_labels, total_labels, label2ids, beam_width_=100, labels=None,
                 keep_on_device=False, cutoff_top_n=None, cutoff_prob=1.0):
        if int(blank_idx) != 0:
            raise NotImplementedError("Gram-CTC supports blank_idx=0 only (as upstream)")
        self.blank_idx = 0
        self.num_base_labels = int(num_base_labels)
        self.total_labels = int(total_labels)
        grams, self.max_order, _ = gram_columns(num_base_labels, total_labels, label2ids)
        self._ids = np.zeros((self.total_labels, GRAM_MAX_ORDER), dtype=np.int32)
        self._len = np.zeros(self.total_labels, dtype=np.int32)
        for c, seq in grams.items():
            self._ids[c, :len(seq)] = seq
            self._len[c] = len(seq)
        self.beam_width = int(beam_width_)
        self.labels = list(labels or [])
        if self.labels and len(self.labels) != self.num_base_labels:
            raise ValueError("the decoder has %d labels but num_base_labels=%d" % (len(self.labels), self.num_base_labels))
        self.keep_on_device = bool(keep_on_device)
        # per-frame label pruning (the definition: e2e_gram_ctc_beam_nbest_cut, include/e2e_ctc.h): a frame expands at most
        # cutoff_top_n columns and of those the fewest whose probabilities sum to cutoff_prob, the blank always.  None / 1.0
        # (or a cutoff_top_n that is no less than total_labels): not pruned.  configure() and restrict() keep them
        self._set_cut(cutoff_top_n, cutoff_prob)
        cut = self._cut()
        cap = (_GramCut.query("max_width", self.total_labels, self.max_order, cut[0]) if cut
               else _C.gram_beam_max_width(self.total_labels, self.max_order))
        if self.beam_width < 1 or self.beam_width > cap:
            raise ValueError("beam_width %d is not supported for a Gram-CTC table of %d columns (max_order %d)%s: 1 to %d"
                             % (self.beam_width, self.total_labels, self.max_order,
                                " with cutoff_top_n=%d" % cut[0] if cut else "", cap))
        self._per_device = {}
        self.configured = False                      # configure(): the search with the LM fields (e2e_gram_ctc_beam_nbest_lm)
        self.lm = None
        self.restricted = False                      # restrict(): only admissible sequences (e2e_gram_ctc_beam_nbest_opt)

    def _cut(self):
        """(cutoff_top_n, cutoff_prob) as the C calls take them if the decoder prunes its table's columns, else None: a search
        that prunes nothing goes to the unpruned entries."""
        V = self.total_labels
        top_n = V if self.cutoff_top_n is None else self.cutoff_top_n
        return (top_n, self.cutoff_prob) if top_n < V or self.cutoff_prob < 1.0 else None

    def _set_cut(self, cutoff_top_n, cutoff_prob):
        if cutoff_top_n is not None and int(cutoff_top_n) < 1:
            raise ValueError("cutoff_top_n=%r: at least 1" % (cutoff_top_n,))
        if not 0.0 < float(cutoff_prob) <= 1.0:
            raise ValueError("cutoff_prob=%r outside (0, 1]" % (cutoff_prob,))
        if (cutoff_top_n is not None or float(cutoff_prob) < 1.0) and self.beam_width == 1:
            raise ValueError("cutoff_top_n / cutoff_prob need beam_width > 1: greedy decoding expands nothing")
        top_n = None if cutoff_top_n is None else int(cutoff_top_n)
        CTCDecoderEngine.check_cut_limit(self.total_labels, top_n, float(cutoff_prob))
        self.cutoff_top_n, self.cutoff_prob = top_n, float(cutoff_prob)

    def configure(self, lm_path="", lmwt_=1.0, wip_=0.0, oov_penalty_=-1000.0, case_sensitive=False):
        """Set up the beam search with a word language model (e2e_gram_ctc_beam_nbest_lm; the definition: include/e2e_ctc.h);
        returns self.  The names and defaults are CTCDecoderEngine's.  The model is loaded here, once, over the
        num_base_labels label strings (LanguageModel keeps a copy per device); `lm_path` empty: no model -- `lmwt_` counts
        as 0, `wip_` still applies per word.  decode_nbest then returns CTCDecoderEngine.decode_nbest's tuple.  A later call
        replaces the former one, and drops a restriction (restrict())."""
        if not self.labels:
            raise ValueError("a configured Gram-CTC search needs the labels: the base labels' strings spell the language "
                             "model's words, and the space among them separates the words")
        if self.beam_width == 1:
            raise ValueError("beam_width 1 is greedy decoding, which carries no language model: configure() needs beam_width > 1")
        lm_path = lm_path or ""
        self.lm = None
        self.restricted = False
        self._lm_path = lm_path
        if lm_path:
            R.require_gpu()
            self.lm = LanguageModel(lm_path, self.labels, bool(case_sensitive))
        self.lmwt = float(lmwt_) if lm_path else 0.0
        self.wip = float(wip_)
        self.oov_penalty = float(oov_penalty_)
        self.case_sensitive = bool(case_sensitive)
        self.space_id = self.labels.index(" ") if " " in self.labels else -1
        self.configured = True
        return self

    def restrict(self, lexicon=None):
        """Restrict the configured search to a vocabulary (the definition: e2e_gram_ctc_beam_nbest_opt); returns self.
        `lexicon` None: the words of the language model of configure()'s `lm_path`, whose lexicon is enabled.  `lexicon` a path
        (a text file, one word per line or white space between the words) or an iterable of words: the model that scores
        nothing is built from them (e2e_lm_load_words) -- `lmwt` and `oov_penalty` then count as 0, `wip` applies; not together
        with `lm_path`.  A later configure() drops the restriction."""
        if not self.configured:
            raise ValueError("restrict needs a configured search: call configure() first (configure(wip=0) for no model and no penalty)")
        if lexicon is not None and self._lm_path:
            raise ValueError("lm_path and lexicon exclude each other (a lexicon together with a language model is not supported)")
        if lexicon is None and self.lm is None:
            raise ValueError("restrict needs a vocabulary: configure(lm_path=...) or lexicon")
        if lexicon is not None:
            words = _lexicon_words(lexicon)
            R.require_gpu()
            self.lm = LanguageModel(None, self.labels, self.case_sensitive, words=words, lexicon=True)
            self.lmwt = 0.0
            self.oov_penalty = 0.0
        elif not self.lm.has_lexicon():
            self.lm.enable_lexicon()
        self.restricted = True
        return self

    def _table(self, dev):
        t = self._per_device.get(dev.index)
        if t is None:
            t = (torch.from_numpy(self._ids).to(dev), torch.from_numpy(self._len).to(dev))
            self._per_device[dev.index] = t
        return t

    def _prep(self, logits_, logits_lengths_, dtypes):
        if logits_.dim() != 3:
            raise ValueError("logits must be (batch, time, alphabet)")
        if logits_.shape[2] != self.total_labels:
            raise ValueError("logits have %d columns; this Gram-CTC table has total_labels=%d"
                             % (logits_.shape[2], self.total_labels))
        dev = R.compute_device(logits_)
        x = logits_.detach()
        if x.dtype not in dtypes:
            x = x.to(torch.float32)
        x = x.to(dev)
        xl = _as_long(logits_lengths_, dev)
        if xl.numel() != x.shape[0]:
            raise ValueError("logits_lengths_ must have one entry per utterance")
        return x, xl, dev

    def _result(self, t):
        return t if self.keep_on_device else t.cpu()

    def _strings(self, rows, lens):
        if not self.labels:
            return ["" for _ in lens]
        return ["".join(self.labels[k] for k in row[:n]) for row, n in zip(rows.tolist(), lens)]

    def decode_greedy(self, logits_, logits_lengths_, return_columns=False):
        """argmax + collapse + gram expansion -> (base ids (B, T*max_order) int64 zero padded, lengths (B), sentences);
        with return_columns also (columns (B,T) int64 zero padded, their lengths (B)): the grams the model chose."""
        x, xl, dev = self._prep(logits_, logits_lengths_, _F32_F64 + _16BIT)
        B, T, V = x.shape
        out = torch.empty((B, T * self.max_order), dtype=torch.long, device=dev)
        out_len = torch.empty(B, dtype=torch.long, device=dev)
        cols = torch.empty((B, T), dtype=torch.long, device=dev)
        cols_len = torch.empty(B, dtype=torch.long, device=dev)
        if B and T:
            with torch.cuda.device(dev):
                ids, lens = self._table(dev)
                sB, sT, sV = x.stride()
                _C.gram_ctc_greedy(x.data_ptr(), R.dtype_code(x.dtype), sB, sT, sV, xl.data_ptr(), B, T, V,
                                   ids.data_ptr(), lens.data_ptr(), self.max_order, out.data_ptr(), out_len.data_ptr(),
                                   cols.data_ptr(), cols_len.data_ptr(), R.stream_handle(dev))
        else:
            out_len.zero_()
            cols_len.zero_()
        out, out_len = self._result(out), self._result(out_len)
        res = (out, out_len, self._strings(out.cpu(), out_len.tolist()))
        return res + (self._result(cols), self._result(cols_len)) if return_columns else res

    def decode_nbest(self, logits_, logits_lengths_, nbest=None, timesteps=False):
        """Prefix beam search on LOG-PROBABILITIES, read out as an n-best list -> (base ids (B,N,maxlen) int64, lengths
        (B,N), sentences [B][n_hyp], scores (B,N) f64 = log probability of the labelling within the beam, num_hypotheses
        (B)).  Ranked by score, ties by the prefix key; slots beyond num_hypotheses[b] are empty (length 0, -inf).
        After configure(): CTCDecoderEngine.decode_nbest's tuple (ids, lengths, sentences, scores, acoustic scores, lm_scores,
        num_words, num_oov, num_hypotheses, timesteps), ranked by scores = acoustic + lmwt * lm - wip * words + oov_penalty * oovs.
        `timesteps` (a configured search only): (B,N,maxlen) int64, the frame at which the node that carries each id was created
        (the ids of one gram share it), -1 behind a sequence, cut to the longest result as the ids are; None unless asked for."""
        N = self.beam_width if nbest is None else int(nbest)
        if not 1 <= N <= self.beam_width:
            raise ValueError("nbest=%d outside [1, beam_width=%d]" % (N, self.beam_width))
        if timesteps and not self.configured:
            raise ValueError("timesteps are part of the configured search's results: call configure() first "
                             "(configure(wip=0) is the search without a model and without penalties)")
        x, xl, dev = self._prep(logits_, logits_lengths_, _F32_F64)
        if self.configured:
            return self._decode_nbest_lm(x, xl, dev, N, bool(timesteps))
        B, T, V = x.shape
        max_out = max(T * self.max_order, 1)
        bufs = out, out_len, n_hyp, scores, _, _ = _nbest_buffers(B, N, max_out, dev, scored=False)
        if B:
            with torch.cuda.device(dev):
                ids, lens = self._table(dev)
                cut = self._cut()
                nbytes = (_GramCut.query("workspace_bytes", B, T, V, self.max_order, self.beam_width, False, False, cut[0]) if cut
                          else _C.gram_beam_workspace_bytes(B, T, V, self.max_order, self.beam_width))
                if not nbytes:
                    raise ValueError("Gram-CTC beam search: %d frames at beam_width %d are not supported" % (T, self.beam_width))
                ws = R.workspace(dev, nbytes)
                sB, sT, sV = x.stride()
                if cut:
                    _GramCut.call("e2e_gram_ctc_beam_nbest_cut", x.data_ptr(), R.dtype_code(x.dtype), sB, sT, sV, xl.data_ptr(), B, T, V,
                                               ids.data_ptr(), lens.data_ptr(), self.max_order, self.num_base_labels,
                                               self.beam_width, False, -1, 0, 0.0, 0.0, 0.0, N,
                                               out.data_ptr(), max_out, out_len.data_ptr(), n_hyp.data_ptr(), scores.data_ptr(),
                                               0, ws.data_ptr(), ws.numel(), R.stream_handle(dev), None, *cut)
                else:
                    _C.gram_ctc_beam_nbest(x.data_ptr(), R.dtype_code(x.dtype), sB, sT, sV, xl.data_ptr(), B, T, V,
                                           ids.data_ptr(), lens.data_ptr(), self.max_order, self.beam_width, N,
                                           out.data_ptr(), max_out, out_len.data_ptr(), n_hyp.data_ptr(), scores.data_ptr(),
                                           ws.data_ptr(), ws.numel(), R.stream_handle(dev))
        return _nbest_result(self, *bufs)

    def _check_nbest(self, nh, lens, max_out):
        """An utterance whose search ran out of entries raises (the status rides on num_hypotheses)."""
        for b, n in enumerate(nh):
            if n < 0:
                raise R.E2EError("Gram-CTC beam search: utterance %d ran out of candidate entries" % b)

    def _decode_nbest_lm(self, x, xl, dev, N, timesteps=False):
        """decode_nbest after configure(): the search on the totals (e2e_gram_ctc_beam_nbest_lm; restricted or with timesteps:
        e2e_gram_ctc_beam_nbest_opt)."""
        B, T, V = x.shape
        max_out = max(T * self.max_order, 1)
        bufs = out, out_len, n_hyp, scores, counts, ts = _nbest_buffers(B, N, max_out, dev, timesteps=timesteps, prefill="ts")
        if B:
            stream = R.stream_handle(dev)
            with torch.cuda.device(dev):
                ids, lens = self._table(dev)
                lm = self.lm.on(dev).handle if self.lm is not None else 0
                cut = self._cut()
                nbytes = (_GramCut.query("workspace_bytes", B, T, V, self.max_order, self.beam_width, True, self.lm is not None, cut[0])
                          if cut else _C.gram_beam_workspace_bytes_lm(B, T, V, self.max_order, self.beam_width, self.lm is not None))
                if not nbytes:
                    raise ValueError("Gram-CTC beam search: %d frames at beam_width %d are not supported" % (T, self.beam_width))
                ws = R.workspace(dev, nbytes, stream)
                sB, sT, sV = x.stride()
                args = (x.data_ptr(), R.dtype_code(x.dtype), sB, sT, sV, xl.data_ptr(), B, T, V,
                        ids.data_ptr(), lens.data_ptr(), self.max_order, self.num_base_labels,
                        self.beam_width, self.space_id, lm, self.lmwt, self.wip, self.oov_penalty, N,
                        out.data_ptr(), max_out, out_len.data_ptr(), n_hyp.data_ptr(), scores.data_ptr(),
                        counts.data_ptr(), ws.data_ptr(), ws.numel(), stream)
                opts = (self.restricted, ts.data_ptr() if ts is not None else 0)
                if cut:                                          # (args with `scored` in its place: behind beam_width)
                    _GramCut.call("e2e_gram_ctc_beam_nbest_cut", *args[:14], True, *args[14:], opts, *cut)
                elif self.restricted or ts is not None:
                    _C.gram_ctc_beam_nbest_opt(*args, (self.restricted, ts.data_ptr() if ts is not None else 0))
                else:
                    _C.gram_ctc_beam_nbest_lm(*args)
        return _nbest_result(self, *bufs)

    def decode(self, logits_, logits_lengths_):
        """Hypothesis 0 of decode_nbest -> (base ids (B,maxlen) int64, lengths (B), sentences)."""
        return _first_hypothesis(self.decode_nbest(logits_, logits_lengths_, nbest=1))

    def open_stream(self, batch_size, max_frames, device=None, timesteps=False):
        """Streaming beam search (e2e_gram_ctc_beam_stream, include/e2e_ctc.h): a GramBeamStream that is fed log-probabilities
        in chunks and keeps the beams of `batch_size` utterances of up to `max_frames` frames on the GPU between the chunks.
        After every chunk the result is, bit for bit, that of decode / decode_nbest on all the frames fed so far.  The
        configuration and the restriction in force now are the stream's.  `timesteps` needs a configured engine."""
        return GramBeamStream(self, batch_size, max_frames, device=device, timesteps=timesteps)


def read_transcriptions(transcriptions, labels, blank_idx=None):
    """The entries of a transcription lexicon as [(word, [label ids])], in order: from the text file at a path (wav2letter's
    format: one entry per line, `word tok tok ...`, split at white space), from a mapping word -> tokens or -> a list of
    token sequences (variants), or from an iterable of (word, tokens).  Tokens are label strings, matched exactly; an
    unknown token, the blank or the space as a token is a ValueError that names the entry."""
    if isinstance(transcriptions, (str, bytes, os.PathLike)):
        path = os.fsdecode(transcriptions)
        if not os.path.isfile(path):
            raise ValueError("Can't find a transcription lexicon: {}".format(path))
        with open(path, encoding="utf-8") as f:
            entries = [(ln.split()[0], ln.split()[1:]) for ln in f.read().splitlines() if ln.split()]
    elif hasattr(transcriptions, "items"):
        entries = []
        for w, t in transcriptions.items():
            variants = [t] if (isinstance(t, str) or not t or isinstance(t[0], str)) else t
            entries += [(w, v) for v in variants]
    else:
        entries = [(w, t) for w, t in transcriptions]
    index = {}
    for i, s in enumerate(labels):
        index.setdefault(s, i)
    out = []
    for n, (w, toks) in enumerate(entries):
        toks = toks.split() if isinstance(toks, str) else list(toks)
        name = "entry %d (%s)" % (n, w)
        if not toks:
            raise ValueError("transcriptions: %s has no tokens" % name)
        ids = []
        for t in toks:
            if t not in index:
                raise ValueError("transcriptions: %s: the token %r is none of the labels" % (name, t))
            if t == " ":
                raise ValueError("transcriptions: %s: the space is the word boundary and no token" % name)
            if blank_idx is not None and index[t] == blank_idx:
                raise ValueError("transcriptions: %s: the blank %r is no token" % (name, t))
            ids.append(index[t])
        out.append((str(w), ids))
    if not out:
        raise ValueError("transcriptions: the lexicon is empty")
    return out


class LanguageModel:
    """n-gram model read from an ARPA file (plain or .gz); stands where KenLM stands upstream
    (ctc_decoder.cpp:60-71).  The device tables belong to one GPU: `on(device)` returns the copy for that device,
    loading it on first use.  With `words` (and no path) it is the model that scores nothing, built from a word list
    (e2e_lm_load_words).  `lexicon=True`, or `enable_lexicon()` later, gives every copy the lexicon a search can be
    restricted to; unrestricted decoders may go on sharing the model.  With `transcriptions` (see read_transcriptions;
    together with a path, or with None for the model that scores nothing) a word is found by its sequence of labels instead
    of their spelling, homophones included (e2e_lm_load_transcriptions); entries whose word the ARPA file does not list
    are dropped, with one warning that counts them."""

    def __init__(self, path, labels, case_sensitive, words=None, lexicon=False, transcriptions=None, blank_idx=None):
        self.path, self.labels, self.case_sensitive = path, list(labels), bool(case_sensitive)
        self.words = None if words is None else list(words)
        if transcriptions is not None and words is not None:
            raise ValueError("words and transcriptions exclude each other")
        self.transcriptions = None if transcriptions is None else read_transcriptions(transcriptions, self.labels, blank_idx)
        self._lexicon = bool(lexicon)
        self._per_device = {}
        self._first = self._load()
        if self.transcriptions is not None and self._first.transcriptions_dropped():
            warnings.warn("transcriptions: %d of %d entries dropped: the language model does not list their words"
                          % (self._first.transcriptions_dropped(), len(self.transcriptions)))

    def _load(self):
        if self.transcriptions is not None:
            flat, off = [], [0]
            for _, ids in self.transcriptions:
                flat += ids
                off.append(len(flat))
            lm = _C.LanguageModel.from_transcriptions(self.path or "", [w for w, _ in self.transcriptions], flat, off,
                                                      self.labels, self.case_sensitive)
        elif self.words is not None:
            lm = _C.LanguageModel.from_words(self.words, self.labels, self.case_sensitive)
        else:
            lm = _C.LanguageModel(self.path, self.labels, self.case_sensitive)
        if self._lexicon:
            lm.enable_lexicon()
        self._per_device[lm.device()] = lm
        return lm

    def enable_lexicon(self):
        """Build the lexicon on every copy loaded so far; copies loaded later carry it too.  Not while a decode that uses the
        model is in flight (the tables are replaced)."""
        for lm in self._per_device.values():
            lm.enable_lexicon()
        self._lexicon = True

    def has_lexicon(self):
        return self._first.has_lexicon()

    def spelling_class(self, spelling):
        """bit 0: a word of the lexicon; bit 1: a proper prefix of a longer word (0 without a lexicon)."""
        return self._first.spelling_class(spelling)

    def on(self, device):
        lm = self._per_device.get(device.index)
        if lm is None:
            with torch.cuda.device(device):
                lm = self._load()
            if lm.device() != device.index:
                raise R.E2EError("the language model could not be loaded on %s" % device)
        return lm

    def order(self):
        return self._first.order()

    def word_index(self, word):
        return self._first.word_index(word)

    def score(self, ctx, word):
        return self._first.score(list(ctx), word)

    def is_transcribed(self):
        return self._first.is_transcribed()

    def transcriptions_dropped(self):
        return self._first.transcriptions_dropped()

    def transcribe(self, ids, space_id):
        """The words of a label sequence as a search over this model reads them (e2e_lm_transcribe): split at the space,
        homophones chosen by the model in the running context; a piece that is no word is '<unk>'."""
        f = self._first
        return [f.word_string(w) if w else "<unk>" for w in f.transcribe([int(k) for k in ids], int(space_id))]


class CTCDecoderEngine:
    """Same constructor arguments and defaults as the pybind class
    (src/decoders/ctc_decoder_py.cpp:8-24); methods keep the reference's keyword names.  The constructor is the reference's;
    what goes beyond it is set with `configure()` before the first decode."""

    def __init__(self, blank_idx, beam_width_=100, labels=None, lm_path="", lmwt_=1.0, wip_=0.0,
                 oov_penalty_=-1000.0, case_sensitive=False, keep_on_device=False):
        self.blank_idx = int(blank_idx)
        self.beam_width = int(beam_width_)
        self.labels = list(labels or [])
        self.lmwt = self._lmwt_given = float(lmwt_)
        self.wip = float(wip_)
        self.oov_penalty = float(oov_penalty_)
        self.case_sensitive = bool(case_sensitive)
        self.keep_on_device = bool(keep_on_device)
        # index of " " among the labels, else -1 (src/decoders/ctc_decoder.cpp:55-59)
        self.space_id = self.labels.index(" ") if " " in self.labels else -1
        # (a lone surrogate is a legal one-character label, but not legal UTF-32: such alphabets take the per-id join)
        self._codes = (np.array([ord(c) for c in self.labels], dtype="<u4")
                       if self.labels and all(len(c) == 1 and not 0xD800 <= ord(c) <= 0xDFFF for c in self.labels) else None)
        self.lm = None
        self.restrict = False
        self.cutoff_top_n, self.cutoff_prob = None, 1.0          # per-frame label pruning (configure): off
        self._check_width(bool(lm_path))
        if lm_path:
            R.require_gpu()
            self.lm = LanguageModel(lm_path, self.labels, self.case_sensitive)
        else:
            self.lmwt = 0.0   # ctc_decoder.cpp:72-74

    def _check_width(self, with_lm):
        if self.labels and self.beam_width > 1:
            # the beam lives in one workgroup's LDS: a width / alphabet it cannot hold is reported now, not at the first
            # decode (upstream has no such limit, ctc_decoder.cpp:353-441; see include/e2e_ctc.h)
            # (a pruned search always takes the general kernel: its limit)
            cap = (_C.ctc_beam_cut_max_width if self._cut(len(self.labels)) else _C.ctc_beam_max_width)(len(self.labels), with_lm)
            if self.beam_width > cap:
                raise ValueError("beam_width %d is not supported for an alphabet of %d labels%s: at most %d"
                                 % (self.beam_width, len(self.labels), " with a language model" if with_lm else "", cap))

    def _cut(self, V):
        """(cutoff_top_n, cutoff_prob) as the C calls take them if the decoder prunes an alphabet of V labels, else None."""
        top_n = V if self.cutoff_top_n is None else self.cutoff_top_n
        return (top_n, self.cutoff_prob) if top_n < V or self.cutoff_prob < 1.0 else None

    def _set_cut(self, cutoff_top_n, cutoff_prob):
        if cutoff_top_n is not None and int(cutoff_top_n) < 1:
            raise ValueError("cutoff_top_n=%r: at least 1" % (cutoff_top_n,))
        if not 0.0 < float(cutoff_prob) <= 1.0:
            raise ValueError("cutoff_prob=%r outside (0, 1]" % (cutoff_prob,))
        if (cutoff_top_n is not None or float(cutoff_prob) < 1.0) and self.beam_width == 1:
            raise ValueError("cutoff_top_n / cutoff_prob need beam_width > 1: greedy decoding expands nothing")
        top_n = None if cutoff_top_n is None else int(cutoff_top_n)
        if self.labels:
            self.check_cut_limit(len(self.labels), top_n, float(cutoff_prob))
        self.cutoff_top_n, self.cutoff_prob = top_n, float(cutoff_prob)

    @staticmethod
    def check_cut_limit(V, cutoff_top_n, cutoff_prob):
        """A pruned frame keeps at most e2e_ctc_label_cut_max() labels besides the blank."""
        K = V if cutoff_top_n is None else min(cutoff_top_n, V)
        if (K < V or cutoff_prob < 1.0) and K > _C.ctc_label_cut_max():
            raise ValueError("min(cutoff_top_n, alphabet) = %d: a pruned frame keeps at most %d labels (set cutoff_top_n)"
                             % (K, _C.ctc_label_cut_max()))

    def configure(self, restrict_to_vocabulary=False, lexicon=None, lm=None, transcriptions=None, lm_path=None,
                  cutoff_top_n=None, cutoff_prob=1.0):
        """Extensions, set once before decoding; returns self.
        `cutoff_top_n`, `cutoff_prob`: per-frame label pruning (the definition: e2e_ctc_label_cut, include/e2e_ctc.h) -- a frame
        expands at most `cutoff_top_n` labels and of those the fewest whose probabilities sum to `cutoff_prob`, the blank always.
        None / 1.0 (or a `cutoff_top_n` that is no less than the alphabet): not pruned.  A pruned search runs the general kernel.
        `restrict_to_vocabulary`: the beam search only forms words of the language model's vocabulary.
        `lexicon`: an iterable of words; the search is restricted to them without a language model -- a model that scores
        nothing is built from the list, `lmwt` and `oov_penalty` then count as 0 (as `lmwt` does upstream without a model),
        `wip` applies, and the width limit is the one with a language model.
        `lm`: a LanguageModel loaded already, for a decoder constructed without `lm_path`: decoders, restricted or not, may
        share one instead of loading the file each.
        `transcriptions`: a transcription lexicon (read_transcriptions): words are found by their label sequences, homophones
        chosen by the language model; `sentences` are then the words.  With the constructor's `lm_path` or the `lm_path` given
        here the model scores them; alone it is the model that scores nothing (every listed word at log10 p = 0)."""
        if lm_path is not None and transcriptions is None:
            raise ValueError("lm_path is the constructor's; configure takes it only together with transcriptions")
        self._set_cut(cutoff_top_n, cutoff_prob)
        if transcriptions is not None:
            if lexicon is not None or lm is not None:
                raise ValueError("transcriptions exclude lexicon and lm (restrict_to_vocabulary=True restricts to the transcriptions)")
            if self.beam_width == 1:
                raise ValueError("transcriptions need beam_width > 1: greedy decoding forms no words")
            path = lm_path or (self.lm.path if self.lm is not None else None)
            self.lm = None
            lm = LanguageModel(path, self.labels, self.case_sensitive, transcriptions=transcriptions, blank_idx=self.blank_idx)
        restrict = bool(restrict_to_vocabulary) or lexicon is not None
        if sum(1 for m in (self.lm is not None, lexicon is not None, lm is not None) if m) > 1:
            raise ValueError("lm_path, lexicon and lm exclude each other (a lexicon together with a language model is not supported)")
        if restrict and self.lm is None and lexicon is None and lm is None:
            raise ValueError("restrict_to_vocabulary needs a vocabulary: lm_path or lexicon")
        if restrict and self.beam_width == 1:
            raise ValueError("restrict_to_vocabulary needs beam_width > 1: greedy decoding has no vocabulary")
        if lm is not None:
            if lm.labels != self.labels or lm.case_sensitive != self.case_sensitive:
                raise ValueError("the shared language model was loaded with other labels or another case_sensitive")
            self._check_width(True)
            self.lm = lm
            self.lmwt = self._lmwt_given
        elif lexicon is not None:
            self._check_width(True)
            R.require_gpu()
            self.lm = LanguageModel(None, self.labels, self.case_sensitive, words=_lexicon_words(lexicon), lexicon=True)
            self.lmwt = 0.0
            self.oov_penalty = 0.0
        if restrict and not self.lm.has_lexicon():
            self.lm.enable_lexicon()
        self.restrict = restrict
        self._check_width(self.lm is not None)
        return self

    def _strings(self, rows, lens):
        # indices2str, ctc_decoder.cpp:203-220: "" when there are no labels.  The empty prefix wins as [-1] (quirk Q6);
        # the reference then reads labels[-1] out of bounds (undefined behaviour) -- here that id spells nothing.
        if not self.labels:
            return ["" for _ in lens]
        if self.lm is not None and self.lm.is_transcribed():
            # a transcription model: the words the search chose, not the labels' strings
            if isinstance(rows, torch.Tensor):
                rows = rows.tolist()
            return [" ".join(self.lm.transcribe([k for k in row[:n] if k >= 0], self.space_id)) for row, n in zip(rows, lens)]
        if self._codes is not None and len(lens) and isinstance(rows, torch.Tensor):
            # one-character labels (the usual alphabet): one table lookup and one decode for the whole batch instead of a
            # Python-level join per id (4 ms of a 17 ms beam-search call at B=64, T=1500)
            ids = rows.numpy()
            if ids.size == 0 or int(ids.min()) >= 0:
                width = ids.shape[1]
                text = self._codes[ids].tobytes().decode("utf-32-le")
                return [text[b * width: b * width + n] for b, n in enumerate(lens)]
            rows = ids.tolist()
        elif isinstance(rows, torch.Tensor):
            rows = rows.tolist()
        return ["".join(self.labels[k] for k in row[:n] if k >= 0) for row, n in zip(rows, lens)]

    def _prep(self, logits_, logits_lengths_, native16=True):
        if logits_.dim() != 3:
            raise ValueError("logits must be (batch, time, alphabet)")
        dev = R.compute_device(logits_)
        x = logits_.detach()
        # (16-bit inputs: the greedy kernels compare them as they are, the beam search reads them as they are -- each is an f32
        #  number, so the search is the f32 one's; upstream converts whatever arrives once, ctc_decoder.cpp:157-160)
        if x.dtype not in ((torch.float32, torch.float64, torch.float16, torch.bfloat16) if native16 else (torch.float32, torch.float64)):
            x = x.to(torch.float32)
        x = x.to(dev)
        xl = _as_long(logits_lengths_, dev)
        if xl.numel() != x.shape[0]:
            raise ValueError("logits_lengths_ must have one entry per utterance")
        V = x.shape[2]
        if not 0 <= self.blank_idx < V:
            raise ValueError("blank_idx %d outside the alphabet of %d columns" % (self.blank_idx, V))
        if self.labels and len(self.labels) != V:
            # upstream indexes labels[id] unchecked (ctc_decoder.cpp:203-220); a mismatch would spell garbage
            raise ValueError("the decoder has %d labels but the logits have %d columns" % (len(self.labels), V))
        return x, xl, dev

    def _result(self, t):
        return t if self.keep_on_device else t.cpu()

    def decode_greedy(self, logits_, logits_lengths_):
        """argmax + blank/repeat collapse -> (targets (B,Tmax) int64 zero padded, lengths (B), sentences)."""
        x, xl, dev = self._prep(logits_, logits_lengths_)
        B, T, V = x.shape
        out = torch.empty((B, T), dtype=torch.long, device=dev)
        out_len = torch.empty(B, dtype=torch.long, device=dev)
        if B:
            with torch.cuda.device(dev):
                sB, sT, sV = x.stride()
                _C.ctc_greedy(x.data_ptr(), R.dtype_code(x.dtype), sB, sT, sV, xl.data_ptr(), B, T, V,
                              self.blank_idx, out.data_ptr(), out_len.data_ptr(), R.stream_handle(dev))
        out, out_len = self._result(out), self._result(out_len)
        sentences = self._strings(out.cpu(), out_len.tolist()) if self.labels else ["" for _ in range(B)]
        return out, out_len, sentences

    def decode(self, logits_, logits_lengths_):
        """Prefix beam search on LOG-PROBABILITIES -> (indices (B,maxlen) int64, lengths (B), sentences)."""
        if self.restrict or self._cut(logits_.shape[-1]):
            # hypothesis 0 of the restricted / pruned n-best list (options of that call: e2e_ctc_beam_nbest_opt, _cut)
            return _first_hypothesis(self.decode_nbest(logits_, logits_lengths_, nbest=1))
        x, xl, dev = self._prep(logits_, logits_lengths_)
        B, T, V = x.shape
        max_out = T + 1
        out = torch.empty((B, max_out), dtype=torch.long, device=dev)
        out_len = torch.empty(B, dtype=torch.long, device=dev)
        if B:
            with torch.cuda.device(dev):
                nbytes = _C.ctc_beam_workspace_bytes_lm(B, T, V, self.beam_width, self.lm is not None)
                ws = R.workspace(dev, nbytes)
                _C.ctc_beam(*self._search_args(x, xl), out.data_ptr(), max_out, out_len.data_ptr(),
                            ws.data_ptr(), ws.numel(), R.stream_handle(dev))
        lens = out_len.tolist()
        # per-utterance status rides on the lengths (include/e2e_ctc.h): no extra call, no extra synchronisation
        for b, n in enumerate(lens):
            if n < 0 or n > max_out:
                raise R.E2EError("beam search: utterance %d %s" % (
                    b, "ran out of prefix-tree nodes" if n < 0 else "needs %d output ids, %d provided" % (n, max_out)))
        width = max(lens) if lens else 0
        ids = out[:, :width].contiguous()    # packed to the longest result (ctc_decoder.cpp:192-200)
        ids, out_len = self._result(ids), self._result(out_len)
        return ids, out_len, self._strings(ids.cpu(), lens)

    def decode_nbest(self, logits_, logits_lengths_, nbest=None, timesteps=False):
        """The same search read out as an n-best list, on LOG-PROBABILITIES (e2e_ctc_beam_nbest, include/e2e_ctc.h) ->
        (indices (B,N,maxlen) int64, lengths (B,N), sentences [B][n_hyp], scores (B,N) f64, ctc_scores, lm_scores,
        num_words (B,N) int32, num_oov (B,N), num_hypotheses (B), timesteps (B,N,maxlen) int64 or None).  Hypotheses are
        ranked by total score, hypothesis 0 is decode()'s result; slots beyond num_hypotheses[b] are empty (length 0, -inf)."""
        N = self.beam_width if nbest is None else int(nbest)
        if not 1 <= N <= self.beam_width:
            raise ValueError("nbest=%d outside [1, beam_width=%d]" % (N, self.beam_width))
        x, xl, dev = self._prep(logits_, logits_lengths_)
        B, T, V = x.shape
        max_out = T + 1
        bufs = out, out_len, n_hyp, scores, counts, ts = _nbest_buffers(B, N, max_out, dev, timesteps=timesteps)
        if B:
            with torch.cuda.device(dev):
                nbytes, entry, cut = self._entry(B, T, V, timesteps=timesteps)
                ws = R.workspace(dev, nbytes)
                entry(*self._search_args(x, xl), N,
                      out.data_ptr(), max_out, out_len.data_ptr(), n_hyp.data_ptr(), scores.data_ptr(),
                      counts.data_ptr(), ts.data_ptr() if timesteps else 0,
                      ws.data_ptr(), ws.numel(), R.stream_handle(dev), self.restrict, *cut)
        return _nbest_result(self, *bufs)

    def _search_args(self, x, xl):
        """What the arguments of every beam-search entry begin with: the input (pointer, dtype code, strides, lengths), the
        sizes and the blank, the width, the space and the model's handle on x's device, the three weights."""
        B, T, V = x.shape
        sB, sT, sV = x.stride()
        lm = self.lm.on(x.device).handle if self.lm is not None else 0
        return (x.data_ptr(), R.dtype_code(x.dtype), sB, sT, sV, xl.data_ptr(), B, T, V, self.blank_idx,
                self.beam_width, self.space_id, lm, self.lmwt, self.wip, self.oov_penalty)

    def _entry(self, B, T, V, stream=False, timesteps=False):
        """(workspace bytes, the n-best entry to call, the arguments it takes behind the unpruned entry's) of a whole call on
        T frames, or of a stream's chunk of T: pruned or not is decided here, and with it which query sizes the workspace."""
        W, with_lm, cut = self.beam_width, self.lm is not None, self._cut(V)
        if not cut:
            if stream:
                return _C.ctc_beam_stream_workspace_bytes(B, V, W, with_lm), _C.ctc_beam_stream, ()
            return _C.ctc_beam_nbest_workspace_bytes(B, T, V, W, with_lm, bool(timesteps)), _C.ctc_beam_nbest, ()
        self.check_cut_limit(V, *cut)
        if stream:
            return _C.ctc_beam_cut_stream_workspace_bytes(B, T, V, W, with_lm, cut[0]), _C.ctc_beam_stream_cut, cut
        return _C.ctc_beam_cut_workspace_bytes(B, T, V, W, with_lm, bool(timesteps), cut[0]), _C.ctc_beam_nbest_cut, cut

    def _check_nbest(self, nh, lens, max_out):
        """Per-utterance and per-hypothesis status ride on the counts and lengths, as in decode()."""
        for b, n in enumerate(nh):
            if n < 0:
                raise R.E2EError("beam search: utterance %d ran out of prefix-tree nodes" % b)
            if max(lens[b]) > max_out:
                raise R.E2EError("beam search: utterance %d needs %d output ids, %d provided" % (b, max(lens[b]), max_out))

    def open_stream(self, batch_size, max_frames, device=None, timesteps=False):
        """Streaming beam search (e2e_ctc_beam_stream, include/e2e_ctc.h): a CTCBeamStream that is fed log-probabilities in
        chunks and keeps the beams of `batch_size` utterances of up to `max_frames` frames on the GPU between the chunks.
        After every chunk the result is, bit for bit, that of decode / decode_nbest on all the frames fed so far."""
        return CTCBeamStream(self, batch_size, max_frames, device=device, timesteps=timesteps)

    def print_scores_for_sentence(self, words):
        """src/decoders/ctc_decoder.cpp:141-151: word, decoder index, vocabulary index, log10 score."""
        if self.lm is None:
            return
        ctx = [self.lm.word_index("<s>")]
        order = self.lm.order()
        for w in words:
            key = w if self.case_sensitive else w.lower()
            idx = self.lm.word_index(key)
            print(w, idx, self.lm.word_index(w), self.lm.score(ctx, idx))
            ctx = ([idx] + ctx)[: max(order - 1, 0)]


class CTCBeamStream(_BeamStream):
    """The CTC beams of `batch_size` utterances, kept on the GPU between chunks (CTCDecoderEngine.open_stream): _BeamStream,
    fed log-probabilities."""

    _STATUS = {-1: "ran out of prefix-tree nodes"}

    def __init__(self, engine, batch_size, max_frames, device=None, timesteps=False):
        if engine.beam_width < 2:
            raise ValueError("a stream needs beam_width > 1: greedy decoding has no beam to keep")
        super().__init__(engine, batch_size, max_frames, device=device, timesteps=timesteps)

    def _row_bytes(self, V):
        e = self.engine
        return _C.ctc_beam_stream_row_bytes(self.max_frames, V, e.beam_width, e.lm is not None, self.timesteps)

    def _prepare(self, logits_, logits_lengths_):
        return self.engine._prep(logits_, logits_lengths_)

    def _max_out(self, frames):
        return frames + 1

    def _launch(self, x, xl, state, N, max_out, bufs, frames_done, stream):
        e, dev = self.engine, x.device
        B, Tc, V = x.shape
        out, out_len, n_hyp, scores, counts, ts = bufs
        # (pruned or not: the engine's knobs, the same for every chunk, as the restriction is)
        nbytes, entry, cut = e._entry(B, Tc, V, stream=True)
        ws = R.workspace(dev, nbytes, stream) if nbytes else None     # (the one-workgroup kernel needs none: a null pointer)
        entry(*e._search_args(x, xl), state.data_ptr(), self.row_bytes, self.max_frames, self.timesteps, N,
              out, max_out, out_len, n_hyp, scores, counts, ts, frames_done,
              ws.data_ptr() if nbytes else 0, ws.numel() if nbytes else 0, stream, e.restrict, *cut)


class GramBeamStream(_BeamStream):
    """The Gram-CTC beams of `batch_size` utterances, kept on the GPU between chunks (GramCTCDecoderEngine.open_stream):
    _BeamStream, fed log-probabilities.  The engine's configuration (configure(), restrict()) at the time the stream was
    opened is the stream's: an engine that was never configured streams the search on the masses (e2e_gram_ctc_beam_stream with
    scored = 0), a configured one the search on the totals."""

    _PREFILL = "ts"
    _NEEDS_CONFIGURE = ("timesteps are part of the configured search's results: call configure() first "
                        "(configure(wip=0) is the search without a model and without penalties)")

    def __init__(self, engine, batch_size, max_frames, device=None, timesteps=False):
        if engine.beam_width < 2:
            raise ValueError("a stream needs beam_width > 1: greedy decoding has no beam to keep")
        super().__init__(engine, batch_size, max_frames, device=device, timesteps=timesteps)
        e = engine
        if self.timesteps and not e.configured:
            raise ValueError(self._NEEDS_CONFIGURE)
        self.scored = self._scored = bool(e.configured)
        self.lm = e.lm if self.scored else None
        self.restricted = bool(e.restricted) if self.scored else False
        self._knobs = (e.space_id, e.lmwt, e.wip, e.oov_penalty) if self.scored else (-1, 0.0, 0.0, 0.0)
        self._cut = e._cut()                                     # the pruning in force now: the same for every chunk

    def feed_nbest(self, logits_, logits_lengths_=None, nbest=None, timesteps=None):
        """_BeamStream.feed_nbest; timesteps: None -- as the stream was opened -- or whether this read-out returns them (a
        configured search only; they cost the stream nothing: the nodes' numbers carry them)."""
        want_ts = self.timesteps if timesteps is None else bool(timesteps)
        if want_ts and not self.scored:
            raise ValueError(self._NEEDS_CONFIGURE)
        return self._feed_nbest(logits_, logits_lengths_, nbest, want_ts)

    def _row_bytes(self, V):
        e = self.engine
        if self._cut:
            return _GramCut.query("stream_row_bytes", self.max_frames, V, e.max_order, e.beam_width, self.scored,
                                                     self.lm is not None, self._cut[0])
        return _C.gram_beam_stream_row_bytes(self.max_frames, V, e.max_order, e.beam_width, self.scored, self.lm is not None)

    def _prepare(self, logits_, logits_lengths_):
        return self.engine._prep(logits_, logits_lengths_, _F32_F64)

    def _max_out(self, frames):
        return max(frames * self.engine.max_order, 1)

    def _launch(self, x, xl, state, N, max_out, bufs, frames_done, stream):
        e, dev = self.engine, x.device
        B, Tc, V = x.shape
        out, out_len, n_hyp, scores, counts, ts = bufs
        space_id, lmwt, wip, oov_penalty = self._knobs
        ids, lens = e._table(dev)
        lm = self.lm.on(dev).handle if self.lm is not None else 0
        cut = self._cut
        if cut:
            nbytes = _GramCut.query("stream_workspace_bytes", B, Tc, V, e.max_order, e.beam_width, self.scored,
                                                             self.lm is not None, cut[0])
        else:
            nbytes = _C.gram_beam_stream_workspace_bytes(B, V, e.max_order, e.beam_width, self.scored, self.lm is not None)
        ws = R.workspace(dev, nbytes, stream)
        sB, sT, sV = x.stride()
        args = (x.data_ptr(), R.dtype_code(x.dtype), sB, sT, sV, xl.data_ptr(), B, Tc, V,
                ids.data_ptr(), lens.data_ptr(), e.max_order, e.num_base_labels, e.beam_width,
                self.scored, space_id, lm, lmwt, wip, oov_penalty,
                state.data_ptr(), self.row_bytes, self.max_frames, N,
                out, max_out, out_len, n_hyp, scores, counts, frames_done,
                ws.data_ptr(), ws.numel(), stream, (self.restricted, ts) if self.scored else None)
        if cut:
            _GramCut.call("e2e_gram_ctc_beam_stream_cut", *args, *cut)
        else:
            _C.gram_ctc_beam_stream(*args)
