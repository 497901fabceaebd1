"""CTCLossSegmented with the reference's constructor and call signature
(pytorch_end2end/modules/ctc_loss_segmented.py:12-146), computed on the MI355X.

    loss = CTCLossSegmented(space_idx=sp)(logits, targets, logits_lengths, targets_lengths)     # (batch,) losses

The batch is force-aligned; the words the model's per-frame arg-max already reproduces frame for frame are found; every
utterance is cut at the spaces around them; each piece is trained with its own CTC loss, so that a well-learned word stops
leaking probability mass across its boundaries.  The loss of an utterance is the sum of its pieces' losses, the gradient
each piece's softmax - posterior on the piece's own frames (definition: include/e2e_ctc.h).

A call is: log-softmax (plumbing), e2e_ctc_align, e2e_ctc_wordseg_plan, ONE read-back of the plan's summary and segment
lengths -- the call's only synchronisation; upstream lives on the host throughout --, then per group of segments
e2e_ctc_wordseg_gather + e2e_ctc_loss_fwd_bwd + e2e_ctc_wordseg_finish.  The frames never leave the GPU.  Segments are
sorted by length and cut into consecutive groups so that no gathered buffer is larger than the input itself (upstream
allocates segments x T x V).  When no utterance is cut the result is CTCLoss's on the original tensors, bit for bit.

Deliberate differences from upstream:
  * upstream counts the segments before it builds them; the two disagree when a qualifying space sits on the last frame
    and when the first boundary is frame 1, and upstream then raises AssertionError / IndexError.  Here the built list is
    the definition and nothing raises;
  * `blank_idx` is used for the alignment, the plan and the loss alike (upstream hard-codes blank 0 in the first and the
    last; at blank_idx=0 the two are identical);
  * the result has the logits' dtype and device (16-bit and other dtypes are computed in f32);
  * `reduce` is accepted and ignored, as upstream: the result is always the (batch,) vector.
"""
import numpy as np
import torch
import torch.nn as nn
from torch.autograd import Function

from .. import _runtime as R
from .._runtime import _C
from ..engines import CTCLossEngine
from ..utils import segmentation as S


class _SegmentedLossFunction(Function):
    """One Function for the whole loss: keeps the assembled (B,T,V) gradient, multiplies it by grad_output[b] in place
    (e2e_ctc_scale_grads) and, like ForwardBackwardLossFunction, computes it again when a retained graph is walked twice."""

    @staticmethod
    def forward(ctx, module, logits, targets, logits_lengths, targets_lengths):
        args = (logits.detach(), targets, logits_lengths, targets_lengths)
        loss, grads = module.compute(*args)
        ctx.module, ctx.args, ctx.grads = module, args, grads
        return loss

    @staticmethod
    def backward(ctx, grad_output):
        grads = ctx.grads
        if grads is None:          # a retained graph walked again: the first walk gave the buffer to autograd
            grads = ctx.module.compute(*ctx.args)[1]
        ctx.grads = None
        if grads.is_cuda and grads.is_contiguous() and grads.dtype in (torch.float32, torch.float64, torch.float16, torch.bfloat16):
            CTCLossEngine.scale_grads_(grads, grad_output)
        else:                      # results moved back to a CPU source tensor
            go = grad_output.contiguous().to(device=grads.device, dtype=grads.dtype)
            grads = grads * go.view(-1, 1, 1)
        if grads.device != grad_output.device:
            grads = grads.to(grad_output.device)
        return None, grads, None, None, None


class CTCLossSegmented(nn.Module):
    """
    Word-segmented CTC loss.

    :param space_idx: index of the space label: utterances are cut at well-recognised spaces
    :param blank_idx: index of the blank label
    :param reduce: accepted and ignored, as upstream: the result is the ``(batch,)`` vector
    :param min_word_length: a word counts as recognised only if it has at least this many labels
    """

    def __init__(self, space_idx, blank_idx=0, reduce=False, min_word_length=3):
        super().__init__()
        self.reduce = reduce
        self.space_idx = int(space_idx)
        self.blank_idx = int(blank_idx)
        self.min_word_length = int(min_word_length)
        self._engine = CTCLossEngine(self.blank_idx)
        self.last_plan = None      # diagnostics of the last call: segments per kind, the groups' (count, frames, labels)
        self._mark = None          # diagnostics: called with a phase's name when the phase has been issued

    def forward(self, logits, targets, logits_lengths, targets_lengths):
        """
        :param logits: float tensor ``(batch, time, alphabet)``, raw (the log-softmax is part of the loss)
        :param targets: ``(batch, max_target_length)`` integer tensor
        :param logits_lengths: ``(batch,)`` frame counts
        :param targets_lengths: ``(batch,)`` target lengths
        :return: ``(batch,)`` losses
        """
        S.check_shapes(logits, targets, logits_lengths, targets_lengths)
        S.check_indices(self.space_idx, self.blank_idx, logits.shape[2])
        return _SegmentedLossFunction.apply(self, logits, targets, logits_lengths, targets_lengths)

    def compute(self, logits, targets, logits_lengths, targets_lengths):
        """(losses (B,), d losses / d logits (B,T,V)) in the logits' dtype, on their device."""
        src_device, src_dtype = logits.device, logits.dtype
        if logits.dim() == 3 and logits.shape[0] == 0:
            return logits.new_zeros(0), torch.zeros_like(logits)
        plan = S.make_plan(logits, targets, logits_lengths, targets_lengths, self.space_idx, self.blank_idx,
                           self.min_word_length, mark=self._mark)
        summary, _, (length, tlen, kind) = S.read_plan(plan, fields=3)      # the call's one synchronisation
        mark = self._mark or (lambda name: None)
        mark("read-back")
        x, dev = plan.x, plan.dev
        B, T, V = x.shape
        self.last_plan = dict(summary, groups=[], max_buffer_elems=0)
        if summary["utterances_cut"] == 0:
            # nothing to cut: CTCLoss on the original tensors, no gather
            losses, grads = self._engine.compute(x, plan.targets[:, :plan.Smax], plan.xl, plan.tl, input_is_logprobs=False)
            mark("loss")
        else:
            losses, grads = self._segmented(plan, length, tlen, kind)
        if src_device != dev or src_dtype != losses.dtype:
            losses, grads = losses.to(src_device, src_dtype), grads.to(src_device, src_dtype)
        return losses, grads

    def _segmented(self, plan, length, tlen, kind):
        x, dev = plan.x, plan.dev
        B, T, V = x.shape
        code = R.dtype_code(x.dtype)
        sB, sT, sV = x.stride()
        tg = plan.targets
        mark = self._mark or (lambda name: None)
        sel = np.nonzero(kind != S.FRAME)[0]
        groups = S.plan_groups(length[sel], B * T)
        losses = torch.empty(B, dtype=x.dtype, device=dev)
        grads = torch.empty((B, T, V), dtype=x.dtype, device=dev)
        with torch.cuda.device(dev):
            stream = R.stream_handle(dev)
            order = np.concatenate(groups) if groups else np.zeros(0, dtype=np.int64)
            # (one small upload for all groups; the stream has nothing queued at this point)
            idx_all = torch.from_numpy(sel[order].astype(np.int32)).to(dev, non_blocking=True)
            done = 0
            for g in groups:
                members = sel[g]
                n, L, Sg = len(members), int(length[members].max()), max(int(tlen[members].max()), 1)
                idx = idx_all[done: done + n]
                done += n
                xg = torch.empty((n, L, V), dtype=x.dtype, device=dev)
                tgg = torch.empty((n, Sg), dtype=torch.long, device=dev)
                xlg = torch.empty(n, dtype=torch.long, device=dev)
                tlg = torch.empty(n, dtype=torch.long, device=dev)
                _C.ctc_wordseg_gather(x.data_ptr(), code, sB, sT, sV, tg.data_ptr(), tg.stride(0), plan.xl.data_ptr(),
                                      plan.tl.data_ptr(), B, T, V, plan.Smax, plan.table.data_ptr(), plan.pool.data_ptr(),
                                      idx.data_ptr(), n, L, Sg, xg.data_ptr(), tgg.data_ptr(), xlg.data_ptr(),
                                      tlg.data_ptr(), stream)
                mark("gather")
                gl, gg = self._engine.compute(xg, tgg, xlg, tlg, input_is_logprobs=False)
                mark("loss")
                _C.ctc_wordseg_finish(x.data_ptr(), code, sB, sT, sV, plan.align.data_ptr(), B, T, V,
                                      plan.table.data_ptr(), gg.data_ptr(), gl.data_ptr(), idx.data_ptr(), n, L, False,
                                      losses.data_ptr(), grads.data_ptr(), plan.ws.data_ptr(), plan.ws.numel(), stream)
                mark("finish")
                self.last_plan["groups"].append((n, L, Sg))
                self.last_plan["max_buffer_elems"] = max(self.last_plan["max_buffer_elems"], n * L * V)
            _C.ctc_wordseg_finish(x.data_ptr(), code, sB, sT, sV, plan.align.data_ptr(), B, T, V, plan.table.data_ptr(),
                                  0, 0, 0, 0, 1, True, losses.data_ptr(), grads.data_ptr(), plan.ws.data_ptr(),
                                  plan.ws.numel(), stream)
            mark("finish")
        return losses, grads
