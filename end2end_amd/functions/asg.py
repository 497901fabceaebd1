"""Autograd glue for ASG (e2e_asg_fwd_bwd): a Function with two differentiable inputs, the emissions and the transitions.

    losses = ASGLossFunction.apply(engine, emissions, transitions, targets, logits_lengths, targets_lengths)

As ForwardBackwardLossFunction, forward asks the engine for the loss and both gradients in one pass and keeps them as plain
attributes.  Backward scales the emission gradient in place by grad_output (e2e_ctc_scale_grads) and contracts the
per-utterance transition slabs with it, `einsum('b,bji->ji', grad_output, tgrads)`.  A retained graph walked a second time
finds the buffers given away and asks the engine again (same inputs, same result).
"""
import torch
from torch.autograd import Function


class ASGLossFunction(Function):
    @staticmethod
    def forward(ctx, engine, emissions, transitions, targets, logits_lengths, targets_lengths):
        args = (emissions.detach(), transitions.detach(), targets, logits_lengths, targets_lengths)
        losses, grads, tgrads = engine.compute(*args)
        ctx.engine, ctx.args = engine, args
        ctx.grads, ctx.tgrads = grads, tgrads          # plain attributes (no double backward)
        return losses

    @staticmethod
    def backward(ctx, grad_output):
        grads, tgrads = ctx.grads, ctx.tgrads
        if grads is None:          # a retained graph walked again: the first walk gave the buffers to autograd
            _, grads, tgrads = ctx.engine.compute(*ctx.args)
        ctx.grads = ctx.tgrads = None
        go = grad_output.contiguous().to(device=tgrads.device, dtype=tgrads.dtype)
        tg = torch.einsum("b,bji->ji", go, tgrads) if ctx.needs_input_grad[2] else None
        if not ctx.needs_input_grad[1]:
            grads = None
        elif grads.is_cuda and grads.is_contiguous() and grads.dtype in (torch.float32, torch.float64):
            ctx.engine.scale_grads_(grads, grad_output)
        else:                      # results moved back to a CPU source tensor, or a 16-bit one
            grads = grads * go.to(device=grads.device, dtype=grads.dtype).view(-1, 1, 1)
        if tg is not None:
            tg = tg.to(device=ctx.args[1].device, dtype=ctx.args[1].dtype)
        return None, grads, tg, None, None, None
