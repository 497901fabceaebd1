"""-m gpu: the compute() contract that the three loss engines share (end2end_amd/engines.py: one skeleton, three kernels
behind it): argument errors, the empty batch, devices, dtypes and the reduction.  B=2, T=20, V=5, S<=3: two blocks of the
blank-free lattice (one partial) and two checkpoints of the Gram-CTC one."""
import numpy as np
import pytest
import torch

import gpu_util as U
from end2end_amd.engines import CTCLossEngine, CTCWithoutBlankLossEngine, GramCTCLossEngine

pytestmark = pytest.mark.gpu

B, T, V, S = 2, 20, 5, 3
ENGINES = {
    "ctc": lambda: CTCLossEngine(0),
    "noblank": lambda: CTCWithoutBlankLossEngine(-1),
    "gram": lambda: GramCTCLossEngine(0, 4, V, {4: [1, 2]}),       # R=4 base labels, one bigram in column 4
}
_cache = {}


def _batch():
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, T, V, generator=g)
    tg = torch.randint(1, 4, (B, S), generator=g)                  # base labels 1..3: targets of all three losses
    return x, tg, torch.tensor([T, T - 3]), torch.tensor([S, S - 1])


def _plain(name):
    """(engine, batch on the CPU, (losses, grads) of compute() on GPU tensors), once per engine"""
    if name not in _cache:
        eng, (x, tg, xl, tl) = ENGINES[name](), _batch()
        out = eng.compute(x.to(U.dev()), tg.to(U.dev()), xl.to(U.dev()), tl.to(U.dev()), input_is_logprobs=False)
        _cache[name] = (eng, (x, tg, xl, tl), tuple(t.clone() for t in out))
    return _cache[name]


@pytest.mark.parametrize("name", list(ENGINES))
def test_argument_errors_and_their_messages(name):
    eng, (x, tg, xl, tl), _ = _plain(name)
    x = x.to(U.dev())
    with pytest.raises(ValueError, match=r"^logits must be \(batch, time, alphabet\)$"):
        eng.compute(x[0], tg, xl, tl)
    with pytest.raises(ValueError, match=r"^targets must be \(batch, max_target_length\)$"):
        eng.compute(x, torch.cat([tg, tg]), xl, tl)
    with pytest.raises(ValueError, match=r"^lengths must have one entry per utterance$"):
        eng.compute(x, tg, torch.cat([xl, xl[:1]]), tl)
    with pytest.raises(ValueError, match=r"^reduction must be None, 'sum' or 'mean'$"):
        eng.compute(x, tg, xl, tl, reduction="max")


@pytest.mark.parametrize("device", ["cuda", "cpu"])
@pytest.mark.parametrize("name", list(ENGINES))
def test_empty_batch(name, device):
    eng = _plain(name)[0]
    x = torch.empty((0, T, V), device=device)
    tg, n = torch.empty((0, S), dtype=torch.long), torch.empty(0, dtype=torch.long)
    losses, grads = eng.compute(x, tg, n, n)
    for t, shape in ((losses, (0,)), (grads, (0, T, V))):
        assert t.shape == shape and t.dtype == torch.float32 and t.device == x.device
    for reduction in ("sum", "mean"):
        losses, grads, reduced = eng.compute(x, tg, n, n, reduction=reduction)
        assert losses.shape == (0,) and grads.shape == (0, T, V)
        assert reduced.dim() == 0 and reduced.dtype == torch.float32 and reduced.device == x.device
        # the sum of no losses is 0 and their mean NaN (torch's, 0 / 0): what every engine returned before they shared this code
        assert reduced.item() == 0.0 if reduction == "sum" else np.isnan(reduced.item())


@pytest.mark.parametrize("name", list(ENGINES))
def test_cpu_tensors_in_give_cpu_tensors_out(name):
    eng, (x, tg, xl, tl), (l_gpu, g_gpu) = _plain(name)
    losses, grads = eng.compute(x, tg, xl, tl, input_is_logprobs=False)
    assert losses.device.type == "cpu" and grads.device.type == "cpu"
    assert losses.dtype == torch.float32 and grads.dtype == torch.float32
    assert torch.equal(losses, l_gpu.cpu()) and torch.equal(grads, g_gpu.cpu())


@pytest.mark.parametrize("name", list(ENGINES))
def test_f16_in_gives_f16_out_equal_to_the_f32_upcast(name):
    """The lattice engines up-cast: bit for bit the f32 call's results, rounded.  CTCLossEngine reads f16 natively (other
    kernels than the up-cast call runs): 4 eps relative and absolute, eps = 2^-10, the 16-bit tolerance of
    tests/test_gpu_module.py (the source dtype's rounding, twice)."""
    eng, (x, tg, xl, tl), _ = _plain(name)
    x16 = x.to(torch.float16).to(U.dev())
    l16, g16 = eng.compute(x16, tg, xl, tl, input_is_logprobs=False)
    l32, g32 = eng.compute(x16.float(), tg, xl, tl, input_is_logprobs=False)
    assert l16.dtype == torch.float16 and g16.dtype == torch.float16 and l16.is_cuda and g16.is_cuda
    assert l32.dtype == torch.float32 and g32.dtype == torch.float32
    if name == "ctc":
        eps = 2.0 ** -10
        U.assert_same(l16.float().cpu().numpy(), l32.to(torch.float16).float().cpu().numpy(), 4 * eps, 4 * eps, "losses")
        U.assert_same(g16.float().cpu().numpy(), g32.to(torch.float16).float().cpu().numpy(), 4 * eps, 4 * eps, "grads")
    else:
        assert torch.equal(l16, l32.to(torch.float16)) and torch.equal(g16, g32.to(torch.float16))


@pytest.mark.parametrize("name", list(ENGINES))
def test_sum_reduction_leaves_losses_and_grads_alone(name):
    """A reduction scales nothing in the engine (grad_scale does): the same losses and grads, and their sum, accumulated
    in f64 and rounded once to the loss dtype (1 ulp of f32 allowed: 2^-23 relative)."""
    eng, (x, tg, xl, tl), (l_none, g_none) = _plain(name)
    d = U.dev()
    losses, grads, reduced = eng.compute(x.to(d), tg.to(d), xl.to(d), tl.to(d), input_is_logprobs=False, reduction="sum")
    assert torch.equal(losses, l_none) and torch.equal(grads, g_none)
    assert reduced.dim() == 0 and reduced.dtype == torch.float32 and reduced.is_cuda
    want = l_none.double().sum().item()
    assert np.isfinite(want) and abs(reduced.item() - want) <= 2.0 ** -23 * abs(want)
