"""GPU: CTC without blank (e2e_ctc_noblank_fwd_bwd) and AlignedTargetsLoss against the reference's fixtures
(tests/golden/noblank.npz, made by tests/golden/make_noblank_golden.py) and against the test-side f64 restatement
(tests/noblank_ref.py) at shapes the reference is too slow for."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import noblank_ref as NR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = np.load(os.path.join(ROOT, "tests", "golden", "noblank.npz"))
CASES = sorted({k.split("/")[0] for k in FIX.files if not k.startswith("aligned")})
ALIGNED = sorted({k.split("/")[0] for k in FIX.files if k.startswith("aligned")})
DEV = torch.device("cuda", 0)


def case(name):
    return {k.split("/", 1)[1]: FIX[k] for k in FIX.files if k.split("/")[0] == name}


def tol(c):
    return 1e-9 if c["logits"].dtype == np.float64 else 1e-5


def check_losses(got, want, rel):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.array_equal(np.isinf(got), np.isinf(want)) and np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    fin = np.isfinite(want)
    assert np.all(np.abs(got[fin] - want[fin]) <= rel * np.maximum(1.0, np.abs(want[fin]))), (got, want)


def check_grads(got, want, atol):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.max(np.abs(got[ok] - want[ok]), initial=0.0) <= atol, np.max(np.abs(got[ok] - want[ok]))


def run_module(c, fused=True, device=DEV):
    from end2end_amd import CTCWithoutBlankLoss
    x = torch.from_numpy(c["logits"]).to(device).requires_grad_()
    tg, xl, tl = (torch.from_numpy(c[k]).to(device) for k in ("targets", "x_len", "t_len"))
    mod = CTCWithoutBlankLoss(reduce=bool(c["reduce"]), after_softmax=bool(c["after_softmax"]),
                              space_idx=int(c["space_idx"]), fused=fused)
    loss = mod(x, tg, xl, tl)
    (loss.sum() if c["reduce"] else (loss * torch.from_numpy(c["w"]).to(device)).sum()).backward()
    return loss.detach().cpu().numpy(), x.grad.cpu().numpy()


def module_want(c):
    """Expected module outputs in f64 from the engine-level fixture (the module-level ones are float32-rounded upstream)."""
    w = np.ones_like(c["w"]) if c["reduce"] else c["w"]
    g = c["eng_grad"] * w[:, None, None]
    if c["after_softmax"]:
        g = g / c["logits"].astype(np.float64)          # torch.log's backward
    loss = c["eng_loss"].sum() if c["reduce"] else c["eng_loss"]
    return loss, g


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name", CASES)
def test_module_matches_reference_fixtures(name, fused):
    c = case(name)
    loss, grad = run_module(c, fused)
    want_l, want_g = module_want(c)
    check_losses(np.atleast_1d(loss), np.atleast_1d(want_l), tol(c))
    check_grads(grad, want_g, tol(c))
    if c["logits"].dtype == np.float32:      # and the float32 values upstream's module itself returned
        check_losses(np.atleast_1d(loss), np.atleast_1d(c["loss"]), 1e-5)
        check_grads(grad, c["grad"], 1e-5)


def abi_call(lp, targets, x_len, t_len, space_idx, input_is_logprobs=True, grad_scale=1.0):
    from end2end_amd import _lib
    L = _lib.load()
    B, T, V = lp.shape
    code = _lib.dtype_code(lp.dtype)
    Smax = targets.shape[1]
    losses = torch.empty(B, dtype=lp.dtype, device=DEV)
    grads = torch.empty((B, T, V), dtype=lp.dtype, device=DEV)
    ws = torch.empty(L.e2e_ctc_noblank_workspace_bytes(B, T, V, Smax, code), dtype=torch.uint8, device=DEV)
    opts = _lib.LossOpts(grad_scale, None, 0, 0)
    _lib.check(L.e2e_ctc_noblank_fwd_bwd(lp.data_ptr(), code, int(input_is_logprobs), *lp.stride(), targets.data_ptr(),
                                         targets.stride(0), x_len.data_ptr(), t_len.data_ptr(), B, T, V, Smax, space_idx,
                                         losses.data_ptr(), grads.data_ptr(), ws.data_ptr(), ws.numel(),
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(opts)))
    torch.cuda.synchronize()
    return losses.cpu().numpy(), grads.cpu().numpy()


@pytest.mark.parametrize("name", CASES)
def test_c_abi_matches_reference_fixtures(name):
    c = case(name)
    x = torch.from_numpy(c["logits"])
    lp = (torch.log(x) if c["after_softmax"] else torch.log_softmax(x.double(), -1).to(x.dtype)).to(DEV)
    tg, xl, tl = (torch.from_numpy(c[k]).to(DEV) for k in ("targets", "x_len", "t_len"))
    loss, grad = abi_call(lp, tg, xl, tl, int(c["space_idx"]))
    # (the f32 log-probabilities are rounded: compare against the restatement on exactly those)
    want_l, want_g = NR.noblank_loss_grad(lp.double().cpu().numpy(), c["targets"], c["x_len"], c["t_len"], int(c["space_idx"]))
    check_losses(loss, want_l, tol(c))
    check_grads(grad, want_g, tol(c))
    if c["logits"].dtype == np.float64:
        check_losses(loss, c["eng_loss"], 1e-9)
        check_grads(grad, c["eng_grad"], 1e-9)
    if np.isinf(want_l).any():                # infeasible: +inf, NaN rows t < x_len, zeros beyond; neighbours finite
        b = int(np.flatnonzero(np.isinf(want_l))[0])
        n = int(c["x_len"][b])
        assert np.isnan(grad[b, :n]).all() and (grad[b, n:] == 0).all()
        assert np.isfinite(np.delete(loss, b)).all()


@pytest.mark.parametrize("name", ALIGNED)
def test_aligned_targets_loss_matches_reference_fixtures(name):
    from end2end_amd import AlignedTargetsLoss
    c = case(name)
    x = torch.from_numpy(c["log_probs"]).to(DEV).requires_grad_()
    tg, xl, tl = (torch.from_numpy(c[k]).to(DEV) for k in ("targets", "x_len", "t_len"))
    loss = AlignedTargetsLoss(bool(c["is_ctc"]), ignore_blank=bool(c["ignore_blank"]))(x, tg, xl, tl)
    loss.sum().backward()
    assert loss.device == x.device
    np.testing.assert_allclose(loss.detach().cpu().numpy(), c["loss"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(x.grad.cpu().numpy(), c["grad"], rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("space_idx", [-1, 4])
@pytest.mark.parametrize("after_softmax", [False, True])
def test_gradcheck_f64(space_idx, after_softmax):
    from end2end_amd import CTCWithoutBlankLoss
    g = torch.Generator().manual_seed(5 + space_idx)
    B, T, V = 3, 12, 5
    x = torch.randn(B, T, V, generator=g, dtype=torch.float64).to(DEV).requires_grad_()
    tg = torch.randint(0, 4, (B, 3), generator=g).to(DEV)
    xl = torch.tensor([12, 9, 6], device=DEV)
    tl = torch.tensor([3, 2, 1], device=DEV)
    mod = CTCWithoutBlankLoss(reduce=False, after_softmax=after_softmax, space_idx=space_idx)
    fn = (lambda z: mod(torch.softmax(z, -1), tg, xl, tl)) if after_softmax else (lambda z: mod(z, tg, xl, tl))
    assert torch.autograd.gradcheck(fn, (x,), eps=1e-6, atol=1e-6, rtol=1e-5)


def test_loss_bounds_the_asg_viterbi_alignment_and_meets_it_on_peaky_inputs():
    from end2end_amd import CTCWithoutBlankLoss
    from end2end_amd.utils.alignment import get_alignment_3d
    g = torch.Generator().manual_seed(11)
    B, T, V, S = 6, 40, 9, 8
    tg = torch.randint(0, V, (B, S), generator=g)
    for i in range(1, S):                           # no label twice in a row: one frame labelling = one lattice path
        tg[:, i] = (tg[:, i - 1] + torch.randint(1, V, (B,), generator=g)) % V
    tl = torch.randint(3, S + 1, (B,), generator=g)
    xl = torch.randint(20, T + 1, (B,), generator=g)
    for peaky in (False, True):
        x = torch.randn(B, T, V, generator=g, dtype=torch.float64)
        if peaky:                                   # one labelling path 40 nats above everything else
            for b in range(B):
                n, s = int(xl[b]), int(tl[b])
                cuts = np.sort(np.random.RandomState(b).choice(np.arange(1, n), s - 1, replace=False))
                seg = np.searchsorted(cuts, np.arange(n), side="right")
                x[b, np.arange(n), tg[b, seg]] += 40.0
        lp = torch.log_softmax(x, -1).to(DEV)
        loss = CTCWithoutBlankLoss(reduce=False)(lp, tg.to(DEV), xl.to(DEV), tl.to(DEV)).cpu()
        al = get_alignment_3d(lp, tg, xl, tl, is_ctc=False)
        lpc = lp.cpu()
        for b in range(B):
            n = int(xl[b])
            vit = float(lpc[b, torch.arange(n), al[b, :n]].sum())
            assert -loss[b].item() >= vit - 1e-9
            if peaky:
                assert abs(-loss[b].item() - vit) <= 1e-3


def _ragged(seed, B, T, V, S, space_idx, scale=1.0, min_t=None):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, V, generator=g) * scale
    tg = torch.randint(0, V, (B, S), generator=g)
    tl = torch.randint(max(S // 2, 0), S + 1, (B,), generator=g)
    xl = torch.randint(min_t or max(T // 2, 1), T + 1, (B,), generator=g)
    xl[0] = T
    xl = torch.maximum(xl, tl)
    return x, tg, xl, tl


def _engine_vs_ref(x, tg, xl, tl, space_idx, logprobs=False):
    from end2end_amd.engines import CTCWithoutBlankLossEngine
    eng = CTCWithoutBlankLossEngine(space_idx)
    loss, grad = eng.compute(x.to(DEV), tg.to(DEV), xl.to(DEV), tl.to(DEV), input_is_logprobs=logprobs)
    flags = eng.redo_flags()
    lp = x.double() if logprobs else torch.log_softmax(x.double(), -1)
    want_l, want_g = NR.noblank_loss_grad(lp.numpy(), tg.numpy(), xl.numpy(), tl.numpy(), space_idx)
    tol = 1e-9 if x.dtype == torch.float64 else 1e-5
    check_losses(loss.cpu().numpy(), want_l, tol)
    check_grads(grad.cpu().numpy(), want_g, tol)
    return flags


@pytest.mark.parametrize("space_idx", [-1, 28])
def test_headline_shape_against_restatement(space_idx):
    x, tg, xl, tl = _ragged(21, 256, 1000, 29, 200, space_idx, min_t=450)
    _engine_vs_ref(x, tg, xl, tl, space_idx)


@pytest.mark.parametrize("B,T,V,S", [(16, 256, 8000, 60), (2, 64, 32000, 20)])
def test_large_alphabets_against_restatement(B, T, V, S):
    x, tg, xl, tl = _ragged(22, B, T, V, S, 3)
    _engine_vs_ref(x, tg, xl, tl, 3)


def test_permuted_view_against_restatement():
    g = torch.Generator().manual_seed(23)
    B, T, V = 8, 120, 29
    x = torch.randn(T, B, V, generator=g).permute(1, 0, 2)
    assert not x.is_contiguous()
    _, tg, xl, tl = _ragged(23, B, T, V, 30, 0)
    _engine_vs_ref(x, tg, xl, tl, 0)


def test_zero_probabilities_give_minus_inf_log_probs():
    g = torch.Generator().manual_seed(24)
    B, T, V = 6, 50, 12
    p = torch.softmax(torch.randn(B, T, V, generator=g), -1)
    p[torch.rand(B, T, V, generator=g) < 0.2] = 0.0
    p = p / p.sum(-1, keepdim=True)
    _, tg, xl, tl = _ragged(24, B, T, V, 10, -1)
    _engine_vs_ref(torch.log(p), tg, xl, tl, -1, logprobs=True)
    _engine_vs_ref(torch.log(p), tg, xl, tl, 5, logprobs=True)


def test_log_probs_below_minus_700_take_the_log_domain():
    x, tg, xl, tl = _ragged(25, 8, 80, 10, 20, 2, scale=200.0)
    lp = torch.log_softmax(x.double(), -1)
    assert ((lp > -np.inf) & (lp < -700)).any()
    flags = _engine_vs_ref(x, tg, xl, tl, 2)
    assert (flags == 1).all(), flags                        # (the forward's redo: e2e_debug_noblank_redo_flags)
    _engine_vs_ref(x * 0.3, tg, xl, tl, -1)                 # (scale x60)


def nb_block(Smax):
    """The LDS block K of the lattice kernel (ctc_loss_noblank.hip nb_lds_bytes / nb_block), restated; 0: not served."""
    Lm = Smax + 2
    for K in range(16, 0, -1):
        if 8 * (3 * (K + 1) * Lm + 2 * K * Lm + 2 * Lm) + 4 * (2 * Lm + 2 * K) + 64 <= 160 * 1024 - 288:
            return K
    return 0


@pytest.mark.parametrize("space_idx", [-1, 3])
@pytest.mark.parametrize("dt", [torch.float32, torch.float64])
@pytest.mark.parametrize("S,K", [(240, 15), (320, 11), (420, 8), (600, 5), (900, 3), (1100, 2), (1500, 1), (1855, 1)])
def test_blocks_shorter_than_16_frames_against_restatement(S, K, dt, space_idx):
    # Targets long enough that the LDS block K -- the checkpoint interval -- drops below 16 frames; most of these K do not
    # divide 16, and the backward hands the blocks through its three-slot ring.  Smax = 1855 is the last width served.
    # Ragged lengths end utterances on the first frame of a block (a checkpoint), on its last frame and in between.
    assert nb_block(S) == K and nb_block(1855) == 1 and nb_block(1856) == 0
    g = torch.Generator().manual_seed(S + K)
    B, T, V = 3, S + 2 * K + 5, 29
    x = torch.randn(B, T, V, generator=g).to(dt)
    tg = torch.randint(0, V, (B, S), generator=g)
    tl = torch.tensor([S, S - 5, S - 13])
    first = -(-(S - 6) // K) * K + 1                 # x_len - 1 a multiple of K, x_len >= t_len
    last = -(-(S - 13) // K) * K                     # x_len a multiple of K
    xl = torch.tensor([T, first, last])
    assert (xl >= tl).all() and (xl <= T).all() and (first - 1) % K == 0 and last % K == 0
    _engine_vs_ref(x, tg, xl, tl, space_idx)


@pytest.mark.parametrize("dt", [torch.float32, torch.float64])
def test_the_widest_row_of_every_block_size_launches(dt):
    # Regression: the LDS limit left less room than the kernel's static LDS takes, and the two widths whose blocks filled
    # it (Smax 784 and 1856) failed to launch.  784 (now K = 3) and the last width of every block size, short targets
    # padded to it; 1856 is refused with the documented error.
    from end2end_amd.engines import CTCWithoutBlankLossEngine
    g = torch.Generator().manual_seed(31)
    B, T, V = 3, 40, 29
    widths = [784] + [max(s for s in range(1856) if nb_block(s) == K) for K in range(1, 17)]
    assert nb_block(784) == 3 and widths[1] == 1855
    with pytest.raises(Exception, match="Smax=1856"):
        CTCWithoutBlankLossEngine(5).compute(torch.randn(B, T, V, device=DEV), torch.zeros(B, 1856, dtype=torch.long),
                                             torch.tensor([40, 33, 17]), torch.tensor([30, 12, 0]))
    for W in widths:
        x = torch.randn(B, T, V, generator=g).to(dt)
        tg = torch.full((B, W), -1, dtype=torch.long)
        tg[:, :30] = torch.randint(0, V, (B, 30), generator=g)
        _engine_vs_ref(x, tg, torch.tensor([40, 33, 17]), torch.tensor([30, 12, 0]), 5)


def test_reduce_and_weighted_backward():
    from end2end_amd import CTCWithoutBlankLoss
    x, tg, xl, tl = _ragged(26, 5, 30, 7, 6, 1)
    x = x.to(DEV)
    args = (tg.to(DEV), xl.to(DEV), tl.to(DEV))
    x1 = x.clone().requires_grad_()
    per = CTCWithoutBlankLoss(reduce=False, space_idx=1)(x1, *args)
    w = torch.linspace(0.3, 2.0, 5, device=DEV)
    (per * w).sum().backward()
    x2 = x.clone().requires_grad_()
    tot = CTCWithoutBlankLoss(reduce=True, space_idx=1)(x2, *args)
    tot.backward()
    assert tot.dim() == 0 and torch.allclose(tot, per.detach().sum(), rtol=1e-6)
    x3 = x.clone().requires_grad_()
    CTCWithoutBlankLoss(reduce=False, space_idx=1)(x3, *args).sum().backward()
    assert torch.allclose(x2.grad, x3.grad, atol=1e-7)
    assert torch.allclose(x1.grad, x3.grad * w[:, None, None], atol=1e-6)


def test_cpu_tensors_in_give_cpu_tensors_out():
    from end2end_amd import CTCWithoutBlankLoss
    x, tg, xl, tl = _ragged(27, 3, 20, 6, 5, -1)
    xc = x.clone().requires_grad_()
    loss = CTCWithoutBlankLoss(reduce=False)(xc, tg, xl, tl)
    loss.sum().backward()
    assert loss.device.type == "cpu" and xc.grad.device.type == "cpu"
    xg = x.to(DEV).requires_grad_()
    lg = CTCWithoutBlankLoss(reduce=False)(xg, tg.to(DEV), xl.to(DEV), tl.to(DEV))
    lg.sum().backward()
    assert torch.equal(loss, lg.cpu()) and torch.equal(xc.grad, xg.grad.cpu())


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_16bit_inputs_equal_their_f32_upcast(dt):
    from end2end_amd.engines import CTCWithoutBlankLossEngine
    x, tg, xl, tl = _ragged(28, 4, 30, 8, 6, 7)
    x16 = x.to(dt).to(DEV)
    eng = CTCWithoutBlankLossEngine(7)
    l16, g16 = eng.compute(x16, tg, xl, tl, input_is_logprobs=False)
    l32, g32 = eng.compute(x16.float(), tg, xl, tl, input_is_logprobs=False)
    assert l16.dtype == dt and g16.dtype == dt
    assert torch.equal(l16, l32.to(dt)) and torch.equal(g16, g32.to(dt))


def test_bad_lengths_or_labels_poison_only_their_utterance():
    from end2end_amd.engines import CTCWithoutBlankLossEngine
    x, tg, xl, tl = _ragged(29, 5, 20, 6, 5, -1)
    xl[1] = 21          # > T
    tl[2] = 6           # > Smax
    tg[3, 0] = 6        # outside [0, V)
    tl[3] = max(int(tl[3]), 1)
    loss, grad = CTCWithoutBlankLossEngine(-1).compute(x.to(DEV), tg, xl, tl, input_is_logprobs=False)
    loss, grad = loss.cpu(), grad.cpu()
    for b in (1, 2, 3):
        assert torch.isnan(loss[b]) and torch.isnan(grad[b]).all()
    for b in (0, 4):
        assert torch.isfinite(loss[b]) and not torch.isnan(grad[b]).any()


def test_two_streams_and_a_shared_workspace_give_identical_results():
    from end2end_amd.engines import CTCWithoutBlankLossEngine
    x, tg, xl, tl = _ragged(30, 16, 200, 29, 40, 0)
    x, tg, xl, tl = (t.to(DEV) for t in (x, tg, xl, tl))
    eng = CTCWithoutBlankLossEngine(0)
    a = eng.compute(x, tg, xl, tl, input_is_logprobs=False)
    b = eng.compute(x, tg, xl, tl, input_is_logprobs=False)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        c = eng.compute(x, tg, xl, tl, input_is_logprobs=False)
    torch.cuda.synchronize()
    for r in (b, c):
        assert torch.equal(a[0], r[0]) and torch.equal(a[1], r[1])
