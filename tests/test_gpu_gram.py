"""GPU: Gram-CTC (e2e_gram_ctc_fwd_bwd through GramCTCLossEngine / GramCTCLoss) against brute force over every path,
against CTC (the reference's arithmetic, oracle_lib) when the table holds unigrams only, and against the test-side f64
lattice (tests/gram_ref.py) at larger shapes."""
import numpy as np
import pytest
import torch

import gram_ref as GR
import oracle_lib as O

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


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


def engine(R, V, l2i):
    from end2end_amd.engines import GramCTCLossEngine
    return GramCTCLossEngine(0, R, V, l2i)


def run(eng, x, tg, xl, tl, logprobs=False):
    loss, grad = eng.compute(x.to(DEV), tg.to(DEV), xl.to(DEV), tl.to(DEV), input_is_logprobs=logprobs)
    return loss.cpu().numpy(), grad.cpu().numpy()


def vs_ref(R, V, l2i, x, tg, xl, tl, logprobs=False, method=GR.lattice):
    loss, grad = run(engine(R, V, l2i), x, tg, xl, tl, logprobs)
    lp = x.double() if logprobs else torch.log_softmax(x.double(), -1)
    want_l, want_g = GR.loss_grad(lp.numpy(), tg.numpy(), xl.numpy(), tl.numpy(), GR.grams_of(R, V, l2i), method)
    tol = 1e-9 if x.dtype == torch.float64 else 1e-5
    check_losses(loss, want_l, tol)
    check_grads(grad, want_g, tol)
    return loss, grad


@pytest.mark.parametrize("logprobs", [False, True])
@pytest.mark.parametrize("dt", [torch.float32, torch.float64])
def test_kernel_equals_brute_force_on_tiny_cases(dt, logprobs):
    rng = np.random.default_rng(77)
    for _ in range(40):
        R, V, l2i, x, tgt = GR.random_tiny_case(rng)
        x = torch.from_numpy(x)[None].to(dt)
        if logprobs:
            x = torch.log_softmax(x, -1)
        S = len(tgt)
        tg = torch.tensor([tgt + [1]], dtype=torch.long)
        vs_ref(R, V, l2i, x, tg, torch.tensor([x.shape[1]]), torch.tensor([S]), logprobs, GR.brute_force)


def _ragged(seed, B, T, V, S, R=None, scale=1.0, min_t=None):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, V, generator=g) * scale
    tg = torch.randint(1, R or V, (B, S), generator=g)
    tl = torch.randint(max(S // 2, 0), S + 1, (B,), generator=g)
    xl = torch.randint(min_t or max(T // 2, 1), T + 1, (B,), generator=g)
    xl[0] = T
    xl = torch.maximum(xl, 2 * tl + 1).clamp(max=T)
    return x, tg, xl, tl


@pytest.mark.parametrize("B,T,S,seed", [(8, 1000, 200, 41), (12, 400, 150, 42)])
def test_unigrams_only_equal_ctc_with_blank_0(B, T, S, seed):
    V = 29
    x, tg, xl, tl = _ragged(seed, B, T, V, S, min_t=2 * S + 2)
    loss, grad = run(engine(V, V, {}), x, tg, xl, tl)
    lp = torch.log_softmax(x.double(), -1).numpy()
    l_ref, g_ref = O.ctc_loss(lp, tg.numpy(), xl.numpy(), tl.numpy(), 0)
    check_losses(loss, l_ref, 1e-5)
    for b in range(B):
        n = int(xl[b])
        check_grads(grad[b, :n], g_ref[b, :n], 1e-5)
        assert (grad[b, n:] == 0).all()


def gram_table(rng, R, *counts):
    """counts[i] random grams of order i + 2 over the base labels 1..R-1 -> (label2ids, V)"""
    l2i, seen, c = {}, set(), R
    for k, n in enumerate(counts, start=2):
        while sum(len(v) == k for v in l2i.values()) < n:
            s = tuple(int(v) for v in rng.integers(1, R, size=k))
            if s not in seen:
                seen.add(s)
                l2i[c] = list(s)
                c += 1
    return l2i, c


def dense_targets(rng, l2i, R, B, S):
    grams = list(l2i.values())
    tg = np.zeros((B, S), dtype=np.int64)
    for b in range(B):
        t = []
        while len(t) < S:
            g = grams[int(rng.integers(len(grams)))] if rng.random() < 0.75 else [int(rng.integers(1, R))]
            t += g * int(rng.integers(1, 3))              # the same gram twice in a row, often
        tg[b] = t[:S]
    return torch.from_numpy(tg)


@pytest.mark.parametrize("logprobs", [False, True])
@pytest.mark.parametrize("dt", [torch.float32, torch.float64])
def test_bigrams_and_trigrams_against_the_lattice(dt, logprobs):
    rng = np.random.default_rng(5)
    R = 8
    l2i, V = gram_table(rng, R, 20, 10)
    B, T, S = 16, 300, 120
    x, _, xl, tl = _ragged(43, B, T, V, S, R=R, min_t=200)
    tg = dense_targets(rng, l2i, R, B, S)
    x = x.to(dt)
    if logprobs:
        x = torch.log_softmax(x, -1)
    vs_ref(R, V, l2i, x, tg, xl, tl, logprobs)


def test_wide_table_against_the_lattice():
    rng = np.random.default_rng(6)
    R = 29
    l2i, V = gram_table(rng, R, 700, 900, 371)
    assert V == 2000
    B, T, S = 8, 256, 60
    x, _, xl, tl = _ragged(44, B, T, V, S, R=R, min_t=130)
    tg = dense_targets(rng, l2i, R, B, S)
    vs_ref(R, V, l2i, x, tg, xl, tl)


@pytest.mark.parametrize("dt", [torch.float32, torch.float64])
def test_masked_gram_gives_the_loss_of_the_table_without_it(dt):
    rng = np.random.default_rng(8)
    R = 6
    l2i, V = gram_table(rng, R, 6, 3)
    B, T, S = 6, 80, 20
    x, _, xl, tl = _ragged(45, B, T, V, S, R=R, min_t=60)
    tg = dense_targets(rng, l2i, R, B, S)
    lp = torch.log_softmax(x.double(), -1).to(dt)
    masked = lp.clone()
    masked[:, :, V - 1] = -np.inf
    l1, g1 = run(engine(R, V, l2i), masked, tg, xl, tl, logprobs=True)
    small = dict(l2i)
    del small[V - 1]
    l2, g2 = run(engine(R, V - 1, small), lp[:, :, :V - 1].contiguous(), tg, xl, tl, logprobs=True)
    tol = 1e-9 if dt == torch.float64 else 1e-5
    check_losses(l1, l2, tol)
    check_grads(g1[:, :, :V - 1], g2, tol)


def test_gradcheck_f64():
    from end2end_amd import GramCTCLoss
    l2i = {4: [1, 2], 5: [2, 2], 6: [1, 2, 3]}
    g = torch.Generator().manual_seed(9)
    B, T, V = 3, 10, 7
    x = torch.randn(B, T, V, generator=g, dtype=torch.float64).to(DEV).requires_grad_()
    tg = torch.tensor([[1, 2, 2, 2], [1, 2, 3, 1], [2, 2, 0, 0]], device=DEV)
    xl = torch.tensor([10, 8, 5], device=DEV)
    tl = torch.tensor([4, 4, 2], device=DEV)
    mod = GramCTCLoss(0, 4, V, l2i, reduce=False, after_logsoftmax=False)
    assert torch.autograd.gradcheck(lambda z: mod(z, tg, xl, tl), (x,), eps=1e-6, atol=1e-6, rtol=1e-5)


def test_reduce_size_average_time_major_and_strides():
    from end2end_amd import GramCTCLoss
    rng = np.random.default_rng(10)
    R = 6
    l2i, V = gram_table(rng, R, 5, 2)
    B, T, S = 5, 40, 10
    x, _, xl, tl = _ragged(46, B, T, V, S, R=R)
    tg = dense_targets(rng, l2i, R, B, S).to(DEV)
    x, xl, tl = x.to(DEV), xl.to(DEV), tl.to(DEV)
    x1 = x.clone().requires_grad_()
    per = GramCTCLoss(0, R, V, l2i)(x1, tg, xl, tl)
    per.sum().backward()
    x2 = x.clone().requires_grad_()
    tot = GramCTCLoss(0, R, V, l2i, reduce=True, size_average=False)(x2, tg, xl, tl)
    tot.backward()
    x3 = x.clone().requires_grad_()
    mean = GramCTCLoss(0, R, V, l2i, reduce=True, size_average=True)(x3, tg, xl, tl)
    mean.backward()
    assert per.shape == (B,) and tot.dim() == 0 and mean.dim() == 0
    assert torch.allclose(tot, per.detach().sum(), rtol=1e-6) and torch.allclose(mean * B, tot, rtol=1e-6)
    assert torch.allclose(x1.grad, x2.grad, atol=1e-7) and torch.allclose(x3.grad * B, x2.grad, atol=1e-6)
    xt = x.permute(1, 0, 2).contiguous().requires_grad_()          # (T, B, V); the kernel reads the strided view
    lt = GramCTCLoss(0, R, V, l2i, time_major=True)(xt, tg, xl, tl)
    lt.sum().backward()
    assert torch.allclose(lt, per.detach(), rtol=1e-6) and torch.allclose(xt.grad.permute(1, 0, 2), x1.grad, atol=1e-7)
    wide = torch.zeros(B, T, 2 * V, device=DEV)
    wide[:, :, ::2] = x
    xs = wide[:, :, ::2]
    assert not xs.is_contiguous()
    ls = GramCTCLoss(0, R, V, l2i, fused=False)(xs, tg, xl, tl)
    assert torch.allclose(ls, per.detach(), rtol=1e-5)


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_16bit_inputs_equal_their_f32_upcast(dt):
    rng = np.random.default_rng(11)
    R = 6
    l2i, V = gram_table(rng, R, 4, 2)
    x, _, xl, tl = _ragged(47, 4, 30, V, 6, R=R)
    tg = dense_targets(rng, l2i, R, 4, 6)
    x16 = x.to(dt).to(DEV)
    eng = engine(R, V, l2i)
    l16, g16 = eng.compute(x16, tg, xl, tl, input_is_logprobs=False)
    l32, g32 = eng.compute(x16.float(), tg, xl, tl, input_is_logprobs=False)
    assert l16.dtype == dt and g16.dtype == dt
    assert torch.equal(l16, l32.to(dt)) and torch.equal(g16, g32.to(dt))


def test_edge_shapes():
    l2i = {4: [1, 1], 5: [1, 2, 3]}
    eng = engine(4, 6, l2i)
    loss, grad = eng.compute(torch.zeros(0, 5, 6, device=DEV), torch.zeros(0, 3, dtype=torch.long), torch.zeros(0, dtype=torch.long),
                             torch.zeros(0, dtype=torch.long))
    assert loss.shape == (0,) and grad.shape == (0, 5, 6)
    g = torch.Generator().manual_seed(12)
    x = torch.randn(3, 7, 6, generator=g, dtype=torch.float64)
    vs_ref(4, 6, l2i, x, torch.zeros(3, 0, dtype=torch.long), torch.tensor([7, 3, 1]), torch.tensor([0, 0, 0]))   # S = 0
    x1 = torch.randn(2, 1, 6, generator=g, dtype=torch.float64)                                                  # T = 1
    vs_ref(4, 6, l2i, x1, torch.tensor([[1, 2, 3], [1, 1, 0]]), torch.tensor([1, 1]), torch.tensor([3, 2]))


def test_a_target_feasible_only_through_grams():
    # "a a b c" needs 5 frames under CTC (a _ a b c); with the grams "aa" and "abc" it fits in 2 (a | abc)
    l2i = {4: [1, 1], 5: [1, 2, 3]}
    x = torch.randn(2, 2, 6, generator=torch.Generator().manual_seed(13), dtype=torch.float64)
    loss, _ = vs_ref(4, 6, l2i, x, torch.tensor([[1, 1, 2, 3], [1, 1, 2, 3]]), torch.tensor([2, 2]), torch.tensor([4, 4]))
    assert np.isfinite(loss).all()
    lc, _ = run(engine(4, 4, {}), x[:, :, :4].contiguous(), torch.tensor([[1, 1, 2, 3]] * 2), torch.tensor([2, 2]),
                torch.tensor([4, 4]))
    assert np.isinf(lc).all()


@pytest.mark.parametrize("dt", [torch.float32, torch.float64])
def test_infeasible_and_bad_utterances_poison_only_themselves(dt):
    l2i = {4: [1, 1], 5: [1, 2, 3]}
    g = torch.Generator().manual_seed(14)
    B, T = 6, 12
    x = torch.randn(B, T, 6, generator=g).to(dt)
    tg = torch.randint(1, 4, (B, 8), generator=g)
    tl = torch.full((B,), 6)
    xl = torch.full((B,), T)
    tl[1], xl[1] = 8, 3                  # infeasible: 8 labels, no gram covers them in 3 frames
    tg[1] = torch.tensor([1, 2, 1, 2, 1, 2, 1, 2])
    tg[2, 0] = 0                         # a target id of 0
    tg[3, 2] = 4                         # a target id >= R
    xl[4] = T + 1                        # a bad length
    loss, grad = run(engine(4, 6, l2i), x, tg, xl, tl)
    assert np.isinf(loss[1]) and loss[1] > 0 and np.isnan(grad[1, :3]).all() and (grad[1, 3:] == 0).all()
    for b in (2, 3, 4):
        assert np.isnan(loss[b]) and np.isnan(grad[b]).all()
    for b in (0, 5):
        assert np.isfinite(loss[b]) and not np.isnan(grad[b]).any()
    ok = [0, 5]
    vs_ref(4, 6, l2i, x[ok], tg[ok], xl[ok], tl[ok])


@pytest.mark.parametrize("scale,T,why,order", [
    pytest.param(8.0, 600, 2, 3, id="8.0-600-2"), pytest.param(14.0, 600, 2, 3, id="14.0-600-2"),
    pytest.param(20.0, 600, 2, 3, id="20.0-600-2"), pytest.param(300.0, 120, 1, 3, id="300.0-120-1"),
    pytest.param(14.0, 600, 2, 6, id="order6-14.0-600-2"), pytest.param(300.0, 120, 1, 6, id="order6-300.0-120-1")])
def test_sharp_logits_take_the_log_domain_redo_and_still_match(scale, T, why, order):
    # Sharp logits unrelated to the targets: at scale 8-20 over 600 frames cells that carry paths flush to zero under their
    # row's scale, the backward finds frames whose posteriors do not sum to 1 and redoes the utterance (flag 2); at scale
    # 300 log-probabilities fall below -700 and the forward sends every utterance to the log domain (flag 1).  Tables of
    # max_order 3 and 6.
    rng = np.random.default_rng(15)
    R = 8
    l2i, V = gram_table(rng, R, 10, 5, *([3] * (order - 3)))
    B, S = 8, 30
    x, _, xl, tl = _ragged(48, B, T, V, S, R=R, scale=scale, min_t=80)
    tg = dense_targets(rng, l2i, R, B, S)
    eng = engine(R, V, l2i)
    loss, grad = run(eng, x, tg, xl, tl)
    flags = eng.redo_flags()
    assert (flags == why).any() and set(flags.tolist()) <= {0, 1, 2}, flags
    if why == 1:
        assert (flags == 1).all()
    want_l, want_g = GR.loss_grad(torch.log_softmax(x.double(), -1).numpy(), tg.numpy(), xl.numpy(), tl.numpy(),
                                  GR.grams_of(R, V, l2i))
    check_losses(loss, want_l, 1e-5)
    check_grads(grad, want_g, 1e-5)


def gc_block(S, M):
    """The LDS block of the lattice kernel (ctc_loss_gram.hip gc_lds_bytes / gc_block), restated."""
    NC = (S + 1) * (M + 1)
    for K in (16, 8, 4, 2, 1):
        if 8 * (2 * K * NC + 4 * NC + 4 * K) + 4 * (3 * NC + S + 1 + K + 16) + 64 <= 160 * 1024 - 256:
            return K
    return 0


@pytest.mark.parametrize("dt", [torch.float32, torch.float64])
@pytest.mark.parametrize("S,T,K,M", [
    pytest.param(200, 437, 8, 3, id="200-437-8"), pytest.param(300, 650, 4, 3, id="300-650-4"),
    pytest.param(500, 1013, 2, 3, id="500-1013-2"), pytest.param(668, 1341, 1, 3, id="668-1341-1"),
    pytest.param(200, 437, 4, 5, id="order5-200-437-4"), pytest.param(447, 931, 1, 5, id="order5-447-931-1"),
    pytest.param(250, 537, 2, 6, id="order6-250-537-2"), pytest.param(336, 709, 1, 7, id="order7-336-709-1"),
    pytest.param(50, 137, 16, 8, id="order8-50-137-16"), pytest.param(80, 197, 8, 8, id="order8-80-197-8"),
    pytest.param(120, 277, 4, 8, id="order8-120-277-4"), pytest.param(200, 437, 2, 8, id="order8-200-437-2"),
    pytest.param(290, 617, 1, 8, id="order8-290-617-1")])
def test_blocks_shorter_than_the_checkpoint_interval_against_the_lattice(dt, S, T, K, M):
    # Targets long enough that the LDS block K is below the 16-frame checkpoint interval: the backward recomputes every
    # block from its checkpoint through the blocks ahead of it.  Ragged lengths end utterances inside a block and away
    # from a checkpoint.  Tables of max_order M: grams of every order 2..M, spelled into the targets.
    assert gc_block(S, M) == K
    rng = np.random.default_rng(S)
    R = 29
    l2i, V = gram_table(rng, R, 60, 20, *([8] * (M - 3)))
    B = 3
    tg = dense_targets(rng, l2i, R, B, S)
    tl = torch.tensor([S, S - 5, S - 13])
    xl = torch.tensor([T, T - 7, T - 26])
    x = torch.randn(B, T, V, generator=torch.Generator().manual_seed(S)).to(dt)
    vs_ref(R, V, l2i, x, tg, xl, tl)


@pytest.mark.parametrize("dt", [torch.float32, torch.float64])
def test_radix_234_order_8_keys_near_the_int64_limit_against_the_lattice(dt):
    # 234 ** 8 - 1 = 0.975 * INT64_MAX: the largest key a table can hold is the gram of eight 233s.  The table mixes it with
    # other order-8 grams of high labels, its own prefix and suffix, and grams of every lower order; the targets spell them.
    rng = np.random.default_rng(234)
    R = 234
    top = [R - 1] * 8
    assert (R ** 8 - 1) / (2 ** 63 - 1) > 0.97
    l2i, V = gram_table(rng, R, 6, 4, 3, 3, 3, 3, 3)
    for g in (top, top[:-1], [R - 2] + top[1:], [R - 1, R - 2] * 4):
        if g not in l2i.values():
            l2i[V] = g
            V += 1
    B, T, S = 4, 160, 120
    assert gc_block(S, 8) == 4
    tg = dense_targets(rng, l2i, R, B, S)
    tg[0, :16] = torch.tensor(top + top)                  # the top key twice in a row (a blank between them)
    x, _, xl, tl = _ragged(50, B, T, V, S, R=R, min_t=100)
    xl[1:] = torch.tensor([T - 1, 99, 120])
    vs_ref(R, V, l2i, x.to(dt), tg, xl, tl)


def test_one_label_past_the_documented_limit_raises():
    eng = engine(29, 30, {29: [1, 2, 3]})
    assert eng.max_target_length() == 668
    x = torch.randn(1, 20, 30, device=DEV)
    with pytest.raises(ValueError, match="668"):
        eng.compute(x, torch.ones(1, 669, dtype=torch.long), torch.tensor([20]), torch.tensor([3]))


def test_module_trains_through_the_upstream_import_path():
    from pytorch_end2end.modules.ctc_loss import GramCTCLoss
    rng = np.random.default_rng(16)
    R = 6
    l2i, V = gram_table(rng, R, 4, 2)
    x, _, xl, tl = _ragged(49, 4, 40, V, 8, R=R)
    tg = dense_targets(rng, l2i, R, 4, 8)
    w = torch.nn.Parameter(x.to(DEV))
    opt = torch.optim.SGD([w], lr=0.5)
    mod = GramCTCLoss(0, R, V, l2i, reduce=True, size_average=True)
    first = None
    for _ in range(5):
        opt.zero_grad()
        loss = mod(w, tg.to(DEV), xl.to(DEV), tl.to(DEV))
        loss.backward()
        opt.step()
        first = first if first is not None else loss.item()
    assert loss.item() < first
