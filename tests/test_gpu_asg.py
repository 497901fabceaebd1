"""GPU: ASG (e2e_asg_fwd_bwd, e2e_asg_viterbi; ASGLoss, asg_loss, ASGDecoder) against the test-side f64 restatement
(tests/asg_ref.py) and its brute force.  Tolerances are test_gpu_noblank.py's: f32 inputs 1e-5 (losses and transition
slabs relative to max(1, |want|), emission gradients absolute), f64 inputs 1e-9; inf / NaN patterns equal.  Every loss case
also checks the best path of the same inputs: paths and merged ids exactly, scores to 1e-12 relative, score <= FCC."""
import ctypes as C

import numpy as np
import pytest
import torch

import asg_ref as AR

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
DTYPES = {"f32": torch.float32, "f64": torch.float64}
# what the kernels' paths turn on (end2end_amd/csrc/ctc_loss_asg.hip): the padded alphabet VP = 32 / 64 / 128 of the dense
# kernels, and the target lattice's two cells per thread of a 256-thread workgroup (limit 512 labels)
VP_EDGES = (31, 32, 33, 63, 64, 65, 127, 128)
THREADS = 256
CELL_EDGES = (THREADS - 1, THREADS, THREADS + 1, 2 * THREADS)


def make(B, T, V, S, dtype, seed, xs=1.0, ts=1.0, ragged=True):
    """Inputs rounded to `dtype` (the reference sees exactly what the kernels see): x (B,T,V), A (V,V), targets (B,S), lengths."""
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.normal(size=(B, T, V)) * xs).to(dtype)
    A = torch.from_numpy(rng.normal(size=(V, V)) * ts).to(dtype)
    tg = torch.from_numpy(rng.integers(0, V, size=(B, S)))
    if ragged:
        xl = torch.from_numpy(rng.integers(max(1, T // 2), T + 1, size=B))
        xl[0] = T
        tl = torch.from_numpy(np.array([rng.integers(1, min(S, int(n)) + 1) for n in xl.tolist()]))
        tl[0] = min(S, T)
    else:
        xl, tl = torch.full((B,), T, dtype=torch.long), torch.full((B,), S, dtype=torch.long)
    return x, A, tg, xl, tl


def ref(x, A, tg, xl, tl):
    return AR.asg_ref(x.double().numpy(), A.double().numpy(), tg.numpy(), xl.numpy(), tl.numpy())


def engine(x, A, tg, xl, tl, grad_scale=1.0, device=DEV):
    from end2end_amd.engines import ASGLossEngine
    out = ASGLossEngine().compute(x.to(device), A.to(device), tg.to(device), xl.to(device), tl.to(device), grad_scale)
    return tuple(t.double().cpu().numpy() for t in out)


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


def check_slabs(got, want, rel):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok]) / np.maximum(1.0, np.abs(want[ok]))
    assert np.max(err, initial=0.0) <= rel, np.max(err, initial=0.0)


def check_against_ref(got, want, dtype):
    tol = 1e-9 if dtype == torch.float64 else 1e-5
    check_losses(got[0], want[0], tol)
    check_grads(got[1], want[1], tol)
    check_slabs(got[2], want[2], tol)


def viterbi(x, A, xl, device=DEV):
    from end2end_amd.engines import ASGViterbiEngine
    out = ASGViterbiEngine().compute(x.to(device), A.to(device), xl.to(device))
    return tuple(t.cpu().numpy() for t in out)


def check_best_path(x, A, xl):
    """Paths and merged ids equal the restatement's exactly, scores to 1e-12 relative, and score <= FCC."""
    got = viterbi(x, A, xl)
    want = AR.viterbi_ref(x.double().numpy(), A.double().numpy(), xl.numpy())
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
    assert np.array_equal(np.isnan(got[1]), np.isnan(want[1]))
    ok = ~np.isnan(want[1])
    assert np.all(np.abs(got[1][ok] - want[1][ok]) <= 1e-12 * np.maximum(1.0, np.abs(want[1][ok])))
    for b in np.flatnonzero(ok):
        n = int(xl[b])
        fcc = AR.fcc_one(x[b, :n].double().numpy(), A.double().numpy())[0]
        assert got[1][b] <= fcc + 1e-9 * max(1.0, abs(fcc))
    return got


def check_all(x, A, tg, xl, tl):
    got = engine(x, A, tg, xl, tl)
    check_against_ref(got, ref(x, A, tg, xl, tl), x.dtype)
    check_best_path(x, A, xl)
    return got


# ---- known answers by enumeration ----

@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_known_answers_by_enumeration(dt):
    dtype = DTYPES[dt]
    x, A, _, xl, _ = make(2, 4, 3, 3, dtype, 11, xs=1.5, ragged=False)
    tg = torch.tensor([[1, 1, 2], [0, 2, 2]])
    tl = torch.tensor([3, 3])
    losses = check_all(x, A, tg, xl, tl)[0]
    tol = 1e-9 if dtype == torch.float64 else 1e-5
    for b in range(2):
        want = AR.brute_loss(x[b].double().numpy(), A.double().numpy(), tg[b].tolist())
        assert abs(losses[b] - want) <= tol * max(1.0, abs(want))


# ---- degenerate sizes ----

@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_degenerate_sizes(dt):
    dtype = DTYPES[dt]
    tol = 1e-9 if dtype == torch.float64 else 1e-5
    x, A, tg, xl, tl = make(3, 1, 5, 1, dtype, 21, ragged=False)            # T = 1, S = 1
    got = check_all(x, A, tg, xl, tl)
    assert (got[2] == 0).all()                                              # no frame pair: exactly 0
    x, A, tg, xl, tl = make(3, 7, 5, 7, dtype, 22, ragged=False)            # T = S: one alignment
    check_all(x, A, tg, xl, tl)
    x, A, tg, xl, tl = make(3, 9, 1, 1, dtype, 23, ragged=False)            # V = 1: one path, one alignment
    tg.zero_()
    got = check_all(x, A, tg, xl, tl)
    assert np.abs(got[0]).max() <= tol * max(1.0, float(x.double().abs().sum(1).max()))
    assert np.abs(got[1]).max() <= tol and np.abs(got[2]).max() <= tol * 9
    x, A, tg, xl, tl = make(4, 9, 2, 4, dtype, 24)                          # V = 2
    check_all(x, A, tg, xl, tl)


# ---- wave and limit edges; the kernels' own edges ----

@pytest.mark.parametrize("V", VP_EDGES)
def test_alphabet_edges(V):
    for dt, seed in (("f32", 31), ("f64", 32)):
        x, A, tg, xl, tl = make(3, 40, V, 12, DTYPES[dt], seed + V)
        check_all(x, A, tg, xl, tl)


@pytest.mark.parametrize("S", CELL_EDGES)
def test_target_lattice_cell_edges(S):
    x, A, tg, xl, tl = make(2, S + 3, 5, S, torch.float32, 40 + S, ragged=False)
    tl[1] = S - 2
    xl[1] = S + 1
    check_all(x, A, tg, xl, tl)


@pytest.mark.parametrize("T", [2, 3])
def test_shortest_recurrences(T):
    x, A, tg, xl, tl = make(3, T, 7, 2, torch.float64, 50 + T)
    check_all(x, A, tg, xl, tl)


LONG = {}


def long_case(dt):
    if dt not in LONG:
        inp = make(8, 300, 29, 60, DTYPES[dt], 61)
        LONG[dt] = (inp, ref(*inp))
    return LONG[dt]


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_longer_ragged_batch(dt):
    inp, want = long_case(dt)
    check_against_ref(engine(*inp), want, DTYPES[dt])
    check_best_path(inp[0], inp[1], inp[3])


# ---- call shape ----

def abi_call(x, A, tg, xl, tl, grad_scale=1.0):
    from end2end_amd import _lib
    L = _lib.load()
    B, T, V = x.shape
    code = _lib.dtype_code(x.dtype)
    Smax = tg.shape[1]
    losses = torch.empty(B, dtype=x.dtype, device=DEV)
    grads = torch.empty((B, T, V), dtype=x.dtype, device=DEV)
    tgrads = torch.empty((B, V, V), dtype=x.dtype, device=DEV)
    ws = torch.empty(L.e2e_asg_workspace_bytes(B, T, V, Smax, code), dtype=torch.uint8, device=DEV)
    opts = _lib.LossOpts(grad_scale, None, 0, 0)
    _lib.check(L.e2e_asg_fwd_bwd(x.data_ptr(), code, *x.stride(), A.data_ptr(), tg.data_ptr(), tg.stride(0), xl.data_ptr(),
                                 tl.data_ptr(), B, T, V, Smax, losses.data_ptr(), grads.data_ptr(), tgrads.data_ptr(),
                                 ws.data_ptr(), ws.numel(), C.c_void_p(torch.cuda.current_stream().cuda_stream),
                                 C.byref(opts)))
    torch.cuda.synchronize()
    return tuple(t.double().cpu().numpy() for t in (losses, grads, tgrads))


def test_call_shape_padded_targets_stride_and_scale():
    x, A, tg, xl, tl = make(4, 20, 6, 8, torch.float32, 71)
    want = ref(x, A, tg, xl, tl)
    wide = torch.full((4, 13), 1 << 40, dtype=torch.long)                   # garbage beyond t_len, a row stride of 13
    for b in range(4):
        wide[b, :tl[b]] = tg[b, :tl[b]]
    view = wide.to(DEV)[:, :8]
    assert view.stride(0) == 13
    got = abi_call(x.to(DEV), A.to(DEV), view, xl.to(DEV), tl.to(DEV))
    check_against_ref(got, want, torch.float32)
    scaled = abi_call(x.to(DEV), A.to(DEV), view, xl.to(DEV), tl.to(DEV), grad_scale=0.25)
    check_losses(scaled[0], want[0], 1e-5)
    check_grads(scaled[1], 0.25 * want[1], 1e-5)
    check_slabs(scaled[2], 0.25 * want[2], 1e-5)
    check_against_ref(engine(x, A, wide[:, :8], xl, tl), want, torch.float32)     # the engine, same garbage


def test_call_shape_views_and_cpu_tensors():
    from end2end_amd import ASGLoss
    x, A, tg, xl, tl = make(4, 20, 6, 8, torch.float64, 72)
    want = ref(x, A, tg, xl, tl)
    tm = x.transpose(0, 1).contiguous().to(DEV)                             # (T,B,V) storage, a permuted view in
    assert not tm.transpose(0, 1).is_contiguous()
    check_against_ref(engine(tm.transpose(0, 1), A, tg, xl, tl), want, torch.float64)
    # the module: time-major emissions and a transposed view of the stored matrix
    mod = ASGLoss(6, reduce=False, time_major=True).to(DEV).double()
    mod.transitions.data = A.t().contiguous().to(DEV).t()
    assert not mod.transitions.is_contiguous()
    e = tm.clone().requires_grad_()
    loss = mod(e, tg.to(DEV), xl.to(DEV), tl.to(DEV))
    loss.sum().backward()
    check_losses(loss.detach().cpu().numpy(), want[0], 1e-9)
    check_grads(e.grad.transpose(0, 1).cpu().numpy(), want[1], 1e-9)
    check_slabs(mod.transitions.grad.cpu().numpy(), want[2].sum(0), 1e-9)
    from end2end_amd import asg_loss
    At = A.t().contiguous().to(DEV).requires_grad_()
    l2 = asg_loss(tm.transpose(0, 1), At.t(), tg.to(DEV), xl.to(DEV), tl.to(DEV))
    l2.sum().backward()
    check_losses(l2.detach().cpu().numpy(), want[0], 1e-9)
    check_slabs(At.grad.t().cpu().numpy(), want[2].sum(0), 1e-9)
    # CPU tensors in, CPU tensors out
    from end2end_amd.engines import ASGLossEngine
    out = ASGLossEngine().compute(x, A, tg, xl, tl)
    assert all(not t.is_cuda and t.dtype == torch.float64 for t in out)
    check_against_ref(tuple(t.numpy() for t in out), want, torch.float64)
    xc = x.clone().requires_grad_()
    Ac = A.clone().requires_grad_()
    asg_loss(xc, Ac, tg, xl, tl).sum().backward()
    assert not xc.grad.is_cuda and not Ac.grad.is_cuda
    check_grads(xc.grad.numpy(), want[1], 1e-9)
    check_slabs(Ac.grad.numpy(), want[2].sum(0), 1e-9)


@pytest.mark.parametrize("half", [torch.float16, torch.bfloat16])
def test_16bit_emissions_equal_their_f32_upcast(half):
    x, A, tg, xl, tl = make(3, 15, 9, 5, torch.float32, 73)
    xh = x.to(half)
    from end2end_amd.engines import ASGLossEngine
    eng = ASGLossEngine()
    got = eng.compute(xh.to(DEV), A.to(DEV), tg.to(DEV), xl.to(DEV), tl.to(DEV))
    up = eng.compute(xh.float().to(DEV), A.to(DEV), tg.to(DEV), xl.to(DEV), tl.to(DEV))
    assert got[0].dtype == half and got[1].dtype == half and got[2].dtype == torch.float32
    assert torch.equal(got[0], up[0].to(half)) and torch.equal(got[1], up[1].to(half)) and torch.equal(got[2], up[2])
    check_against_ref(tuple(t.double().cpu().numpy() for t in up), ref(xh.float(), A, tg, xl, tl), torch.float32)


def test_targets_beyond_the_limit_are_refused_with_the_limit():
    from end2end_amd import _C
    x, A, tg, xl, tl = make(1, 4, 3, 2, torch.float32, 74, ragged=False)
    wide = torch.zeros(1, _C.asg_max_target_length() + 1, dtype=torch.long)
    with pytest.raises(ValueError, match=str(_C.asg_max_target_length())):
        engine(x, A, wide, xl, tl)
    at_limit = engine(x, A, wide[:, :-1], xl, tl)                           # the width alone is no obstacle
    check_against_ref(at_limit, ref(x, A, wide[:, :-1], xl, tl), torch.float32)


# ---- range ----

@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_range(dt):
    dtype = DTYPES[dt]
    x, A, tg, xl, tl = make(4, 50, 9, 10, dtype, 81, xs=30.0, ts=5.0)
    check_all(x, A, tg, xl, tl)
    rng = np.random.default_rng(82)                                         # entries of -800 in both
    x2, A2 = x.clone(), A.clone()
    x2[torch.from_numpy(rng.random(x.shape) < 0.1)] = -800.0
    A2[torch.from_numpy(rng.random(A.shape) < 0.2)] = -800.0
    A2[int(tg[0, 1]), int(tg[0, 0])] = -800.0                               # and on an arc the first target has to take
    x2[1, 3, :] = -800.0                                                    # a whole frame
    want = ref(x2, A2, tg, xl, tl)
    assert np.isfinite(want[0]).all() and want[0][0] > 700
    check_all(x2, A2, tg, xl, tl)


# ---- invariances ----

def test_invariances():
    x, A, tg, xl, tl = make(4, 25, 7, 6, torch.float64, 91)
    base = engine(x, A, tg, xl, tl)
    moved = engine(x, A + 3.25, tg, xl, tl)
    assert np.max(np.abs(moved[0] - base[0])) <= 1e-9 and np.max(np.abs(moved[1] - base[1])) <= 1e-9
    shift = torch.from_numpy(np.random.default_rng(92).normal(size=(4, 25, 1)) * 4)
    moved = engine(x + shift, A, tg, xl, tl)
    assert np.max(np.abs(moved[0] - base[0])) <= 1e-9 and np.max(np.abs(moved[1] - base[1])) <= 1e-9
    assert np.max(np.abs(base[1].sum(-1))) <= 1e-9                          # rows: P_fcc and P_fal each sum to 1
    assert np.max(np.abs(base[2].sum((1, 2)))) <= 1e-9                      # slabs: both sum to n - 1


# ---- poisoning ----

@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_poisoned_utterances_poison_only_themselves(dt):
    dtype = DTYPES[dt]
    x, A, tg, xl, tl = make(6, 12, 5, 14, dtype, 101, ragged=False)
    xl[:] = torch.tensor([12, 10, 12, 12, 9, 12])
    tl[:] = torch.tensor([4, 11, 3, 5, 2, 6])                               # 1: more labels than frames
    xl[3] = 13                                                              # 3: x_len > T
    tg[5, 2] = 5                                                            # 5: a label == V
    got = engine(x, A, tg, xl, tl)
    check_against_ref(got, ref(x, A, tg, xl, tl), dtype)
    assert np.isinf(got[0][1]) and np.isnan(got[1][1, :10]).all() and (got[1][1, 10:] == 0).all() and np.isnan(got[2][1]).all()
    for b in (3, 5):
        assert np.isnan(got[0][b]) and np.isnan(got[1][b]).all() and np.isnan(got[2][b]).all()
    keep = [0, 2, 4]
    clean = engine(x[keep], A, tg[keep], xl[keep], tl[keep])
    for g, c in zip(got, clean):
        assert np.array_equal(g[keep], c)
    paths, scores, coll, lens = viterbi(x, A, xl)                           # the best path has no targets: only x_len counts
    assert (paths[3] == -100).all() and np.isnan(scores[3]) and lens[3] == 0 and (coll[3] == 0).all()
    want = AR.viterbi_ref(x.double().numpy(), A.double().numpy(), xl.numpy())
    assert np.array_equal(paths, want[0]) and np.array_equal(coll, want[2])


# ---- autograd ----

def test_gradcheck():
    from end2end_amd import asg_loss
    x, A, tg, xl, tl = make(2, 6, 4, 3, torch.float64, 111)
    xd, Ad = x.to(DEV).requires_grad_(), A.to(DEV).requires_grad_()
    tgd, xld, tld = tg.to(DEV), xl.to(DEV), tl.to(DEV)
    assert torch.autograd.gradcheck(lambda e, a: asg_loss(e, a, tgd, xld, tld), (xd, Ad), eps=1e-6, atol=1e-6, rtol=1e-6,
                                    nondet_tol=0.0)


def test_reduce_weights_retained_graph_and_optimiser_step():
    from end2end_amd import ASGLoss, asg_loss
    x, A, tg, xl, tl = make(5, 14, 6, 5, torch.float64, 112)
    want = ref(x, A, tg, xl, tl)
    dev = [t.to(DEV) for t in (tg, xl, tl)]
    mod = ASGLoss(6, reduce=False).to(DEV).double()
    red = ASGLoss(6, reduce=True).to(DEV).double()
    with torch.no_grad():
        mod.transitions.copy_(A.to(DEV))
        red.transitions.copy_(A.to(DEV))
    xd = x.to(DEV)
    vec = mod(xd, *dev)
    assert vec.shape == (5,) and torch.equal(red(xd, *dev), vec.sum())
    # weighted backward: sum_b w_b times the engine's slabs, for both gradients
    w = torch.from_numpy(np.random.default_rng(113).normal(size=5)).to(DEV)
    e = xd.clone().requires_grad_()
    loss = mod(e, *dev)
    (loss * w).sum().backward(retain_graph=True)
    wn = w.cpu().numpy()
    check_grads(e.grad.cpu().numpy(), want[1] * wn[:, None, None], 1e-9)
    check_slabs(mod.transitions.grad.cpu().numpy(), np.einsum("b,bji->ji", wn, want[2]), 1e-9)
    first = (e.grad.clone(), mod.transitions.grad.clone())
    e.grad = None
    mod.transitions.grad = None
    (loss * w).sum().backward()                                             # the retained graph walked again
    assert torch.equal(e.grad, first[0]) and torch.equal(mod.transitions.grad, first[1])
    # an optimiser step on the transitions changes the next loss
    opt = torch.optim.SGD([mod.transitions], lr=0.01)
    opt.zero_grad()
    before = mod(xd, *dev).sum()
    before.backward()
    opt.step()
    after = mod(xd, *dev).sum()
    assert float(after.detach()) < float(before.detach()) - 1e-6
    lf = asg_loss(xd, mod.transitions.detach(), *dev)
    assert torch.equal(lf.sum(), after)


# ---- determinism ----

def test_bit_identical_across_calls_and_streams():
    from end2end_amd.engines import ASGLossEngine
    inp, _ = long_case("f32")
    dev = [t.to(DEV) for t in inp]
    eng = ASGLossEngine()
    first = eng.compute(*dev)
    second = eng.compute(*dev)
    outs = []
    for _ in range(2):
        s = torch.cuda.Stream(DEV)
        s.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(s):
            outs.append(eng.compute(*dev))                                  # (a workspace per stream: nothing shared)
    torch.cuda.synchronize()
    for other in [second] + outs:
        for a, b in zip(first, other):
            assert torch.equal(a, b) or (torch.isnan(a) == torch.isnan(b)).all() and torch.equal(a.nan_to_num(), b.nan_to_num())


# ---- best path ----

def test_best_path_ties_go_to_the_lowest_label():
    for V in (3, 33, 128):
        x = torch.zeros(2, 9, V)
        paths, scores, coll, lens = viterbi(x, torch.zeros(V, V), torch.tensor([9, 5]))
        assert (paths[0] == 0).all() and (paths[1, :5] == 0).all() and (paths[1, 5:] == -100).all()
        assert (scores == 0).all() and (coll == 0).all() and lens.tolist() == [1, 1]
    # ties between parts of a row and between end states: equal maxima at labels 40 and 90 of 128
    V = 128
    x = torch.full((1, 4, V), -1.0, dtype=torch.float64)
    x[0, :, 40] = 0.0
    x[0, :, 90] = 0.0
    check_best_path(x, torch.zeros(V, V, dtype=torch.float64), torch.tensor([4]))
    assert viterbi(x, torch.zeros(V, V, dtype=torch.float64), torch.tensor([4]))[0][0].tolist() == [40] * 4


def test_best_path_equals_forced_alignment_on_one_hot_emissions():
    from end2end_amd.utils.alignment import get_alignment_3d
    V, T = 6, 14
    frames = [[2, 2, 2, 4, 4, 0, 0, 0, 0, 5, 1, 1, 3, 3], [1, 1, 1, 1, 3, 3, 0, 2, 2, 2, 2, 2, 0, 0]]
    xl = torch.tensor([14, 11])
    x = torch.full((2, T, V), -20.0)
    for b in range(2):
        for t in range(int(xl[b])):
            x[b, t, frames[b][t]] = 0.0
    paths, scores, coll, lens = check_best_path(x, torch.zeros(V, V), xl)
    for b in range(2):
        assert paths[b, :int(xl[b])].tolist() == frames[b][:int(xl[b])]
    lp = torch.log_softmax(x.double(), -1).float()
    al = get_alignment_3d(lp.to(DEV), torch.from_numpy(coll), xl, torch.from_numpy(lens), is_ctc=False)
    assert np.array_equal(al.numpy(), paths)


def test_decoder_sentences_and_path_results():
    from end2end_amd import ASGDecoder, ASGEncoder
    enc = ASGEncoder("abc ", num_replabels=2)                               # ids: a b c space <1> <2>
    V, T = enc.num_symbols, 12
    frames = [[4, 0, 0, 5, 5, 1, 1, 3, 2, 4, 4, 2], [1, 4, 4, 4, 0, 2, 2, 2, 5, 3, 3, 3]]
    xl = torch.tensor([12, 9])
    x = torch.full((2, T, V), -5.0)
    for b in range(2):
        for t in range(T):
            x[b, t, frames[b][t]] = 1.0
    rng = np.random.default_rng(121)
    A = torch.from_numpy(rng.normal(size=(V, V)) * 0.1).float()
    dec = ASGDecoder(labels=list("abc "), num_replabels=2)
    res = dec.decode(x.to(DEV), A.to(DEV), xl.to(DEV))
    path = dec.decode_path(x.to(DEV), A.to(DEV), xl.to(DEV))
    want = AR.viterbi_ref(x.double().numpy(), A.double().numpy(), xl.numpy())
    assert not res.decoded_targets.is_cuda and np.array_equal(path.paths.numpy(), want[0])
    assert np.array_equal(res.decoded_targets.numpy(), want[2]) and res.decoded_targets.shape == (2, T)
    assert res.decoded_targets_lengths.tolist() == want[3].tolist()
    assert np.allclose(path.scores.numpy(), want[1], rtol=1e-12, atol=0)
    for b in range(2):
        assert res.decoded_sentences[b] == enc.decode(path.paths[b].tolist())
    assert res.decoded_sentences[0] == "aaab ccc"                           # <1> leading: dropped; a <2>; b; space; c <1>; c
    tm = ASGDecoder(labels=list("abc "), num_replabels=2, time_major=True, keep_on_device=True)
    res2 = tm.decode(x.transpose(0, 1).to(DEV), A.to(DEV), xl.to(DEV))
    assert res2.decoded_targets.is_cuda and res2.decoded_sentences == res.decoded_sentences
    full = ASGDecoder(labels=list("abc ") + ["1", "2"], num_replabels=2).decode(x.to(DEV), A.to(DEV))
    assert full.decoded_sentences[0] == res.decoded_sentences[0] and full.decoded_targets_lengths[1] >= res.decoded_targets_lengths[1]
