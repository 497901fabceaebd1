"""CPU: ASG -- the encoder's repeat labels, the test-side restatement (tests/asg_ref.py) against its own brute force, the
host-only part of the C ABI (limits, workspace queries, construction checks) and the names under pytorch_end2end."""
import random

import numpy as np
import pytest

import asg_ref as AR


# ---- 1. encoder ----

def test_encoder_examples_and_ids():
    from end2end_amd import ASGEncoder
    e = ASGEncoder()                                    # " " + a..z + "'", R = 2
    assert e.num_symbols == 28 + 2 and e.num_replabels == 2
    ids = {ch: i for i, ch in enumerate(" abcdefghijklmnopqrstuvwxyz'")}
    r1, r2 = 28, 29
    assert e.encode("hello").tolist() == [ids["h"], ids["e"], ids["l"], r1, ids["o"]]
    assert e.encode("aaaa").tolist() == [ids["a"], r2, ids["a"]]
    assert e.encode("HeLLo, World!").tolist() == e.encode("hello world").tolist()
    assert e.clean("HeLLo, World!") == "hello world"
    assert e.decode([ids["h"], ids["h"], ids["e"], ids["l"], ids["l"], r1, r1, ids["o"]]) == "hello"   # a frame path
    assert e.decode([r1, ids["a"], r2]) == "aaa"        # a leading repeat label is dropped
    assert e.decode_pure([ids["l"], r1, ids["o"]]) == "l1o"
    e1 = ASGEncoder("ab", num_replabels=1)
    assert e1.num_symbols == 3 and e1.encode("aaab").tolist() == [0, 2, 0, 1]


@pytest.mark.parametrize("R", [0, 1, 2, 3])
def test_encoder_round_trip_on_random_runs(R):
    from end2end_amd import ASGEncoder
    e = ASGEncoder("abc '", num_replabels=R)
    rng = random.Random(100 + R)
    for _ in range(200):
        s = "".join(rng.choice("abc 'XZ") * rng.randint(1, 7) for _ in range(rng.randint(0, 8)))
        ids = e.encode(s).tolist()
        assert e.decode(ids) == e.clean(s), (s, ids)
        if R >= 1:
            assert all(a != b for a, b in zip(ids, ids[1:])), (s, ids)
            assert e.clean(s) == "".join(ch for ch in s.casefold() if ch in "abc '")
        assert all(0 <= i < e.num_symbols for i in ids)


# ---- 2. the restatement against its brute force ----

REF_CASES = [(1, 3, [0, 0]), (2, 4, [0, 1, 0]), (3, 4, [1, 1, 2]), (3, 1, [2])]


def _inputs(V, n, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(1, n, V)) * 1.5, rng.normal(size=(V, V))


@pytest.mark.parametrize("V,n,y", REF_CASES)
def test_restatement_equals_enumeration(V, n, y):
    x, A = _inputs(V, n, 7 * V + n)
    tg = np.array([y])
    loss, grads, tgrads = AR.asg_ref(x, A, tg, [n], [len(y)])
    assert abs(loss[0] - AR.brute_loss(x[0], A, y)) <= 1e-13
    if all(a != b for a, b in zip(y, y[1:])):           # (a repeated label is counted once per alignment k: FAL can pass FCC)
        assert loss[0] >= -1e-13
    h = 1e-5
    for t in range(n):                                  # both gradients by central differences of the enumeration
        for v in range(V):
            xp, xm = x.copy(), x.copy()
            xp[0, t, v] += h
            xm[0, t, v] -= h
            fd = (AR.brute_loss(xp[0], A, y) - AR.brute_loss(xm[0], A, y)) / (2 * h)
            assert abs(fd - grads[0, t, v]) <= 1e-8, (t, v)
    for j in range(V):
        for i in range(V):
            Ap, Am = A.copy(), A.copy()
            Ap[j, i] += h
            Am[j, i] -= h
            fd = (AR.brute_loss(x[0], Ap, y) - AR.brute_loss(x[0], Am, y)) / (2 * h)
            assert abs(fd - tgrads[0, j, i]) <= 1e-8, (j, i)
    if n == 1:
        assert (tgrads == 0).all()


def test_restatement_edge_cases_and_viterbi():
    x, A = _inputs(3, 4, 5)
    x = np.repeat(x, 4, axis=0)
    tg = np.array([[0, 1, 2, 0, 1], [0, 1, 0, 0, 0], [0, 3, 0, 0, 0], [0, 1, 0, 0, 0]])
    loss, g, tgr = AR.asg_ref(x, A, tg, [4, 5, 4, 4], [5, 2, 2, 2])
    assert np.isinf(loss[0]) and np.isnan(g[0]).all() and np.isnan(tgr[0]).all()          # n < s
    assert np.isnan(loss[1]) and np.isnan(loss[2]) and np.isfinite(loss[3])               # bad length, bad label
    assert np.isfinite(g[3]).all() and abs(g[3].sum(axis=1)).max() <= 1e-12 and abs(tgr[3].sum()) <= 1e-12
    # best path: brute force over all paths, first maximum in lexicographic order of the reversed path is not defined
    # here -- random inputs have no ties
    paths, scores, coll, lens = AR.viterbi_ref(x[:1], A, [4])
    import itertools
    best = max(itertools.product(range(3), repeat=4), key=lambda pi: AR.path_score(x[0], A, pi))
    assert paths[0].tolist() == list(best) and abs(scores[0] - AR.path_score(x[0], A, best)) <= 1e-12
    z = np.zeros((1, 5, 3))
    p0, s0, c0, l0 = AR.viterbi_ref(z, np.zeros((3, 3)), [4])
    assert p0[0].tolist() == [0, 0, 0, 0, -100] and s0[0] == 0 and c0[0].tolist() == [0] * 5 and l0[0] == 1


# ---- 3. host-only ABI ----

def test_limits_and_workspace_queries():
    from end2end_amd import _C, _lib
    L = _lib.load()
    assert L.e2e_asg_max_labels() == _C.asg_max_labels() == 128
    assert L.e2e_asg_max_target_length() == _C.asg_max_target_length() == 512
    for dt in (_C.F32, _C.F64):
        assert L.e2e_asg_workspace_bytes(4, 100, 129, 10, dt) == 0
        assert L.e2e_asg_workspace_bytes(4, 100, 29, 513, dt) == 0
        assert L.e2e_asg_workspace_bytes(4, 100, 0, 10, dt) == 0
        assert L.e2e_asg_workspace_bytes(4, 100, 128, 512, dt) > 8 * 4 * 100 * (128 + 512)
        assert _C.asg_workspace_bytes(4, 100, 128, 512, dt) == L.e2e_asg_workspace_bytes(4, 100, 128, 512, dt)
    assert L.e2e_asg_viterbi_workspace_bytes(4, 100, 129) == 0
    assert L.e2e_asg_viterbi_workspace_bytes(4, 100, 128) >= 4 * 100 * 128
    # the headline shape, as the header states it
    assert abs(L.e2e_asg_workspace_bytes(256, 1000, 29, 200, _C.F32) / 1e6 - 471) < 1


def test_calls_outside_the_limits_are_refused_before_any_gpu_work():
    from end2end_amd import _C, _lib
    L = _lib.load()
    one = 1                                             # (non-null addresses: the argument checks come first)
    rc = L.e2e_asg_fwd_bwd(one, _C.F32, 1, 1, 1, one, one, 1, one, one, 1, 4, 129, 2, one, one, one, one, 1 << 20, None, None)
    assert rc == _C.ERR_UNSUPPORTED and b"128" in L.e2e_last_error()
    rc = L.e2e_asg_fwd_bwd(one, _C.F32, 1, 1, 1, one, one, 1, one, one, 1, 4, 29, 513, one, one, one, one, 1 << 20, None, None)
    assert rc == _C.ERR_UNSUPPORTED and b"512" in L.e2e_last_error()
    opts = _lib.LossOpts(1.0, one, _lib.REDUCE_SUM, 0)
    import ctypes
    rc = L.e2e_asg_fwd_bwd(one, _C.F32, 1, 1, 1, one, one, 1, one, one, 1, 4, 29, 2, one, one, one, one, 1 << 20, None,
                           ctypes.byref(opts))
    assert rc == _C.ERR_UNSUPPORTED
    rc = L.e2e_asg_viterbi(one, _C.F32, 1, 1, 1, one, one, 1, 4, 129, one, -100, one, one, one, one, 1 << 20, None)
    assert rc == _C.ERR_UNSUPPORTED
    rc = L.e2e_asg_fwd_bwd(one, _C.F16, 1, 1, 1, one, one, 1, one, one, 1, 4, 29, 2, one, one, one, one, 1 << 20, None, None)
    assert rc == -1                                     # E2E_ERR_ARG: 16-bit inputs are up-cast by the caller


def test_python_classes_state_the_limit():
    import torch
    from end2end_amd import ASGLoss
    from end2end_amd.engines import ASGLossEngine, ASGViterbiEngine
    with pytest.raises(ValueError, match="128"):
        ASGLoss(129)
    with pytest.raises(ValueError, match="128"):
        ASGLossEngine(0)
    m = ASGLoss(5)
    assert tuple(m.transitions.shape) == (5, 5) and m.transitions.requires_grad and float(m.transitions.detach().abs().sum()) == 0
    import copy
    import pickle
    m2 = pickle.loads(pickle.dumps(copy.deepcopy(m)))   # a module with its engine copies and pickles, as the other losses do
    assert tuple(m2.transitions.shape) == (5, 5)
    with pytest.raises(ValueError, match="128"):        # at the call, before a GPU is asked for
        ASGLossEngine().compute(torch.zeros(1, 3, 129), torch.zeros(129, 129), torch.zeros(1, 2, dtype=torch.long), [3], [2])
    with pytest.raises(ValueError, match="128"):
        ASGViterbiEngine().compute(torch.zeros(1, 3, 129), torch.zeros(129, 129), [3])
    with pytest.raises(ValueError, match="columns"):
        m(torch.zeros(1, 3, 6), torch.zeros(1, 2, dtype=torch.long), torch.tensor([3]), torch.tensor([2]))


# ---- 4. names ----

def test_names_resolve_under_upstreams_package():
    import inspect
    import string
    import end2end_amd
    import pytorch_end2end.decoders
    import pytorch_end2end.encoders
    import pytorch_end2end.modules.asg_loss
    assert pytorch_end2end.encoders.ASGEncoder is end2end_amd.ASGEncoder
    from pytorch_end2end.encoders.text_encoders import ASGEncoder
    assert ASGEncoder is end2end_amd.ASGEncoder
    assert pytorch_end2end.modules.asg_loss.ASGLoss is end2end_amd.ASGLoss
    assert pytorch_end2end.modules.asg_loss.asg_loss is end2end_amd.asg_loss
    assert pytorch_end2end.decoders.ASGDecoder is end2end_amd.ASGDecoder
    params = inspect.signature(ASGEncoder.__init__).parameters
    assert [(k, v.default) for k, v in params.items()][1:] == [
        ("allowed_chars", " " + string.ascii_lowercase + "'"), ("to_lower", str.casefold), ("num_replabels", 2)]
    params = inspect.signature(end2end_amd.ASGLoss.__init__).parameters
    assert [(k, v.default) for k, v in params.items()][1:] == [
        ("num_labels", inspect.Parameter.empty), ("reduce", True), ("time_major", False)]
    assert list(inspect.signature(end2end_amd.ASGLoss.forward).parameters) == list(
        inspect.signature(end2end_amd.CTCWithoutBlankLoss.forward).parameters)
    params = inspect.signature(end2end_amd.ASGDecoder.__init__).parameters
    assert [(k, v.default) for k, v in params.items()][1:] == [
        ("labels", None), ("num_replabels", 0), ("time_major", False), ("keep_on_device", False)]
