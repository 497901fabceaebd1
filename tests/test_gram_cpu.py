"""CPU: Gram-CTC -- the test-side lattice against brute force over every path (pinning the definition independently of
the kernel), the constructor's checks, upstream's import surface and signatures, the C ABI's symbols and workspace."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import gram_ref as GR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lattice_equals_brute_force_on_tiny_random_cases():
    rng = np.random.default_rng(1234)
    n_inf = n_gram = 0
    for _ in range(240):
        R, V, l2i, x, tgt = GR.random_tiny_case(rng)
        grams = GR.grams_of(R, V, l2i)
        lp = x - np.log(np.sum(np.exp(x), axis=1, keepdims=True))
        bl, bp = GR.brute_force(lp, tgt, grams)
        ll, lpst = GR.lattice(lp, tgt, grams)
        if np.isinf(bl):
            n_inf += 1
            assert np.isinf(ll) and np.isnan(lpst).all()
            continue
        n_gram += bool(l2i)
        assert abs(ll - bl) <= 1e-10 * max(1.0, abs(bl)), (tgt, l2i, ll, bl)
        assert np.max(np.abs(lpst - bp)) <= 1e-10
    assert n_inf >= 10 and n_gram >= 100, (n_inf, n_gram)


def test_named_repeat_cases_against_brute_force():
    # "aaa" with the gram "aa": aa|a, a|aa, a|a|a (a blank between equal columns); "ll" "ll" with the gram "ll"
    for R, l2i, tgt in [(2, {2: [1, 1]}, [1, 1, 1]), (3, {3: [1, 1], 4: [1, 2]}, [1, 1, 1, 1]),
                        (3, {3: [2, 2]}, [2, 2, 2, 2]), (3, {3: [1, 2, 1]}, [1, 2, 1, 2, 1])]:
        V = R + len(l2i)
        grams = GR.grams_of(R, V, l2i)
        x = np.random.default_rng(len(tgt) + R).normal(size=(6 if V <= 4 else 5, V))
        lp = x - np.log(np.sum(np.exp(x), axis=1, keepdims=True))
        bl, bp = GR.brute_force(lp, tgt, grams)
        ll, lpst = GR.lattice(lp, tgt, grams)
        assert np.isfinite(bl) and abs(ll - bl) <= 1e-10 * abs(bl) and np.max(np.abs(lpst - bp)) <= 1e-10


def test_lattice_equals_brute_force_with_grams_of_order_4_to_8():
    # the orders the GPU tests trust gram_ref.lattice for: tiny tables (R = 2-3, V**T <= 4096) whose grams have 4..8 base
    # labels, overlapping ('aaaa' beside 'aaaaa', one gram a prefix of another), targets spelled from them with repeats
    rng = np.random.default_rng(48)
    n_fin = n_long = 0
    for case in range(120):
        R = int(rng.integers(2, 4))
        seqs = set()
        while len(seqs) < int(rng.integers(1, 4)):
            k = int(rng.integers(4, 9))
            g = tuple(int(v) for v in rng.integers(1, R, size=k))
            seqs |= {g, g[:-1]} if rng.random() < 0.3 and len(seqs) < 2 else {g}
        l2i = {R + i: list(s) for i, s in enumerate(sorted(seqs))}
        V = R + len(l2i)
        T = int(rng.integers(1, 8))
        while V ** T > 4096:
            T -= 1
        grams = GR.grams_of(R, V, l2i)
        tgt = []
        for _ in range(int(rng.integers(0, T + 2))):
            tgt += list(l2i[int(rng.choice(list(l2i)))]) if rng.random() < 0.7 else [int(rng.integers(1, R))]
        x = rng.normal(size=(T, V)) * float(rng.choice([0.5, 1.0, 3.0]))
        lp = x - np.log(np.sum(np.exp(x), axis=1, keepdims=True))
        bl, bp = GR.brute_force(lp, tgt, grams)
        ll, lpst = GR.lattice(lp, tgt, grams)
        if np.isinf(bl):
            assert np.isinf(ll) and ll > 0 and np.isnan(lpst).all(), (tgt, l2i, ll)
            continue
        n_fin += 1
        n_long += len(tgt) > T                       # (more labels than frames: only grams spell it)
        assert abs(ll - bl) <= 1e-10 * max(1.0, abs(bl)), (tgt, l2i, ll, bl)
        assert np.max(np.abs(lpst - bp)) <= 1e-10, (tgt, l2i)
    assert n_fin >= 50 and n_long >= 20, (n_fin, n_long)


@pytest.mark.parametrize("R", [2, 3])
def test_one_order_8_gram_spells_the_whole_target_in_one_frame(R):
    l2i = {R: [1] * 8, R + 1: [1] * 4} if R == 2 else {R: [1, 2, 2, 1, 2, 1, 1, 2], R + 1: [2, 2, 1]}
    grams = GR.grams_of(R, R + 2, l2i)
    lp = np.log(np.array([[0.1] * R + [0.5, 0.4 - 0.1 * (R - 1)]]))
    for tgt in (l2i[R], l2i[R] + [1]):
        bl, bp = GR.brute_force(lp, tgt, grams)
        ll, lpst = GR.lattice(lp, tgt, grams)
        if len(tgt) == 8:
            assert abs(bl + np.log(0.5)) < 1e-12 and bp[0, R] == 1.0      # the one path: the gram's column
            assert abs(ll - bl) <= 1e-12 and np.max(np.abs(lpst - bp)) <= 1e-12
        else:
            assert np.isinf(bl) and np.isinf(ll)                        # one label more: no path in one frame


def test_a_gram_needs_fewer_frames_than_ctc():
    # "aa" needs three frames under CTC (a, blank, a) but one with the gram "aa"
    grams = GR.grams_of(2, 3, {2: [1, 1]})
    lp = np.log(np.full((1, 3), 1.0 / 3))
    bl, _ = GR.brute_force(lp, [1, 1], grams)
    assert abs(bl - np.log(3.0)) < 1e-12
    assert np.isinf(GR.brute_force(np.log(np.full((2, 2), 0.5)), [1, 1], GR.grams_of(2, 2, {}))[0])


def test_constructor_rules():
    from end2end_amd import GramCTCLoss
    from end2end_amd.modules.ctc_loss import CTCLoss
    ok = dict(blank_idx=0, num_base_labels=4, total_labels=6, label2ids={4: [1, 2], 5: [2, 2, 3]})
    GramCTCLoss(**ok)
    GramCTCLoss(**dict(ok, label2ids={1: [1], 4: (1, 2), 5: [2, 2, 3]}))   # entries for c < R may be given as [c]
    GramCTCLoss(0, 4, 4, {})                                                   # unigrams only
    with pytest.raises(NotImplementedError):
        GramCTCLoss(**dict(ok, blank_idx=1))
    bad = [
        dict(label2ids={4: [1, 2]}),                              # column 5 has no entry
        dict(label2ids={2: [3], 4: [1, 2], 5: [2, 2, 3]}),        # an entry for c < R is not [c]
        dict(label2ids={0: [1], 4: [1, 2], 5: [2, 2, 3]}),        # key 0
        dict(label2ids={4: [1, 2], 5: [2, 2, 3], 6: [1, 3]}),     # key out of range
        dict(label2ids={4: [1, 2], 5: [2, 0]}),                   # id 0
        dict(label2ids={4: [1, 2], 5: [2, 4]}),                   # id >= R
        dict(label2ids={4: [1, 2], 5: [1, 2]}),                   # two columns spell the same gram
        dict(label2ids={4: [1, 2], 5: [3]}),                      # a gram column spelling a unigram
        dict(label2ids={4: [1, 2], 5: []}),                       # empty gram
        dict(label2ids={4: [1, 2], 5: [1] * 9}),                  # longer than 8
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            GramCTCLoss(**dict(ok, **kw))
    with pytest.raises(ValueError):                               # R ** max_order overflows int64
        GramCTCLoss(0, 300, 301, {300: [1] * 8})
    assert issubclass(GramCTCLoss, CTCLoss)


def test_width_check_before_any_gpu_call():
    import torch
    from end2end_amd.engines import GramCTCLossEngine
    eng = GramCTCLossEngine(0, 4, 6, {4: [1, 2], 5: [2, 2, 3]})
    with pytest.raises(ValueError, match="columns"):
        eng.compute(torch.zeros(1, 3, 5), torch.ones(1, 1, dtype=torch.long), torch.tensor([3]), torch.tensor([1]))


def test_import_surface_and_signatures_match_upstream():
    import cpp_gram_ctc_loss
    import end2end_amd
    import pytorch_end2end
    from pytorch_end2end.modules.ctc_loss import CTCLoss, GramCTCLoss
    assert pytorch_end2end.__all__ == ["CTCLoss", "CTCDecoder", "CTCEncoder"]
    assert end2end_amd.GramCTCLoss is GramCTCLoss and "GramCTCLoss" in end2end_amd.__all__
    assert issubclass(GramCTCLoss, CTCLoss)
    params = inspect.signature(cpp_gram_ctc_loss.GramCTCLossEngine.__init__).parameters
    assert list(params) == ["self", "blank_idx", "num_base_labels", "total_labels", "label2ids"]
    comp = inspect.signature(cpp_gram_ctc_loss.GramCTCLossEngine.compute).parameters
    assert list(comp)[:5] == ["self", "logits", "targets", "logits_lengths", "targets_lengths"]
    params = inspect.signature(GramCTCLoss.__init__).parameters
    assert [(k, v.default) for k, v in params.items()][:9] == [
        ("self", inspect.Parameter.empty), ("blank_idx", inspect.Parameter.empty),
        ("num_base_labels", inspect.Parameter.empty), ("total_labels", inspect.Parameter.empty),
        ("label2ids", inspect.Parameter.empty), ("size_average", None), ("reduce", None),
        ("after_logsoftmax", False), ("time_major", False)]


def test_binding_rejects_bad_arguments_before_any_gpu_call():
    from end2end_amd import _C
    args = dict(x=0, input_is_logprobs=True, sB=0, sT=0, sV=0, targets=0, tgt_stride=1, x_len=0, t_len=0, B=1, T=4,
                V=5, Smax=2, keys=0, cols=0, n_grams=0, losses=0, grads=0, workspace=0, workspace_bytes=0, stream=0)
    with pytest.raises(ValueError, match="dtype"):
        _C.gram_ctc_fwd_bwd(dtype=_C.F16, radix=3, max_order=2, **args)
    for r in (0, 6):
        with pytest.raises(ValueError, match="radix"):
            _C.gram_ctc_fwd_bwd(dtype=_C.F32, radix=r, max_order=2, **args)
    for m in (0, 9):
        with pytest.raises(ValueError, match="max_order"):
            _C.gram_ctc_fwd_bwd(dtype=_C.F32, radix=3, max_order=m, **args)
    with pytest.raises(ValueError, match="table"):
        _C.gram_ctc_fwd_bwd(dtype=_C.F32, radix=3, max_order=2, **dict(args, n_grams=3))


def test_library_exports_and_header_declares_the_new_entry_points():
    from end2end_amd import _lib
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "e2e_ctc.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for sym in ("e2e_gram_ctc_workspace_bytes", "e2e_gram_ctc_fwd_bwd"):
        assert re.search(r"\b%s\s*\(" % sym, hdr) and hasattr(L, sym) and re.search(r" T %s$" % sym, out, re.M)
    assert L.e2e_ctc_abi_version() == 4 == _lib.ABI_VERSION
    assert re.search(r"#define E2E_CTC_ABI_VERSION 4\b", hdr)


def test_workspace_of_the_headline_shape_stays_under_128_megabytes():
    from end2end_amd import _lib
    L = _lib.load()
    n = L.e2e_gram_ctc_workspace_bytes(256, 1000, 379, 200, 3, _lib.F32)
    assert 0 < n <= 128e6, n


def test_documented_capacity():
    # include/e2e_ctc.h: Smax <= 668 at max_order 3 (>= 500 required), and the workspace query is 0 beyond
    from end2end_amd import _lib
    from end2end_amd.engines import GramCTCLossEngine
    L = _lib.load()
    for order, limit in [(1, 1316), (2, 887), (3, 668), (4, 536), (8, 299)]:
        assert L.e2e_gram_ctc_workspace_bytes(2, 100, 400, limit, order, _lib.F32) > 0
        assert L.e2e_gram_ctc_workspace_bytes(2, 100, 400, limit + 1, order, _lib.F32) == 0
    assert GramCTCLossEngine(0, 29, 30, {29: [1, 2, 3]}).max_target_length() == 668 >= 500
