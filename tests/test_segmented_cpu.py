"""CPU: word-segmented CTC -- the test-side restatement against upstream's own results (tests/golden/segmented.npz), the
import surface and defaults of upstream, the C ABI's symbols, the host-side grouping rule and the argument checks that
need no device."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import golden_util as G
import segmented_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = G.npz("segmented.npz")
CASES = sorted({k.split("/")[0] for k in FIX.files})


def case(name):
    return {k.split("/", 1)[1]: FIX[k] for k in FIX.files if k.split("/")[0] == name}


def upstream_logp(c):
    """The log-softmax as upstream takes it: in f32."""
    return torch.log_softmax(torch.from_numpy(c["logits"]), 2).double().numpy()


def ref_segments(c):
    """The restatement's segments of a golden case, aligned as upstream aligns: Viterbi on the f32 log-softmax."""
    a = SR.alignment(upstream_logp(c), c["targets"], c["x_len"], c["t_len"], blank=0)
    return SR.plan(c["logits"], a, c["targets"], c["x_len"], c["t_len"], int(c["space_idx"]), 0, int(c["min_word_length"]))


def golden_segments(c):
    return [(int(c["seg_utt"][i]), int(c["seg_start"][i]), int(c["seg_x_len"][i]),
             [int(v) for v in c["seg_targets"][i, :c["seg_t_len"][i]]]) for i in range(len(c["seg_utt"]))]


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_upstream(name):
    c = case(name)
    segs = ref_segments(c)
    assert [(b, s, n, tg) for b, s, n, _, tg in segs] == golden_segments(c)
    # a segmented utterance has no whole segment, an unsegmented one nothing else
    per_utt = {}
    for b, _, _, kind, _ in segs:
        per_utt.setdefault(b, []).append(kind)
    assert all(kinds == [SR.WHOLE] or SR.WHOLE not in kinds for kinds in per_utt.values())
    loss, grad = SR.losses_and_grads(c["logits"], segs, 0, logp=upstream_logp(c))
    assert np.allclose(loss, c["losses"], rtol=1e-6, atol=0), (loss, c["losses"])      # (upstream rounds f64 results to f32 once)
    assert np.max(np.abs(grad - c["grad"])) <= 2e-6


def test_fixture_has_what_the_issue_asks_for():
    assert 25 <= len(CASES) <= 40
    cut = [n for n in CASES if len(case(n)["seg_utt"]) > len(case(n)["x_len"])]
    assert len(cut) >= 20
    assert {int(case(n)["min_word_length"]) for n in CASES} == {0, 1, 2, 3}
    for n in CASES:
        B, T, V = case(n)["logits"].shape
        assert B <= 4 and T <= 48 and V <= 7
    assert os.path.getsize(os.path.join(G.GOLDEN, "segmented.npz")) < 256 * 1024


def test_boundaries_where_upstream_raises_are_defined():
    # a qualifying space on the last frame; a first boundary at frame 1: the built list is the definition
    a = [2, 3, 4, 1]
    assert SR.boundaries(a, a, 4, space=1, blank=0, min_word_length=3) == [0, 3]
    a = [1, 1, 2, 3, 4, 1, 2]
    assert SR.boundaries(a, a, 7, space=1, blank=0, min_word_length=0) == [0, 1, 5, 6]
    segs = SR.segments(np.array([a]), np.array([a]), np.array([[1, 2, 3, 4, 1, 2]]), [7], [6], 5, 1, 0, 0)
    assert [(s, n, k) for _, s, n, k, _ in segs] == [(0, 1, SR.CHUNK), (1, 1, SR.FRAME), (2, 3, SR.CHUNK), (5, 1, SR.FRAME), (6, 1, SR.CHUNK)]
    assert sum(n for _, _, n, _, _ in segs) == 7


def test_module_imports_under_both_names_with_upstream_defaults():
    from pytorch_end2end.modules.ctc_loss_segmented import CTCLossSegmented as A
    from end2end_amd.modules.ctc_loss_segmented import CTCLossSegmented as B
    import end2end_amd
    assert A is B is end2end_amd.CTCLossSegmented
    params = inspect.signature(A.__init__).parameters
    assert [(k, v.default) for k, v in params.items()] == [
        ("self", inspect.Parameter.empty), ("space_idx", inspect.Parameter.empty), ("blank_idx", 0), ("reduce", False),
        ("min_word_length", 3)]
    assert list(inspect.signature(A.forward).parameters) == ["self", "logits", "targets", "logits_lengths", "targets_lengths"]
    from end2end_amd.utils.segmentation import word_segments
    params = inspect.signature(word_segments).parameters
    assert [(k, v.default) for k, v in params.items()][4:] == [("space_idx", inspect.Parameter.empty), ("blank_idx", 0),
                                                              ("min_word_length", 3)]
    doc = inspect.getdoc(inspect.getmodule(A))
    assert "only synchronisation" in doc and "Deliberate differences" in doc


def test_library_exports_and_header_declares_the_new_entry_points():
    from end2end_amd import _C, _lib
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "e2e_ctc.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for sym in ("e2e_ctc_wordseg_table_elems", "e2e_ctc_wordseg_workspace_bytes", "e2e_ctc_wordseg_plan",
                "e2e_ctc_wordseg_gather", "e2e_ctc_wordseg_finish"):
        assert re.search(r"\b%s\s*\(" % sym, hdr) and hasattr(L, sym) and re.search(r" T %s$" % sym, out, re.M), sym
    assert L.e2e_ctc_abi_version() == 4 == _lib.ABI_VERSION
    assert "#define E2E_CTC_ABI_VERSION 4" in hdr
    assert _C.ctc_wordseg_table_elems(256, 1000) == 16 + 257 + 5 * 256000
    assert 0 < _C.ctc_wordseg_workspace_bytes(256, 1000) <= 27 * 256000
    assert (_C.WORDSEG_WHOLE, _C.WORDSEG_FRAME, _C.WORDSEG_CHUNK) == (SR.WHOLE, SR.FRAME, SR.CHUNK)


def test_binding_rejects_bad_arguments_before_any_gpu_call():
    from end2end_amd import _C
    plan = dict(x=0, sB=0, sT=0, sV=0, align=0, targets=0, tgt_stride=1, x_len=0, t_len=0, B=1, T=4, V=5, Smax=2,
                min_word_length=3, table=0, table_elems=0, pool=0, workspace=0, workspace_bytes=0, stream=0)
    with pytest.raises(_C.E2EError, match="dtype"):
        _C.ctc_wordseg_plan(dtype=_C.F16, blank=0, space=1, **plan)
    with pytest.raises(_C.E2EError, match="space"):
        _C.ctc_wordseg_plan(dtype=_C.F32, blank=0, space=5, **plan)
    with pytest.raises(_C.E2EError, match="blank"):
        _C.ctc_wordseg_plan(dtype=_C.F32, blank=-1, space=1, **plan)
    with pytest.raises(_C.E2EError, match="table"):
        _C.ctc_wordseg_plan(dtype=_C.F32, blank=0, space=1, **plan)
    gather = dict(x=0, dtype=_C.F32, sB=0, sT=0, sV=0, targets=0, tgt_stride=1, x_len=0, t_len=0, B=1, T=4, V=5, Smax=2,
                  table=0, pool=0, idx=0, xg=0, tg=0, xlg=0, tlg=0, stream=0)
    with pytest.raises(_C.E2EError, match="L=5"):
        _C.ctc_wordseg_gather(n_idx=1, L=5, S=1, **gather)
    with pytest.raises(_C.E2EError, match="null"):
        _C.ctc_wordseg_gather(n_idx=1, L=4, S=1, **gather)
    with pytest.raises(_C.E2EError, match="null"):
        _C.ctc_wordseg_finish(x=0, dtype=_C.F32, sB=0, sT=0, sV=0, align=0, B=1, T=4, V=5, table=0, g_grads=0, g_losses=0,
                              g_idx=0, n_idx=0, L=1, last=True, losses=0, grads=0, workspace=0, workspace_bytes=0, stream=0)


def test_python_layer_checks_its_arguments_without_a_device():
    from end2end_amd import CTCLossSegmented
    x = torch.randn(2, 6, 4)
    tg, xl, tl = torch.tensor([[1, 2], [2, 3]]), torch.tensor([6, 5]), torch.tensor([2, 2])
    with pytest.raises(ValueError, match="space_idx"):
        CTCLossSegmented(space_idx=4)(x, tg, xl, tl)
    with pytest.raises(ValueError, match="blank_idx"):
        CTCLossSegmented(space_idx=1, blank_idx=-1)(x, tg, xl, tl)
    with pytest.raises(ValueError, match="batch, time, alphabet"):
        CTCLossSegmented(space_idx=1)(x[0], tg, xl, tl)
    with pytest.raises(ValueError, match="targets"):
        CTCLossSegmented(space_idx=1)(x, tg[:1], xl, tl)
    with pytest.raises(ValueError, match="lengths"):
        CTCLossSegmented(space_idx=1)(x, tg, xl[:1], tl)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            CTCLossSegmented(space_idx=1)(x, tg, xl, tl)


def test_groups_stay_within_the_budget_and_hold_every_segment_once():
    from end2end_amd.utils.segmentation import plan_groups
    rng = np.random.default_rng(0)
    lists = [[], [7], [300, 5, 5, 5], [3] * 40 + [25, 25, 130, 300], list(rng.integers(1, 1001, 500)), [1000] * 9,
             list(rng.integers(1, 30, 2000)) + [1000]]
    budgets = [1, 600, 600, 600, 256 * 1000, 4000, 2000]
    for lengths, budget in zip(lists, budgets):
        groups = plan_groups(lengths, budget)
        flat = np.concatenate(groups) if groups else np.zeros(0, dtype=np.int64)
        assert sorted(flat.tolist()) == list(range(len(lengths)))
        lens = np.asarray(lengths, dtype=np.int64)
        assert all(np.all(np.diff(lens[flat]) >= 0) for _ in [0])          # consecutive runs of the sorted list
        for g in groups:
            assert len(g) * int(lens[g].max()) <= budget or len(g) == 1
    # many short words beside one unsegmented utterance: not segments * T frames
    groups = plan_groups([3] * 40 + [25, 25, 130, 300], 600)
    assert [len(g) for g in groups] == [40, 3, 1]
