"""GPU: the selection kernel alone (e2e_ctc_label_cut, end2end_amd.utils.label_cut) against the numpy restatement of the
definition (tests/label_cut_ref.py): ids and counts with np.array_equal.

Per alphabet width V in label_cut_ref.CUT_V (a wave per frame up to 256 columns, a workgroup beyond; rows kept in LDS up to
8192 columns of f32) and input dtype: every cutoff_top_n of cut_top_ns(V) with every cutoff_prob of CUT_PROBS, the blank at 0,
at V - 1 or at a column that is never among the top, the input contiguous, a (T,B,V) view or a view with sV = 2, ragged
lengths with 0 and 1.  The first frames of utterance 0 are the edges: an all-equal row, a one-hot row, rows of bit-equal
columns straddling every place, -inf columns, a NaN.  A frame within label_cut_ref.BOUNDARY of cutoff_prob is not compared
(LEFT_OUT_FRAMES: 5 of some 7 000 for f32 and for f64, none for the 16-bit types, none at cutoff_prob = 1;
tests/test_label_cut_cpu.py recomputes them)."""
import numpy as np
import pytest
import torch

import label_cut_ref as LC

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
DTYPES = {"f32": torch.float32, "f64": torch.float64, "f16": torch.float16, "bf16": torch.bfloat16}


def viewed(x, view):
    """x (B,T,V) on the GPU as the combination's view."""
    x = x.to(DEV)
    if view == "time_major":
        return x.permute(1, 0, 2).contiguous().permute(1, 0, 2)
    if view == "strided":
        wide = torch.zeros(x.shape[:2] + (2 * x.shape[2],), dtype=x.dtype, device=DEV)
        wide[:, :, ::2] = x
        return wide[:, :, ::2]
    return x.contiguous()


@pytest.mark.parametrize("dtype", LC.CUT_DTYPES)
@pytest.mark.parametrize("V", LC.CUT_V)
def test_selection_equals_the_definition(V, dtype):
    from end2end_amd.utils import label_cut
    left_out = set(LC.LEFT_OUT_FRAMES.get((V, dtype), ()))
    views = set()
    for top_n in LC.cut_top_ns(V):
        for prob in LC.CUT_PROBS:
            c = LC.cut_case(V, dtype, top_n, prob)
            x = viewed(torch.from_numpy(c.lp).to(DTYPES[dtype]), c.view)
            views.add((c.view, x.stride(2)))
            ids, n = label_cut(x, torch.tensor(c.lens), cutoff_top_n=top_n, cutoff_prob=prob, blank_idx=c.blank)
            ids, n = ids.numpy(), n.numpy()
            assert ids.dtype == np.int32 and n.dtype == np.int32 and ids.shape == c.ids.shape and n.shape == c.n.shape
            want_ids, want_n = c.ids.copy(), c.n.copy()
            for (tn, pr, b, t) in left_out:
                if (tn, pr) == (top_n, prob):                            # not compared: both sides take the restatement's
                    ids[b, t], n[b, t] = want_ids[b, t], want_n[b, t]
            assert np.array_equal(n, want_n), (V, dtype, top_n, prob, np.argwhere(n != want_n)[:4].tolist())
            assert np.array_equal(ids, want_ids), (V, dtype, top_n, prob, np.argwhere(ids != want_ids)[:4].tolist())
            assert int((c.margin < LC.BOUNDARY).sum()) == sum(1 for o in left_out if o[:2] == (top_n, prob))
    assert {v for v, _ in views} == set(LC.CUT_VIEWS) and ("strided", 2) in views


@pytest.mark.parametrize("V", (29, 1000, 8000))
def test_two_calls_give_identical_bytes_and_the_device_results_stay(V):
    from end2end_amd.utils import label_cut
    lp, lens = LC.cut_input(V, "f32")
    x = torch.from_numpy(lp).to(DEV)
    a = label_cut(x, torch.tensor(lens), cutoff_top_n=40, cutoff_prob=0.99, keep_on_device=True)
    b = label_cut(x, torch.tensor(lens).to(DEV), cutoff_top_n=40, cutoff_prob=0.99, keep_on_device=True)
    assert a[0].is_cuda and a[1].is_cuda
    assert a[0].cpu().numpy().tobytes() == b[0].cpu().numpy().tobytes()
    assert a[1].cpu().numpy().tobytes() == b[1].cpu().numpy().tobytes()
    # lengths default to every frame; cutoff_top_n defaults to the alphabet
    ids, n = label_cut(x[:, :4, :29], cutoff_prob=0.9)
    assert ids.shape == (x.shape[0], 4, 30) and (n.numpy() >= 1).all()


def test_argument_errors_reach_python():
    from end2end_amd import _C
    from end2end_amd.utils import label_cut
    x = torch.zeros(1, 2, 5, device=DEV)
    for kw in (dict(cutoff_top_n=0), dict(cutoff_prob=0.0), dict(cutoff_prob=1.1), dict(blank_idx=5)):
        with pytest.raises(_C.E2EError):
            label_cut(x, **kw)
    with pytest.raises(_C.E2EError, match="at most 1024"):
        label_cut(torch.zeros(1, 1, 2000, device=DEV), cutoff_top_n=1500)
