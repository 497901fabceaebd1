"""CPU: CTC without blank and the aligned-targets loss -- the test-side restatement against the reference's fixtures,
the import surface and signatures of upstream, argument checks of the binding, the C ABI's symbols and workspace."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import noblank_ref as NR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = np.load(os.path.join(ROOT, "tests", "golden", "noblank.npz"))
CASES = sorted({k.split("/")[0] for k in FIX.files if not k.startswith("aligned")})


def case(name):
    return {k.split("/", 1)[1]: FIX[k] for k in FIX.files if k.split("/")[0] == name}


def logprobs(c):
    x = torch.from_numpy(c["logits"]).double()
    return (torch.log(x) if int(c["after_softmax"]) else torch.log_softmax(x, -1)).numpy()


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_reference_fixtures(name):
    c = case(name)
    loss, grad = NR.noblank_loss_grad(logprobs(c), c["targets"], c["x_len"], c["t_len"], int(c["space_idx"]))
    want_l, want_g = c["eng_loss"], c["eng_grad"]
    assert np.array_equal(np.isinf(loss), np.isinf(want_l)) and np.array_equal(np.isnan(loss), np.isnan(want_l))
    fin = np.isfinite(want_l)
    assert np.all(np.abs(loss[fin] - want_l[fin]) <= 1e-12 * np.abs(want_l[fin]))
    assert np.array_equal(np.isnan(grad), np.isnan(want_g))
    ok = ~np.isnan(want_g)
    assert np.max(np.abs(grad[ok] - want_g[ok]), initial=0.0) <= 1e-10


def test_fixtures_cover_the_issue_cases():
    spaces = {int(case(n)["space_idx"]) for n in CASES}
    assert {-1, 2, 5} <= spaces
    assert any(np.isinf(case(n)["eng_loss"]).any() for n in CASES)
    assert case("q10_empty")["t_len"].min() == 0 and case("t1_space")["logits"].shape[1] == 1
    assert case("f64")["logits"].dtype == np.float64


def test_import_surface_and_signatures_match_upstream():
    from pytorch_end2end.functions.ctc_without_blank import CTCWithoutBlankLossFunction
    from pytorch_end2end.modules.alignment_loss import AlignedTargetsLoss
    from pytorch_end2end.modules.ctc_without_blank import CTCWithoutBlankLoss
    import end2end_amd
    import pytorch_end2end
    assert pytorch_end2end.__all__ == ["CTCLoss", "CTCDecoder", "CTCEncoder"]
    assert end2end_amd.CTCWithoutBlankLoss is CTCWithoutBlankLoss and end2end_amd.AlignedTargetsLoss is AlignedTargetsLoss
    params = inspect.signature(CTCWithoutBlankLoss.__init__).parameters
    assert [(k, v.default) for k, v in params.items()][:4] == [
        ("self", inspect.Parameter.empty), ("reduce", True), ("after_softmax", False), ("space_idx", -1)]
    fwd = inspect.signature(CTCWithoutBlankLossFunction.forward).parameters
    assert list(fwd) == ["ctx", "logits", "targets", "logits_lengths", "targets_lengths", "space_idx"]
    assert fwd["space_idx"].default == -1
    params = inspect.signature(AlignedTargetsLoss.__init__).parameters
    assert [(k, v.default) for k, v in params.items()] == [
        ("self", inspect.Parameter.empty), ("is_ctc", inspect.Parameter.empty), ("ignore_blank", False)]


def test_binding_rejects_bad_dtype_and_space_before_any_gpu_call():
    from end2end_amd import _C
    args = dict(x=0, input_is_logprobs=True, sB=0, sT=0, sV=0, targets=0, tgt_stride=1, x_len=0, t_len=0, B=1, T=4,
                V=5, Smax=2, losses=0, grads=0, workspace=0, workspace_bytes=0, stream=0)
    with pytest.raises(ValueError, match="dtype"):
        _C.ctc_noblank_fwd_bwd(dtype=_C.F16, space_idx=-1, **args)
    for bad in (-2, 5, 99):
        with pytest.raises(ValueError, match="space_idx"):
            _C.ctc_noblank_fwd_bwd(dtype=_C.F32, space_idx=bad, **args)


def test_library_exports_and_header_declares_the_new_entry_points():
    from end2end_amd import _lib
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "e2e_ctc.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for sym in ("e2e_ctc_noblank_workspace_bytes", "e2e_ctc_noblank_fwd_bwd"):
        assert re.search(r"\b%s\s*\(" % sym, hdr) and hasattr(L, sym) and re.search(r" T %s$" % sym, out, re.M)
    assert L.e2e_ctc_abi_version() == 4 == _lib.ABI_VERSION


def test_workspace_of_the_headline_shape_stays_under_128_megabytes():
    from end2end_amd import _lib
    L = _lib.load()
    n = L.e2e_ctc_noblank_workspace_bytes(256, 1000, 29, 200, _lib.F32)
    assert 0 < n <= 128e6, n


def test_documented_capacity():
    # include/e2e_ctc.h and DESIGN 4.5: targets of up to Smax = 1 855 labels (LDS blocks of one frame), the workspace query
    # 0 one label beyond, whatever the batch, the frames and the dtype
    from end2end_amd import _lib
    L = _lib.load()
    for B, T, dtype in [(1, 1, _lib.F32), (2, 100, _lib.F32), (4, 3000, _lib.F64)]:
        assert L.e2e_ctc_noblank_workspace_bytes(B, T, 29, 1855, dtype) > 0
        assert L.e2e_ctc_noblank_workspace_bytes(B, T, 29, 1856, dtype) == 0
    hdr = open(os.path.join(ROOT, "include", "e2e_ctc.h")).read()
    assert "Smax = 1 855" in hdr and "2 900" not in hdr


def _static_lds():
    """{kernel name: static LDS bytes (group_segment_fixed_size)} of the built library's lattice kernels"""
    import sys
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tools", "perf"))
    import entry_audit
    from end2end_amd import _lib
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in entry_audit.code_objects(_lib.LIB_PATH, tmp):
            notes = subprocess.run([entry_audit.LLVM + "/llvm-readelf", "--notes", co], check=True, capture_output=True,
                                   text=True).stdout
            for blk in re.split(r"\n\s*- \.", notes):
                name = re.search(r"\.name:\s*(\S+)", blk)
                size = re.search(r"\.group_segment_fixed_size:\s*(\d+)", blk)
                if name and size and "lattice_kernel" in name.group(1):
                    out[name.group(1)] = int(size.group(1))
    return out


def test_the_lds_of_every_served_width_fits_beside_the_static_lds():
    # The dynamic LDS a width asks for (nb_lds_bytes of its block K, restated as in test_gpu_noblank.py::nb_block) plus the
    # kernel's static LDS must fit the 160 KiB of a gfx950 workgroup, or the launch fails (it did at Smax 784 and 1856 while
    # the limit assumed 256 bytes of static LDS).  Gram-CTC's lattice kernel against its own widths, the same way.
    static = _static_lds()
    nb = [v for k, v in static.items() if "noblank" in k]
    gc = [v for k, v in static.items() if "gram" in k]
    assert len(nb) == 2 and len(gc) == 2, static

    def nb_lds(S):
        Lm = S + 2
        for K in range(16, 0, -1):
            n = 8 * (3 * (K + 1) * Lm + 2 * K * Lm + 2 * Lm) + 4 * (2 * Lm + 2 * K) + 64
            if n <= 160 * 1024 - 288:
                return n
        return 0

    def gc_lds(S, M):
        NC = (S + 1) * (M + 1)
        for K in (16, 8, 4, 2, 1):
            n = 8 * (2 * K * NC + 4 * NC + 4 * K) + 4 * (3 * NC + S + 1 + K + 16) + 64
            if n <= 160 * 1024 - 256:
                return n
        return 0

    assert nb_lds(1855) and not nb_lds(1856)
    assert max(nb_lds(S) for S in range(1856)) + max(nb) <= 160 * 1024, (static, max(nb_lds(S) for S in range(1856)))
    widest = max(gc_lds(S, M) for M in range(1, 9) for S in range(1400))
    assert widest + max(gc) <= 160 * 1024, (static, widest)
