"""-m gpu: bench.py's plain run, started as a fresh child (never an exec from this process, which has touched the GPU): one
headline line, --steps honoured, nothing of --full measured, and --dump-outputs writes what the last timed step returned --
checked against the oracle on a sample of the seeded batch, rebuilt on the host."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import oracle_lib as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32_RTOL, F32_ATOL = 1e-4, 2e-6          # tests/test_gpu_loss.py


def test_plain_run_prints_the_headline_and_dumps_the_step_outputs(tmp_path):
    dump = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
                        "--dump-outputs", str(dump)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    res = json.loads(lines[0])
    assert res["metric"] == "ctc_fwd_bwd_frames_per_sec" and res["unit"] == "frames/s" and res["higher_is_better"] is True
    assert res["dtype"] == "f32" and res["n_gpus"] == 1 and res["steps"] == 7 and res["warmup"] == 2
    assert res["ms_per_step"] > 0 and abs(res["value"] * res["ms_per_step"] * 1e-3 - 256 * 1000) <= 1e-6 * 256 * 1000
    assert "roofline" not in res and "module_ms_per_step" not in res and "decode" not in res

    assert sorted(p.name for p in dump.iterdir()) == ["grads.npy", "losses.npy", "mean_loss.npy"]
    assert sum(p.stat().st_size for p in dump.iterdir()) <= 64 << 20
    losses, grads, mean = (np.load(dump / n) for n in ("losses.npy", "grads.npy", "mean_loss.npy"))
    assert losses.dtype == grads.dtype == mean.dtype == np.float32
    assert losses.shape == (256,) and grads.shape == (256, 1000, 29) and mean.shape == (1,)
    np.testing.assert_allclose(mean[0], losses.astype(np.float64).mean(), rtol=1e-5)

    sys.path.insert(0, ROOT)
    import bench
    w = bench.WORKLOAD
    (x, tg, xl, tl), _ = bench.make_batch(1000, w["B"], w["T"], w["V"], w["S"], "cpu")
    idx = [0, 1, 128, 255]
    lp = torch.log_softmax(x[idx].double(), -1).numpy()
    l_ref, g_ref = O.ctc_loss(lp, tg[idx].numpy(), xl[idx].numpy(), tl[idx].numpy(), 0)
    np.testing.assert_allclose(losses[idx], l_ref, rtol=F32_RTOL)
    # the step's gradient is that of the batch mean: 1/B times the oracle's
    np.testing.assert_allclose(grads[idx].astype(np.float64) * w["B"], g_ref, rtol=F32_RTOL, atol=F32_ATOL)
