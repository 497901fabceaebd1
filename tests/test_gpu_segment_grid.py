"""-m gpu: the banded segment kernel's grid (launch_segments_band, end2end_amd/csrc/ctc_loss_fast.hip).  Its fast index is the
utterance and the segment index is folded over the grid's y and z extents, which end at 65 535 each, while a call may have up
to 2^18 segments of 16 frames.  One utterance of 65 538 segments (1 048 608 frames: two z planes of 32 769, the second with no
surplus; a single y extent would not hold them) with a targets tensor 128 wide -- the route with the lean halo chains and the
banded segment kernel --, against the f64 oracle at the default tolerances: losses 6e-7 relative, gradients 2e-6 + 1e-4 |g|.
The fault this guards against shows only beyond 1 048 560 frames; the call takes 0.9 s and the oracle 1.6 s.
"""
import numpy as np
import pytest
import torch

import oracle_lib as O
import gpu_util as U
from end2end_amd import _lib

pytestmark = pytest.mark.gpu


def test_more_segments_than_one_grid_extent_holds():
    T, V, S, width = 65538 * 16, 4, 20, 128
    rng = np.random.default_rng(9100)
    x = rng.standard_normal((1, T, V)).astype(np.float32)
    tg = rng.integers(1, V, size=(1, width))
    keep = {}
    la, ga = U.c_abi_loss(torch.from_numpy(x), tg, [T], [S], 0, False, _lib.ALGO_AUTO, keep=keep, width=width, padding=-1)
    route = keep["route"]
    assert route // 1000 == 2 and route % 10 == 4 and route % 100 // 10 == 4, "route %d: not the lean halo chains" % route
    xd = x.astype(np.float64)
    m = xd.max(axis=-1, keepdims=True)
    lp = xd - m - np.log(np.exp(xd - m).sum(axis=-1, keepdims=True))
    l_o, g_o = O.ctc_loss(lp, tg, np.array([T]), np.array([S]), 0)
    print("loss", la, "oracle", l_o, "max |dgrad| %.3g" % np.abs(ga - g_o).max())
    U.assert_same(la, l_o, 6e-7, 0.0, "losses")
    U.assert_same(ga, g_o, 1e-4, 2e-6, "grads")
