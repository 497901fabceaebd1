"""-m gpu: what e2e_ctc_noblank_fwd_bwd and e2e_gram_ctc_fwd_bwd share at the C ABI (csrc/lattice_common.h: one argument
check, one workspace check, one launch): a workspace at any address, and refused calls that touch nothing.  Every refused
call here returns before a launch.  B=2, T=20, V=5, S<=3, the shape of test_gpu_engines_contract.py."""
import ctypes as C

import pytest
import torch

import gpu_util as U
from end2end_amd import _lib
from end2end_amd.engines import gram_table

pytestmark = pytest.mark.gpu

B, T, V, S = 2, 20, 5, 3
ERR_ARG, ERR_WORKSPACE = -1, -3                   # include/e2e_ctc.h
SENTINEL = 7.0


class Call:
    """One entry point at the shape above: fresh outputs filled with SENTINEL, and call(workspace address, bytes, ...)."""

    def __init__(self, which):
        self.L = L = _lib.load()
        d = U.dev()
        g = torch.Generator().manual_seed(11)
        self.x = torch.randn(B, T, V, generator=g).to(d)
        self.tg = torch.randint(1, 4, (B, S), generator=g).to(d)
        self.xl, self.tl = torch.tensor([T, T - 3], device=d), torch.tensor([S, S - 1], device=d)
        self.losses = torch.full((B,), SENTINEL, device=d)
        self.grads = torch.full((B, T, V), SENTINEL, device=d)
        self.reduced = torch.full((1,), SENTINEL, device=d)
        if which == "gram":
            keys, cols, self.order = gram_table(4, V, {4: [1, 2]})
            self.keys, self.cols = torch.from_numpy(keys).to(d), torch.from_numpy(cols).to(d)
            self.fn, self.flags_fn, self.flags_extra = L.e2e_gram_ctc_fwd_bwd, L.e2e_debug_gram_redo_flags, (self.order,)
            self.extra = (self.keys.data_ptr(), self.cols.data_ptr(), self.keys.numel(), 4, self.order)
            self.nbytes = L.e2e_gram_ctc_workspace_bytes(B, T, V, S, self.order, _lib.F32)
        else:
            self.fn, self.flags_fn, self.flags_extra = L.e2e_ctc_noblank_fwd_bwd, L.e2e_debug_noblank_redo_flags, ()
            self.extra = (-1,)
            self.nbytes = L.e2e_ctc_noblank_workspace_bytes(B, T, V, S, _lib.F32)
        assert self.nbytes > 256

    def __call__(self, ws, nbytes, T=T, dtype=_lib.F32, opts=None):
        return self.fn(self.x.data_ptr(), dtype, 0, *self.x.stride(), self.tg.data_ptr(), self.tg.stride(0),
                       self.xl.data_ptr(), self.tl.data_ptr(), B, T, V, S, *self.extra, self.losses.data_ptr(),
                       self.grads.data_ptr(), ws, nbytes, _lib.stream_ptr(U.dev()), C.byref(opts) if opts is not None else None)

    def flags(self, ws):
        out = (C.c_int * B)()
        _lib.check(self.flags_fn(ws, B, T, S, *self.flags_extra, out))
        return out[:]

    def untouched(self):
        torch.cuda.synchronize()
        return all(bool((t == SENTINEL).all()) for t in (self.losses, self.grads, self.reduced))


def _at(buf, offset):
    """the first address in `buf` that lies `offset` bytes behind a 256-byte boundary"""
    return buf.data_ptr() + (offset - buf.data_ptr()) % 256


@pytest.mark.parametrize("which", ["noblank", "gram"])
def test_a_misaligned_workspace_of_exactly_the_size_asked_for_serves_as_an_aligned_one(which):
    a, m = Call(which), Call(which)
    buf_a = torch.empty(a.nbytes + 512, dtype=torch.uint8, device=U.dev())
    buf_m = torch.empty(a.nbytes + 512, dtype=torch.uint8, device=U.dev())
    ws_a, ws_m = _at(buf_a, 0), _at(buf_m, 8)
    assert ws_a % 256 == 0 and ws_m % 256 == 8
    _lib.check(a(ws_a, a.nbytes))
    _lib.check(m(ws_m, m.nbytes))
    torch.cuda.synchronize()
    assert not (a.losses == SENTINEL).any() and torch.isfinite(a.losses).all() and torch.isfinite(a.grads).all()
    assert torch.equal(a.losses, m.losses) and torch.equal(a.grads, m.grads)
    assert a.flags(ws_a) == m.flags(ws_m)


@pytest.mark.parametrize("which", ["noblank", "gram"])
def test_refused_calls_leave_the_outputs_untouched(which):
    c = Call(which)
    buf = torch.empty(c.nbytes + 256, dtype=torch.uint8, device=U.dev())
    ws = _at(buf, 0)
    # (the size asked for is the layout + 256 for the alignment: an aligned workspace one byte short of the layout)
    assert c(ws, c.nbytes - 256 - 1) == ERR_WORKSPACE
    assert c.L.e2e_last_error().decode().startswith("workspace too small")
    assert c.untouched()
    assert c(ws, c.nbytes, T=0) == ERR_ARG and c.untouched()
    assert c(ws, c.nbytes, dtype=_lib.F16) == ERR_ARG and c.untouched()
    bad_reduction = _lib.LossOpts(1.0, c.reduced.data_ptr(), 3, 0)
    assert c(ws, c.nbytes, opts=bad_reduction) == ERR_ARG and c.untouched()
    nowhere_to_reduce = _lib.LossOpts(1.0, None, _lib.REDUCE_SUM, 0)
    assert c(ws, c.nbytes, opts=nowhere_to_reduce) == ERR_ARG and c.untouched()
    # and the same call, accepted, fills them
    ok = _lib.LossOpts(1.0, c.reduced.data_ptr(), _lib.REDUCE_SUM, 0)
    _lib.check(c(ws, c.nbytes, opts=ok))
    torch.cuda.synchronize()
    assert not c.untouched() and abs(c.reduced.item() - c.losses.double().sum().item()) <= 2.0 ** -23 * abs(c.reduced.item())
