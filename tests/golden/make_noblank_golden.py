#!/usr/bin/env python3
"""Generator of the CTC-without-blank and aligned-targets-loss golden vectors (tests/golden/noblank.npz).

Runs the REFERENCE's own code -- pytorch_end2end/functions/ctc_without_blank.py (:13-138), modules/ctc_without_blank.py
and modules/alignment_loss.py -- loaded by path from /root/reference in this container.  Their numba decorators are served
by a stand-in `numba` (`jit` returns the function unchanged, `vectorize` is np.vectorize), and their
`from pytorch_end2end.... import ...` lines by stand-in `pytorch_end2end` packages registered in sys.modules of this
process only, whose members are the reference's own files (functions/utils.py, utils/alignment.py).  No test imports
this script; only its outputs (data) are committed.  Inputs come from seeded torch generators and are stored with the
outputs: module-level losses and logits.grad of (loss * w).sum().backward() (float32-rounded upstream whatever the input
dtype), and the engine level in f64: losses and the kept gradient exp(lp) - posterior of the numpy lattice itself.

    python tests/golden/make_noblank_golden.py
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/pytorch_end2end"

fake = types.ModuleType("numba")
fake.jit = lambda *a, **k: (lambda f: f)
fake.vectorize = lambda *a, **k: (lambda f: np.vectorize(f))
fake.float64 = lambda *a: None
sys.modules["numba"] = fake


def _package(name):
    mod = types.ModuleType(name)
    mod.__path__ = []
    sys.modules[name] = mod
    return mod


def _load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


for pkg in ("pytorch_end2end", "pytorch_end2end.functions", "pytorch_end2end.modules", "pytorch_end2end.utils"):
    _package(pkg)
_load("pytorch_end2end.functions.utils", "functions/utils.py")
_load("pytorch_end2end.utils.alignment", "utils/alignment.py")
_load("pytorch_end2end.functions.ctc_without_blank", "functions/ctc_without_blank.py")
ref_fn = sys.modules["pytorch_end2end.functions.ctc_without_blank"]
ref_nb = _load("pytorch_end2end.modules.ctc_without_blank", "modules/ctc_without_blank.py")
ref_al = _load("pytorch_end2end.modules.alignment_loss", "modules/alignment_loss.py")


def noblank_case(seed, B, T, V, S, space_idx, after_softmax=False, dtype=torch.float32, x_len=None, t_len=None,
                 targets=None, sharp=1.0, reduce=False):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, T, V, generator=g, dtype=torch.float64) * sharp
    if after_softmax:
        logits = torch.softmax(logits, -1)
    logits = logits.to(dtype)
    tg = torch.randint(0, V, (B, max(S, 1)), generator=g) if targets is None else torch.tensor(targets)
    tl = torch.randint(max(S // 2, 0), S + 1, (B,), generator=g) if t_len is None else torch.tensor(t_len)
    xl = torch.randint(max(T // 2, 1), T + 1, (B,), generator=g) if x_len is None else torch.tensor(x_len)
    if x_len is None:
        xl[0] = T
    w = torch.rand(B, generator=g, dtype=torch.float64).to(dtype) + 0.5
    x = logits.clone().requires_grad_()
    loss = ref_nb.CTCWithoutBlankLoss(reduce=reduce, after_softmax=after_softmax, space_idx=space_idx)(x, tg, xl, tl)
    (loss.sum() if reduce else (loss * w.to(loss.dtype)).sum()).backward()
    # the engine level in f64 (upstream's module rounds losses and kept gradients to float32, even for f64 inputs):
    # eng_grad = exp(lp) - posterior, the kept gradient of the Function
    lp64 = torch.log(logits.double()) if after_softmax else torch.log_softmax(logits.double(), -1)
    eng_loss, eng_grad = ref_fn._ctc_without_blank_3d_loss(lp64.numpy(), tg.numpy(), xl.numpy(), tl.numpy(), space_idx)
    return dict(logits=logits.numpy(), targets=tg.numpy(), x_len=xl.numpy(), t_len=tl.numpy(),
                space_idx=np.array(space_idx), after_softmax=np.array(int(after_softmax)), reduce=np.array(int(reduce)),
                w=w.numpy(), loss=loss.detach().double().numpy(), grad=x.grad.numpy(),
                eng_loss=np.asarray(eng_loss, dtype=np.float64), eng_grad=eng_grad)


def aligned_case(seed, B, T, V, S, is_ctc, ignore_blank):
    g = torch.Generator().manual_seed(seed)
    lp = torch.log_softmax(torch.randn(B, T, V, generator=g, dtype=torch.float64) * 2.0, -1).float()
    tg = torch.randint(1, V, (B, S), generator=g)
    tl = torch.randint(max(S // 2, 1), S + 1, (B,), generator=g)
    xl = torch.randint(max(T // 2, 1), T + 1, (B,), generator=g)
    xl[0] = T
    xl = torch.maximum(xl, 2 * tl + 1)
    x = lp.clone().requires_grad_()
    loss = ref_al.AlignedTargetsLoss(is_ctc, ignore_blank=ignore_blank)(x, tg, xl, tl)
    loss.sum().backward()
    return dict(log_probs=lp.numpy(), targets=tg.numpy(), x_len=xl.numpy(), t_len=tl.numpy(), is_ctc=np.array(int(is_ctc)),
                ignore_blank=np.array(int(ignore_blank)), loss=loss.detach().double().numpy(), grad=x.grad.numpy())


def main():
    V = 6
    cases = {
        # space_idx -1: ragged lengths, repeated labels (doubled pairs in row 1)
        "plain": noblank_case(1, 4, 12, V, 5, -1, targets=[[1, 2, 3, 4, 5], [2, 2, 3, 3, 1], [0, 5, 5, 1, 2], [4, 1, 0, 2, 3]],
                              t_len=[5, 5, 3, 4], x_len=[12, 9, 7, 12]),
        # a middle space label: a target that starts / ends with it (doubled spaces), the target [sp], an empty target
        "space_mid": noblank_case(2, 5, 14, V, 4, 2, targets=[[2, 1, 4, 2], [1, 3, 3, 5], [2, 0, 0, 0], [4, 4, 4, 4], [1, 2, 3, 2]],
                                  t_len=[4, 4, 1, 0, 3], x_len=[14, 10, 6, 5, 9]),
        # the last label as space, probabilities in (after_softmax)
        "space_last_softmax": noblank_case(3, 4, 10, V, 4, V - 1, after_softmax=True, t_len=[4, 2, 3, 1], x_len=[10, 8, 4, 6]),
        "softmax_nospace": noblank_case(4, 3, 9, V, 3, -1, after_softmax=True, t_len=[3, 2, 3], x_len=[9, 5, 3]),
        # one frame: without spaces a single label; with spaces [sp a sp], [sp] and the empty target
        "t1_nospace": noblank_case(5, 3, 1, V, 1, -1, targets=[[3], [0], [5]], t_len=[1, 1, 1], x_len=[1, 1, 1]),
        "t1_space": noblank_case(6, 3, 1, V, 1, V - 1, targets=[[3], [5], [0]], t_len=[1, 1, 0], x_len=[1, 1, 1]),
        # an infeasible utterance (L > T without spaces; S > T with them) between feasible ones
        "infeasible": noblank_case(7, 3, 8, V, 6, -1, t_len=[4, 6, 2], x_len=[8, 5, 6]),
        "infeasible_space": noblank_case(8, 3, 8, V, 6, 1, t_len=[3, 6, 5], x_len=[8, 5, 8]),
        # Q10: space_idx -1 and an empty target score column V-1
        "q10_empty": noblank_case(9, 3, 7, V, 3, -1, t_len=[0, 2, 0], x_len=[7, 6, 3]),
        "f64": noblank_case(10, 4, 16, 7, 5, 3, dtype=torch.float64, sharp=2.0),
        "reduce": noblank_case(11, 3, 11, V, 4, 0, reduce=True),
        "longer": noblank_case(12, 3, 60, 12, 20, 11, sharp=2.0),
    }
    for i, (is_ctc, ignore_blank) in enumerate([(True, False), (True, True), (False, False), (False, True)]):
        cases["aligned_%s_%s" % ("ctc" if is_ctc else "asg", "ign" if ignore_blank else "all")] = \
            aligned_case(20 + i, 4, 16, 6, 5, is_ctc, ignore_blank)
    flat = {}
    for name, c in cases.items():
        for k, v in c.items():
            flat[name + "/" + k] = v
        print(name, "loss", np.round(c["loss"], 4).tolist())
    np.savez_compressed(os.path.join(HERE, "noblank.npz"), **flat)


if __name__ == "__main__":
    main()
