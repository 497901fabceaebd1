#!/usr/bin/env python3
"""Generator of the word-segmented CTC golden vectors (tests/golden/segmented.npz).

Runs the REFERENCE's own class -- pytorch_end2end/modules/ctc_loss_segmented.py:CTCLossSegmented -- imported from
/root/reference in this container.  Upstream cannot import it as it stands: it asks for `pytorch_end2end.ctc_loss`, which
does not exist, and its alignment is decorated with numba.jit, which is not installed here.  Two stand-ins are put on
sys.modules for the import (generator only; nothing of this travels -- the outputs below are data):
  * `numba`, whose `jit` returns the function unchanged (as make_align_golden.py);
  * `pytorch_end2end.ctc_loss`, whose CTCLoss is the reference's own pytorch_end2end/modules/ctc_loss.py:CTCLoss over the
    reference's compiled engine oracle/_ref/cpp_ctc_loss.so (as make_golden.py imports it).
Inputs are seeded, small and peaky along a random monotone alignment, so that words are recognised; blank_idx = 0,
min_word_length in 0..3.  Per case: the inputs, upstream's (B,) losses, the logits' gradient of loss.sum(), and the
per-segment lengths and targets captured at upstream's inner loss call.  Cases where upstream raises (its segment count
and its segment list disagree: a qualifying space on the last frame, a first boundary at frame 1) are left out and counted.

    python tests/golden/make_segmented_golden.py
"""
import importlib
import os
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, os.path.join(ROOT, "oracle", "_ref"))

import torch  # noqa: E402

N_GENERATED = 40
SPACE = 1


def import_upstream():
    fake = types.ModuleType("numba")
    fake.jit = lambda *a, **k: (lambda f: f)
    sys.modules["numba"] = fake
    pkg = types.ModuleType("pytorch_end2end")
    pkg.__path__ = [os.path.join(REF, "pytorch_end2end")]
    sys.modules["pytorch_end2end"] = pkg
    loss_mod = importlib.import_module("pytorch_end2end.modules.ctc_loss")
    shim = types.ModuleType("pytorch_end2end.ctc_loss")
    shim.CTCLoss = loss_mod.CTCLoss
    sys.modules["pytorch_end2end.ctc_loss"] = shim
    return importlib.import_module("pytorch_end2end.modules.ctc_loss_segmented").CTCLossSegmented


def utterance(rng, V, T):
    """A target of short words and a monotone frame path that spells it: (target ids, path ids), path within T frames."""
    letters = [c for c in range(2, V)]
    while True:
        target, path = [], []
        n_words = int(rng.integers(1, 5))
        for w in range(n_words):
            if w or rng.random() < 0.3:
                target.append(SPACE)
            target += [int(rng.choice(letters)) for _ in range(int(rng.integers(1, 5)))]
        if rng.random() < 0.3:
            target.append(SPACE)
        prev = -1
        for c in target:
            if c == prev or rng.random() < 0.35:
                path.append(0)
            path += [c] * int(rng.integers(1, 3))
            prev = c
        if rng.random() < 0.5:
            path.append(0)
        if len(path) <= T:
            return target, path


def make_case(seed):
    rng = np.random.default_rng(seed)
    B, T, V = int(rng.integers(1, 5)), int(rng.integers(24, 49)), int(rng.integers(4, 8))
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, T, V, generator=g) * 0.7
    utts = [utterance(rng, V, T) for _ in range(B)]
    S = max(len(t) for t, _ in utts)
    targets = torch.zeros((B, S), dtype=torch.long)
    x_len, t_len = torch.zeros(B, dtype=torch.long), torch.zeros(B, dtype=torch.long)
    for b, (tg, path) in enumerate(utts):
        targets[b, :len(tg)] = torch.tensor(tg)
        t_len[b], x_len[b] = len(tg), len(path)
        for t, c in enumerate(path):
            if rng.random() < 0.9:                      # the rest stays noise: words the model does not recognise
                logits[b, t, c] += 6.0
    return dict(logits=logits, targets=targets, x_len=x_len, t_len=t_len, min_word_length=int(seed % 4))


def run_upstream(cls, case):
    mod = cls(space_idx=SPACE, blank_idx=0, min_word_length=case["min_word_length"])
    seen = {}

    def recorder(_module, args):
        _, tg, xl, tl = args
        seen["x_len"], seen["t_len"], seen["targets"] = xl.data.clone(), tl.data.clone(), tg.data.clone()

    mod.ctc.register_forward_pre_hook(recorder)
    x = case["logits"].clone().requires_grad_()
    loss = mod(x, case["targets"], case["x_len"], case["t_len"])
    loss.sum().backward()
    return loss.detach(), x.grad, seen


def main():
    cls = import_upstream()
    flat, kept, segmented, raised = {}, 0, 0, {}
    for seed in range(N_GENERATED):
        case = make_case(seed)
        try:
            loss, grad, seen = run_upstream(cls, case)
        except (AssertionError, IndexError) as e:
            raised[type(e).__name__] = raised.get(type(e).__name__, 0) + 1
            continue
        B = case["logits"].shape[0]
        sx, st = seen["x_len"].numpy().astype(np.int64), seen["t_len"].numpy().astype(np.int64)
        n = len(sx)
        width = max(int(st.max()), 1)
        stg = np.zeros((n, width), dtype=np.int64)
        for i in range(n):
            stg[i, :st[i]] = seen["targets"][i, :st[i]].numpy()
        # the segments partition every utterance's frames in order: where each one lies
        utt, start, b, t = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), 0, 0
        for i in range(n):
            utt[i], start[i] = b, t
            t += int(sx[i])
            if t == int(case["x_len"][b]):
                b, t = b + 1, 0
        assert b == B and t == 0, "upstream's segments do not partition the frames"
        name = "case%02d" % seed
        flat[name + "/logits"] = case["logits"].numpy()
        flat[name + "/targets"] = case["targets"].numpy()
        flat[name + "/x_len"] = case["x_len"].numpy()
        flat[name + "/t_len"] = case["t_len"].numpy()
        flat[name + "/space_idx"] = np.array(SPACE)
        flat[name + "/min_word_length"] = np.array(case["min_word_length"])
        flat[name + "/losses"] = loss.numpy()
        flat[name + "/grad"] = grad.numpy()
        flat[name + "/seg_utt"], flat[name + "/seg_start"] = utt, start
        flat[name + "/seg_x_len"], flat[name + "/seg_t_len"], flat[name + "/seg_targets"] = sx, st, stg
        kept += 1
        segmented += n > B
        print(name, tuple(case["logits"].shape), "min_word_length", case["min_word_length"], "segments", n)
    n_raised = sum(raised.values())
    print("generated %d, kept %d (%d segmented), left out because upstream raised: %d %s" % (N_GENERATED, kept, segmented, n_raised, raised))
    assert n_raised * 4 <= N_GENERATED, "upstream raised in more than a quarter of the cases"
    assert segmented >= 20, "fewer than 20 kept cases are segmented"
    np.savez_compressed(os.path.join(HERE, "segmented.npz"), **flat)


if __name__ == "__main__":
    main()
