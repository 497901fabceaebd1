"""GPU: seeded fuzz of the streaming ASG beam search (e2e_asg_beam_stream) over the cases of tests/asg_beam_fuzz_util.py,
unchanged: every seed of its three families is fed in a chunking drawn from a generator seeded by (family, seed) -- chunks of
one frame, chunks of a random size and calls in which some utterances get no frame, mixed -- and the read-out after the last
chunk and after one randomly chosen interior chunk is held to the GPU's own whole call (e2e_asg_beam_nbest_opt) on the
frames fed: np.array_equal on ids, lengths, n_hyp, scores, counts and timesteps.  The yardstick does the same arithmetic, so
the restatement's margin does not enter and no case is left out.  An utterance whose drawn length lies outside [1, T] is fed
no frame and must read n_hyp = 0.

  family  cases
  plain   132
  long    6
  lm      24
"""
import os

import numpy as np
import pytest
import torch

import asg_beam_fuzz_util as F
import asg_beam_util as U
import asg_stream_util as S
from test_gpu_asg_beam import DTYPES

pytestmark = pytest.mark.gpu


def draw_chunking(family, seed, lens):
    """-> (the calls' per-utterance chunk lengths, the interior call to check after or None)."""
    rng = np.random.default_rng([sorted(F.FAMILIES).index(family), seed, 4711])
    left, calls = list(lens), []
    while any(left):
        kind = int(rng.integers(3))
        size = 1 if kind == 0 else int(rng.integers(1, max(left) + 1))
        take = [min(n, size) for n in left]
        if kind == 2:                                                   # some utterances sit this call out (all of them, at times)
            take = [n if rng.integers(2) else 0 for n in take]
        calls.append(take)
        left = [n - k for n, k in zip(left, take)]
    if not calls:
        calls.append([0] * len(lens))
    return calls, int(rng.integers(len(calls) - 1)) if len(calls) > 1 else None


def check_case(family, seed):
    c = F.draw(family, seed)
    B, T, V = c.x.shape
    dt = DTYPES[c.dtype]
    lens = [n if F.alive(c, b) else 0 for b, n in enumerate(c.lens)]
    calls, interior = draw_chunking(family, seed, lens)
    assert [sum(k[b] for k in calls) for b in range(B)] == lens
    lm = None
    if c.model:
        from end2end_amd.engines import LanguageModel
        labels = list(c.chars) + ["<%d>" % (r + 1) for r in range(c.R)]
        lm = LanguageModel(os.path.join(U.GOLDEN, c.model), labels, c.case_sensitive)
    A = None if c.no_A else torch.from_numpy(c.A).to(dt)
    layout = "time_major" if c.shape["time_major"] else "strided" if c.shape["strided"] else None
    r = S.check_stream(torch.from_numpy(c.x).to(dt), A, lens, calls, c.R, c.W, c.space, lm=lm, layout=layout,
                       check_after={interior, len(calls) - 1}, nbest=c.nbest, lmwt=c.lmwt if c.model else 0.0, wip=c.wip,
                       oov_penalty=c.oov)
    for b in range(B):
        if not F.alive(c, b):
            assert r["n_hyp"][b] == 0 and r["done"][b] == 0


@pytest.mark.parametrize("seed", range(F.FAMILIES["plain"]))
def test_fuzz_plain(seed):
    check_case("plain", seed)


@pytest.mark.parametrize("seed", range(F.FAMILIES["long"]))
def test_fuzz_long(seed):
    check_case("long", seed)


@pytest.mark.parametrize("seed", range(F.FAMILIES["lm"]))
def test_fuzz_lm(seed):
    check_case("lm", seed)


def test_the_families_are_the_fuzz_utilitys():
    assert F.FAMILIES == {"plain": 132, "long": 6, "lm": 24}            # (the counts of this file's docstring)
