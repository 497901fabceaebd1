"""GPU: seeded fuzz of the streaming Gram-CTC beam search (e2e_gram_ctc_beam_stream) over the cases of
tests/gram_beam_fuzz_util.py, unchanged: every seed of its plain, long, lm and lex families is fed in a chunking drawn from a
generator seeded by (family, seed) -- chunks of one frame, chunks of a random size and calls in which some or all utterances
get no frame, mixed -- and the read-out after the last chunk and after one randomly chosen interior chunk is held to the GPU's
own whole call (e2e_gram_ctc_beam_nbest, scored: e2e_gram_ctc_beam_nbest_opt) on the frames fed: np.array_equal on ids,
lengths, n_hyp, scores, counts and timesteps (gram_stream_util.check_stream).  The yardstick does the same arithmetic, so the
restatements' margin does not enter and no case is left out.  With a model every resume refills the answer cache from the
members' own sequences: at up to 128 members, and at some 200 columns in the wide tables of lm and lex.

  family  cases
  plain   132
  long    6
  lm      28
  lex     28
"""
import numpy as np
import pytest
import torch

import gram_beam_fuzz_util as F
import gram_stream_util as S
from test_gpu_gram_beam_fuzz import DTYPES, layout_of, raw_search, scored

pytestmark = pytest.mark.gpu

CASES = {"plain": 132, "long": 6, "lm": 28, "lex": 28}                 # (the docstring's table)


def draw_chunking(family, seed, lens):
    """-> (the calls' per-utterance chunk lengths, the interior call to check after or None)."""
    rng = np.random.default_rng([F.SEARCHES.index(family), seed, 4712])
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
    lens = [F.frames_of(c, b) for b in range(B)]
    calls, interior = draw_chunking(family, seed, lens)
    assert [sum(k[b] for k in calls) for b in range(B)] == lens
    r = S.check_stream(torch.from_numpy(c.x).to(DTYPES[c.dtype]), lens, calls, raw_search(c), layout=layout_of(c),
                       check_after={interior, len(calls) - 1}, nbest=c.nbest, timesteps=scored(c) and c.timesteps)
    assert r["done"].tolist() == lens
    for b in range(B):
        if lens[b] == 0:                                                # never fed: the empty hypothesis
            assert r["n_hyp"][b] == 1 and r["lens"][b, 0] == 0 and not np.any(r["scores"][b, 0])


@pytest.mark.parametrize("seed", range(F.FAMILIES["plain"]))
def test_fuzz_plain(seed):
    check_case("plain", seed)


@pytest.mark.parametrize("seed", range(F.FAMILIES["long"]))
def test_fuzz_long(seed):
    check_case("long", seed)


@pytest.mark.parametrize("seed", range(F.FAMILIES["lm"]))
def test_fuzz_lm(seed):
    check_case("lm", seed)


@pytest.mark.parametrize("seed", range(F.FAMILIES["lex"]))
def test_fuzz_lex(seed):
    check_case("lex", seed)


def test_the_chunkings_mix_what_they_are_there_to_mix():
    """Single frames, sizes above one, calls in which some and calls in which all utterances sit out, interior read-outs; and
    resumes with a model at 128 members and at a table of 150 columns and more."""
    kinds = set()
    wide, full = False, False
    for family in CASES:
        for seed in range(F.FAMILIES[family]):
            c = F.draw(family, seed)
            lens = [F.frames_of(c, b) for b in range(len(c.lens))]
            calls, interior = draw_chunking(family, seed, lens)
            kinds.add("interior" if interior is not None else "last only")
            left = list(lens)
            for take in calls:
                if max(take) == 1:
                    kinds.add("one frame")
                if max(take) > 1:
                    kinds.add("several frames")
                if not any(take):
                    kinds.add("all sit out")
                elif any(k == 0 and n > 0 for k, n in zip(take, left)):
                    kinds.add("some sit out")
                left = [n - k for n, k in zip(left, take)]
            if scored(c) and (c.model or c.words) and len(calls) >= 3:
                wide |= c.V >= 150 and c.W >= 100
                full |= c.W == 128 and max(lens) >= 4
    assert kinds == {"interior", "last only", "one frame", "several frames", "all sit out", "some sit out"}
    assert wide and full


def test_the_families_are_the_fuzz_utilitys():
    assert {k: F.FAMILIES[k] for k in F.SEARCHES} == CASES
