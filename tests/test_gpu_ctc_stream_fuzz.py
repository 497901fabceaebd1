"""GPU: seeded fuzz of the streaming CTC beam search (e2e_ctc_beam_stream) over the cases of tests/ctc_beam_fuzz_util.py,
unchanged: every long, lm, lex and trans case, and the plain cases of two frames and more, is fed as a stream.  Half of the
cases go through CTCDecoder.open_stream / feed_nbest, half through stream_util.RawStream, whose state and outputs start as
garbage.  The chunking is drawn per utterance from a generator seeded by (family, seed): chunks of no frame, of one frame and of
a few, then one chunk for the rest; max_frames is T or a few more.  After every chunk each output equals the whole-utterance
call (e2e_ctc_beam_nbest_opt) on the frames fed so far, bit for bit (np.array_equal: DESIGN 4.4 "Equality"); the whole call is
held to the restatement by tests/test_gpu_ctc_beam_fuzz.py, so no margin enters and no case is left out.  In a third of the
cases the rows are permuted between two chunks; in a third one row is reset midway and its results start over; in some raw
cases a chunk that would pass max_frames returns status -2 and leaves the row byte for byte as it was.

  family  cases
  plain   the 130 of 132 with T >= 2
  long    6
  lm      36
  lex     36
  trans   36
The file's wall time on an MI355X is 4 s for its 245 tests: a chunk and its whole call are two launches of milliseconds.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ctc_beam_fuzz_util as F
import stream_util as S
from test_gpu_ctc_beam_fuzz import DEV, DTYPES, decoder, language_model

pytestmark = pytest.mark.gpu

PLAIN = [s for s in range(F.FAMILIES["plain"]) if F.draw("plain", s).x.shape[1] >= 2]


def draw_plan(family, seed, lens, T):
    """-> what the case does: the calls' per-utterance chunk lengths before the last one (which feeds the rest), after which
    call the rows are permuted (and how), after which one which row is reset, before which a chunk too long is refused."""
    rng = np.random.default_rng([F.SEARCHES.index(family), seed, 5813])
    B = len(lens)
    left, calls = list(lens), []
    for _ in range(int(rng.integers(2, 6))):
        take = [min(n, (0, 1, 1, int(rng.integers(2, 6)))[int(rng.integers(4))]) for n in left]
        calls.append(take)
        left = [n - k for n, k in zip(left, take)]
    p = SimpleNamespace()
    p.calls, p.raw = calls, seed % 2 == 1
    p.extra = int(rng.integers(0, 3))                                   # max_frames = T + extra
    p.permute_after = int(rng.integers(len(calls))) if seed % 3 == 0 and B > 1 else None
    p.perm = [int(i) for i in rng.permutation(B)]
    p.reset_after = int(rng.integers(len(calls))) if seed % 3 == 1 else None
    p.reset_row = int(rng.integers(B))
    p.refuse_before = int(rng.integers(len(calls) + 1)) if p.raw and seed % 4 == 3 else None
    p.refuse_row = int(rng.integers(B))
    return p


class Feeder:
    """The stream of a case, through the module or through the raw call: feed(chunk (B,Tc,V) on the GPU, lens) -> the dict of
    stream_util.KEYS (the module's packed tensors padded out again)."""

    def __init__(self, c, p, B, T):
        self.c, self.raw, self.T = c, p.raw, T
        self.max_frames = T + p.extra
        if p.raw:
            self.s = S.RawStream(B, self.max_frames, c.V, c.W, c.labels, c.blank, language_model(c), c.restricted, c.lmwt, c.wip,
                                 c.oov, timesteps=c.timesteps, max_out=T + 1)
        else:
            self.dec = decoder(c)
            self.s = self.dec.open_stream(B, self.max_frames, device=DEV, timesteps=c.timesteps)

    def feed(self, chunk, lens, expect_rc=0):
        c = self.c
        N = c.W if c.nbest is None else c.nbest
        if self.raw:
            return self.s.feed(chunk, lens, nbest=c.nbest, expect_rc=expect_rc)
        xl = torch.tensor(lens)
        res = self.s.feed_nbest(chunk.transpose(0, 1) if c.shape["time_major"] else chunk, xl.to(DEV) if c.seed % 4 == 0 else xl,
                                nbest=c.nbest)
        B, width = chunk.shape[0], res.decoded_targets.shape[2]
        host = lambda t: t.cpu().numpy()   # noqa: E731
        ids = np.zeros((B, N, self.T + 1), dtype=np.int64)
        ids[:, :, :width] = host(res.decoded_targets)
        ts = None
        if c.timesteps:
            ts = np.full((B, N, self.T + 1), -1, dtype=np.int64)
            ts[:, :, :width] = host(res.timesteps)
        return dict(ids=ids, lens=host(res.decoded_targets_lengths), n_hyp=host(res.num_hypotheses),
                    scores=np.stack([host(res.scores), host(res.ctc_scores), host(res.lm_scores)], -1),
                    counts=np.stack([host(res.num_words), host(res.num_oov_words)], -1), ts=ts,
                    done=np.asarray(self.s.frames), sentences=res.decoded_sentences)

    @property
    def state(self):
        return self.s.state

    def permute(self, perm):
        idx = torch.tensor(perm, device=DEV)
        if self.raw:
            self.s.state = self.s.state.index_select(0, idx)            # a copy elsewhere: no address survives in a row
        else:
            self.s.state.copy_(self.s.state.index_select(0, idx))

    def reset(self, row):
        if self.raw:
            self.s.state[row, :S.HEADER] = 0
        else:
            self.s.reset([row])


def check_case(family, seed):
    c = F.draw(family, seed)
    B, T, V = c.x.shape
    lens = [F.frames_of(c, b) for b in range(B)]
    p = draw_plan(family, seed, lens, T)
    lp = torch.from_numpy(c.x).to(DTYPES[c.dtype])
    dlp = lp.to(DEV)
    lm = language_model(c)
    f = Feeder(c, p, B, T)
    whole = {}

    def expected(fed):
        """The whole call on the frames fed so far, per utterance."""
        if fed not in whole:
            whole[fed] = S.reference(lp, list(fed), c.blank, c.W, c.labels, lm, c.restricted, c.lmwt, c.wip, c.oov,
                                     nbest=c.nbest, timesteps=c.timesteps)
        return whole[fed]

    order = list(range(B))                                              # slot j holds utterance order[j]
    fed = [0] * B                                                       # per utterance
    calls = p.calls + [None]
    for i, take in enumerate(calls):
        if p.refuse_before == i:
            # one row is asked to pass max_frames: -2, nothing of it is written, the row stays as it is; the others, fed no
            # frame, read out what they hold
            j = p.refuse_row
            n = f.max_frames - fed[order[j]] + 1
            before = f.state.clone()
            r = f.feed(torch.zeros((B, n, V), dtype=lp.dtype, device=DEV), [n if k == j else 0 for k in range(B)])
            assert r["done"][j] == -2 and r["n_hyp"][j] == -2 and torch.equal(f.state[j], before[j]), (family, seed, i)
            assert (r["ids"][j] == -7).all() and (r["lens"][j] == -7).all()
            ref = expected(tuple(fed))
            for k in range(B):
                if k != j:
                    for key in S.KEYS:
                        assert ref[key] is None or np.array_equal(r[key][k], ref[key][order[k]]), (family, seed, i, key)
        if take is None:
            take = [lens[b] - fed[b] for b in range(B)]                 # the rest
        Tc = max(max(take), 1)
        chunk = torch.zeros((B, Tc, V), dtype=lp.dtype, device=DEV)
        for j, b in enumerate(order):
            chunk[j, :take[b]] = dlp[b, fed[b]:fed[b] + take[b]]
        r = f.feed(chunk, [take[b] for b in order])
        fed = [fed[b] + take[b] for b in range(B)]
        assert r["done"].tolist() == [fed[b] for b in order], (family, seed, i)
        ref = expected(tuple(fed))
        for key in S.KEYS:
            assert ref[key] is None or np.array_equal(r[key], ref[key][order]), (family, seed, i, key)
        if i == p.permute_after:
            f.permute(p.perm)
            order = [order[k] for k in p.perm]
        if i == p.reset_after:
            f.reset(order.index(p.reset_row))
            fed[p.reset_row] = 0                                        # its results start over
    assert fed == lens
    for b in range(B):
        if lens[b] == 0:                                                # never fed: the root alone
            j = order.index(b)
            assert r["n_hyp"][j] == 1 and r["lens"][j, 0] == 1 and r["ids"][j, 0, 0] == -1


@pytest.mark.parametrize("seed", PLAIN)
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


@pytest.mark.parametrize("seed", range(F.FAMILIES["trans"]))
def test_fuzz_trans(seed):
    check_case("trans", seed)


def test_the_plans_mix_what_they_are_there_to_mix():
    """Chunks of no frame, one frame and several, permutations, resets and refusals in every family that can have them, through
    the module and through the raw call, under both kernels."""
    for family in ("plain", "long", "lm", "lex", "trans"):
        kinds = set()
        for seed in (PLAIN if family == "plain" else range(F.FAMILIES[family])):
            c = F.draw(family, seed)
            lens = [F.frames_of(c, b) for b in range(len(c.lens))]
            p = draw_plan(family, seed, lens, c.x.shape[1])
            general = F.takes_general(c.V, c.W, F.lm_kind(c) != "none")
            kinds.add(("raw" if p.raw else "module", general))
            for take in p.calls:
                kinds |= {"no frame"} if 0 in take else set()
                kinds |= {"one frame"} if 1 in take else set()
                kinds |= {"several"} if max(take) > 1 else set()
                kinds |= {"all sit out"} if not any(take) else set()
            kinds |= {"permuted"} if p.permute_after is not None else set()
            kinds |= {"reset"} if p.reset_after is not None else set()
            kinds |= {"refused"} if p.refuse_before is not None else set()
            kinds |= {"max_frames beyond T"} if p.extra else {"max_frames = T"}
        want = {"no frame", "one frame", "several", "all sit out", "permuted", "reset", "refused", "max_frames beyond T",
                "max_frames = T", ("raw", False), ("module", False)}
        if family != "long":
            want |= {("raw", True), ("module", True)}
        assert kinds >= want, (family, want - kinds)
    assert len(PLAIN) == 130
