"""GPU: seeded fuzz of Gram-CTC decoding -- e2e_gram_ctc_beam_nbest, e2e_gram_ctc_beam_nbest_lm / _opt and e2e_gram_ctc_greedy
-- against the plain-Python restatements tests/gram_decode_ref.py, tests/gram_decode_lm_ref.py and tests/gram_lexicon_ref.py.

Each case (tests/gram_beam_fuzz_util.py) is one call through GramCTCDecoder, with configure(), restrict_to_vocabulary() and
decode_nbest(..., timesteps=...) as the case says and in its call shape (time-major, a view with gaps, CPU tensors,
keep_on_device, nbest); one case in four goes through the C call instead, into outputs filled with garbage
(gram_stream_util.reference), so that what the kernel leaves unwritten shows.  Every utterance whose margin is at least
MIN_GAP is compared: the hypotheses and their order, lengths, num_hypotheses, word and OOV counts and timesteps exactly,
the scores -- scored searches: total, acoustic and LM score -- to 1e-9 * max(1, |score|), the empty slots as
test_gpu_gram_decode.check_empty_slots has them.  An unmasked plain utterance is also held against the Gram-CTC loss of its
best hypothesis: pruning only loses mass.  Greedy: ids, columns and lengths equal the definition, the padding is zero.

  family  cases  utterances  left out for margin  smallest margin  reference: total, slowest (one CPU core)
  plain   132    285         1 (seed 115, 0)      2.1e-6           38 s, 1.5 s (V=1023, W=32, B=4, T=9)
  long    6      12          0                    1.2e-5           3.1 s, 1.0 s (V=33, W=6, B=2, T=680)
  lm      28     52          0                    1.2e-6           14 s, 2.4 s (V=47, W=128, B=2, T=19)
  lex     28     50          0                    4.9e-6           5.8 s, 1.2 s (V=67, W=127, B=2, T=13)
  greedy  30     -           -                    -                -

The GPU side of a case is one launch of a few milliseconds; the file's wall time on an MI355X is about 45 s for its 228
tests (the slowest case 1.6 s), nearly all of it the references; tests/test_gpu_gram_stream_fuzz.py: 196 tests in 4 s.
"""
import os

import numpy as np
import pytest
import torch

import gram_beam_fuzz_util as F
import gram_decode_lm_ref as LR
import gram_decode_ref as DR
import gram_ref as GR
import gram_stream_util as S
from test_gpu_asg_beam_fuzz import shaped
from test_gpu_gram_decode import gram_loss

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
DTYPES = {"f32": torch.float32, "f64": torch.float64, "f16": torch.float16, "bf16": torch.bfloat16}
TOL = 1e-9
NINF = float("-inf")
CASES = {"plain": 132, "long": 6, "lm": 28, "lex": 28, "greedy": 30}        # (the docstring's table)


def scored(c):
    return c.family in ("lm", "lex")


def language_model(c):
    """The case's model as the C call takes it: an ARPA model, with its lexicon where the search is restricted, or a word list."""
    from end2end_amd.engines import LanguageModel
    if c.words is not None:
        return LanguageModel(None, c.labels, c.case_sensitive, words=c.words, lexicon=True)
    if c.model is None:
        return None
    return LanguageModel(os.path.join(LR.GOLDEN, c.model), c.labels, c.case_sensitive, lexicon=c.restricted)


def raw_search(c):
    if not scored(c):
        return S.Search(c.R, c.V, c.l2i, c.W)
    return S.Search(c.R, c.V, c.l2i, c.W, True, c.labels, language_model(c), c.restricted, lmwt=c.lmwt, wip=c.wip, oov_penalty=c.oov)


def layout_of(c):
    return "time_major" if c.shape["time_major"] else "strided" if c.shape["strided"] else None


def run(c):
    """The case's one call -> (gram_stream_util's dict of numpy arrays, the sentences or None)."""
    x = torch.from_numpy(c.x).to(DTYPES[c.dtype])
    if c.raw:
        return S.reference(S.view_of(x.to(DEV), layout_of(c)), c.lens, raw_search(c), nbest=c.nbest,
                           timesteps=scored(c) and c.timesteps), None
    from end2end_amd.decoders import GramCTCDecoder
    dev = torch.device("cpu") if c.shape["cpu"] else DEV
    lens = torch.tensor(c.lens)
    if not c.shape["cpu"] and c.seed % 2:
        lens = lens.to(DEV)
    dec = GramCTCDecoder(0, c.R, c.V, c.l2i, beam_width=c.W, labels=c.labels if scored(c) else None, after_logsoftmax=True,
                         time_major=c.shape["time_major"], keep_on_device=c.shape["keep_on_device"])
    if scored(c):
        dec.configure(lm_path=os.path.join(LR.GOLDEN, c.model) if c.model and c.words is None else None, lmwt=c.lmwt, wip=c.wip,
                      oov_penalty=c.oov, case_sensitive=c.case_sensitive)
        if c.restricted:
            dec.restrict_to_vocabulary(c.words)
    res = dec.decode_nbest(shaped(x, c.shape, dev), lens, nbest=c.nbest, timesteps=scored(c) and c.timesteps)
    assert res.decoded_targets.is_cuda == c.shape["keep_on_device"]
    host = lambda t: t.cpu().numpy()   # noqa: E731
    got = dict(ids=host(res.decoded_targets), lens=host(res.decoded_targets_lengths), n_hyp=host(res.num_hypotheses),
               scores=host(res.scores), counts=None, ts=None)
    if scored(c):
        got["scores"] = np.stack([host(res.scores), host(res.ctc_scores), host(res.lm_scores)], -1)
        got["counts"] = np.stack([host(res.num_words), host(res.num_oov_words)], -1)
        assert (res.timesteps is not None) == c.timesteps
        got["ts"] = host(res.timesteps) if c.timesteps else None
    return got, res.decoded_sentences


def check_utterance(got, b, head, is_scored, what):
    """Utterance b against the head of the restatement's ranking: everything exact but the scores."""
    n = int(got["n_hyp"][b])
    assert n == len(head), (what, n, len(head))
    lens, ids = got["lens"][b].tolist(), got["ids"][b]
    assert [tuple(ids[j, :lens[j]].tolist()) for j in range(n)] == [r["ids"] for r in head], what
    for j, w in enumerate(head):
        assert not ids[j, lens[j]:].any(), (what, j)
        if is_scored:
            for i, k in enumerate(("total", "ac", "lm")):
                g = float(got["scores"][b, j, i])
                assert abs(g - w[k]) <= TOL * max(1.0, abs(w[k])), (what, j, k, g, w[k])
            assert got["counts"][b, j].tolist() == [w["words"], w["oov"]], (what, j)
            if got["ts"] is not None:
                assert tuple(got["ts"][b, j, :lens[j]].tolist()) == w["frames"], (what, j)
                assert (got["ts"][b, j, lens[j]:] == -1).all(), (what, j)
        else:
            g = float(got["scores"][b, j])
            assert abs(g - w["total"]) <= TOL * max(1.0, abs(w["total"])), (what, j, g, w["total"])
    # the empty slots (test_gpu_gram_decode.check_empty_slots, test_gpu_gram_lexicon.check_rows)
    assert not got["lens"][b, n:].any() and not ids[n:].any(), what
    if is_scored:
        assert np.isneginf(got["scores"][b, n:, :2]).all() and not got["scores"][b, n:, 2].any(), what
        assert not got["counts"][b, n:].any(), what
        assert got["ts"] is None or (got["ts"][b, n:] == -1).all(), what
    else:
        assert np.isneginf(got["scores"][b, n:]).all(), what


def check_case(family, seed):
    c = F.draw(family, seed)
    ref = F.reference(family, seed)
    got, sentences = run(c)
    N = c.W if c.nbest is None else c.nbest
    B, T = len(c.lens), c.x.shape[1]
    assert got["scores"].shape[:2] == (B, N) and got["ids"].shape[:2] == (B, N)
    for b in range(B):
        if (seed, b) in F.LEFT_OUT[family]:
            continue
        ranking, gap, _ = ref[b]
        assert gap >= F.MIN_GAP
        head = ranking[:N]                                              # nbest: the head of the full list
        check_utterance(got, b, head, scored(c), (family, seed, b))
        if sentences is not None:
            assert sentences[b] == ["".join(c.labels[i] for i in r["ids"]) if scored(c) else "" for r in head]
        n = F.frames_of(c, b)
        if n == 0:                                                      # no frame: the empty hypothesis alone, all scores 0
            assert int(got["n_hyp"][b]) == 1 and int(got["lens"][b, 0]) == 0 and not np.any(got["scores"][b, 0])
        elif family == "plain" and not c.masked and head:
            # pruning only loses mass: the best hypothesis never scores above -GramCTCLoss of its sequence
            loss = gram_loss(c.R, c.V, c.l2i, torch.from_numpy(c.x[b]).double(), n, [list(head[0]["ids"])])[0]
            assert float(got["scores"][b, 0]) <= -loss + 1e-7, (seed, b, float(got["scores"][b, 0]), -loss)


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


# ---- the width cap above 1024 columns ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1025, 1100])
def test_the_width_cap_beyond_1024_columns(V):
    """cap + 1 is refused on the host before any launch; cap itself decodes what the restatement does."""
    from end2end_amd import _C
    from end2end_amd.decoders import GramCTCDecoder
    at_cap = [s for s in range(F.FAMILIES["plain"]) if F.draw("plain", s).V == V and F.draw("plain", s).at_cap]
    assert at_cap
    c = F.draw("plain", at_cap[0])
    K = max([len(g) for g in c.l2i.values()] + [1])
    cap = _C.gram_beam_max_width(V, K)
    assert cap == F.max_width(V) == c.W < 128
    z = torch.zeros(8, dtype=torch.long, device=DEV)           # (addresses that no kernel may touch: the host refuses first)
    with pytest.raises(_C.E2EError, match="beam_width"):
        _C.gram_ctc_beam_nbest(z.data_ptr(), _C.F32, 0, 0, 0, z.data_ptr(), 1, 1, V, z.data_ptr(), z.data_ptr(), K,
                               cap + 1, 1, z.data_ptr(), 1, z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), 0, 0)
    assert _C.gram_beam_workspace_bytes(1, 4, V, K, cap + 1) == 0 and _C.gram_beam_workspace_bytes(1, 4, V, K, cap) > 0
    with pytest.raises(ValueError, match="beam_width"):
        GramCTCDecoder(0, c.R, V, c.l2i, beam_width=cap + 1)
    check_case("plain", at_cap[0])


# ---- what the draw found: lex seed 10 -----------------------------------------------------------------------------------------
def test_without_a_space_label_a_last_word_may_be_unfinished():
    """A table without a space (space_id = -1), restricted: the one word's last spelling may be a proper prefix that is no word
    (it counts as out of vocabulary), whether single ids or a gram spell it.  The restricted walk took the -1 behind a gram's
    last id for the space and asked for a finished word there."""
    from end2end_amd.decoders import GramCTCDecoder
    labels, l2i = ["_", "a", "b", "c"], {4: [1, 2], 5: [1, 2, 3]}      # the grams `ab` and `abc`
    dec = GramCTCDecoder(0, 4, 6, l2i, beam_width=4, labels=labels, after_logsoftmax=True)
    dec.configure(wip=0.0).restrict_to_vocabulary(["abc"])

    def forced(cols):
        lp = torch.full((1, len(cols), 6), NINF, dtype=torch.float64)
        for t, col in enumerate(cols):
            lp[0, t, col] = 0.0
        res = dec.decode_nbest(lp.to(DEV), timesteps=True)
        n = int(res.num_hypotheses[0])
        return [(res.decoded_sentences[0][j], int(res.num_words[0, j]), int(res.num_oov_words[0, j])) for j in range(n)]

    assert forced([1]) == [("a", 1, 1)] and forced([1, 2]) == [("ab", 1, 1)] and forced([4]) == [("ab", 1, 1)]
    assert forced([1, 2, 3]) == forced([4, 3]) == forced([5]) == [("abc", 1, 0)]
    assert forced([2]) == [] and forced([4, 1]) == [] and forced([5, 4]) == []


# ---- greedy ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(F.FAMILIES["greedy"]))
def test_fuzz_greedy(seed):
    from end2end_amd.decoders import GramCTCDecoder
    c = F.draw("greedy", seed)
    grams = GR.grams_of(c.R, c.V, c.l2i)
    K = max(len(g) for g in grams.values())
    x = torch.from_numpy(c.x).to(DTYPES[c.dtype])
    B, T, V = x.shape
    dec = GramCTCDecoder(0, c.R, V, c.l2i, beam_width=1, time_major=c.shape["time_major"])
    res = dec.decode_greedy(shaped(x, c.shape, DEV), torch.tensor(c.lens).to(DEV), return_columns=True)
    assert res.decoded_targets.shape == (B, T * K) and res.columns.shape == (B, T)
    xs = x.double().numpy()                                             # (the conversion up is exact: the same arg-max)
    ties, made = 0, 0
    for b in range(B):
        ids, cols = DR.greedy(xs[b], c.lens[b], grams)
        n, m = int(res.decoded_targets_lengths[b]), int(res.columns_lengths[b])
        assert (n, m) == (len(ids), len(cols)), (seed, b)
        assert res.decoded_targets[b, :n].tolist() == ids and not res.decoded_targets[b, n:].any(), (seed, b)
        assert res.columns[b, :m].tolist() == cols and not res.columns[b, m:].any(), (seed, b)
        top = xs[b, :c.lens[b]].max(axis=1, keepdims=True)
        ties += int(((xs[b, :c.lens[b]] == top).sum(axis=1) > 1).sum())
        made += int(c.tied[b, :c.lens[b]].sum())
    assert ties >= made                                                 # (the constructed ties survive the conversion)


def test_the_families_are_the_fuzz_utilitys():
    assert F.FAMILIES == CASES
