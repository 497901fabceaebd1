"""GPU: seeded fuzz of CTCDecoder's searches -- e2e_ctc_beam_nbest / _opt through both kernels (ctc_beam_lds.hip,
ctc_beam_general.hip), e2e_ctc_beam and e2e_ctc_greedy -- against the plain-Python restatements tests/lexicon_ref.py and
tests/transcription_ref.py.

Each case (tests/ctc_beam_fuzz_util.py) is one call through CTCDecoder.decode_nbest, built with the case's model, lexicon or
transcriptions and in its call shape (time-major, a view with gaps, CPU tensors, keep_on_device, lengths on either device,
nbest, timesteps); one case in four goes through the C call instead (e2e_ctc_beam_nbest, restricted: _opt), into outputs
filled with garbage, now and then with max_out below the longest hypothesis.  Every utterance whose margin is at least MIN_GAP
is compared with the head of the restatement's ranking: the hypotheses and their order, lengths, num_hypotheses, word and OOV
counts and timestamps exactly, the three scores to nbest_util.ATOL (relative above 1), the padding and the empty slots,
decoded_sentences (transcriptions: against transcription_ref.words_of, and transcribe()), and decode() against hypothesis 0.
An unmasked plain utterance is also held against the CTC loss of its best hypothesis: pruning only loses mass.  Greedy: ids,
lengths and zero padding equal the definition.

  family  cases  utterances  left out for margin  smallest margin  reference: total, slowest (one CPU core)
  plain   132    332         6                    1.8e-7           95 s, 2.2 s (seed 116: V=55, W=512, B=2, T=11)
  long    6      12          0                    1.8e-4           0.9 s, 0.5 s (seed 5: V=29, W=7, T=423)
  lm      36     66          0                    3.3e-6           28 s, 1.8 s (seed 16: V=308, W=256)
  lex     36     60          0                    1.8e-6           2.1 s, 0.3 s (seed 35: V=8, W=512)
  trans   36     77          0                    9.0e-6           4.1 s, 2.5 s (seed 23: V=307, W=100, T=8)
  greedy  30     -           -                    -                -
(The six plain utterances left out: five of f16 / bf16 cases, whose sums lie on a grid and tie exactly between unrelated
prefixes, and one with a tied frame.)  The long family's widths and alphabets are the one-workgroup kernel's; every other
search family reaches both kernels.

The GPU side of a case is one launch of milliseconds; the file's wall time on an MI355X is 87 s for its 277 tests (the slowest
case 3.6 s), nearly all of it the references; tests/test_gpu_ctc_stream_fuzz.py: 245 tests in 4 s.
"""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import ctc_beam_fuzz_util as F
import nbest_util as NB
import transcription_ref as TR
from test_gpu_asg_beam_fuzz import shaped

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
DTYPES = {"f32": torch.float32, "f64": torch.float64, "f16": torch.float16, "bf16": torch.bfloat16}
ATOL = NB.ATOL
CASES = {"plain": 132, "long": 6, "lm": 36, "lex": 36, "trans": 36, "greedy": 30}       # (the docstring's table)


def lm_path(c):
    return F.model_path(c.model, c.pruned) if c.model else None


_models = {}


def language_model(c):
    """The case's model as the C call takes it (None: no model), once per process and configuration."""
    from end2end_amd.engines import LanguageModel
    if F.lm_kind(c) == "none":
        return None
    key = (c.family, c.seed) if c.entries is not None or c.words is not None else (c.model, c.pruned, tuple(c.labels),
                                                                                  c.case_sensitive, c.restricted)
    if key not in _models:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            if c.entries is not None:
                lm = LanguageModel(lm_path(c), c.labels, True, transcriptions=c.entries, blank_idx=c.blank, lexicon=c.restricted)
                assert lm.transcriptions_dropped() == F.table_of(c).dropped
            elif c.words is not None:
                lm = LanguageModel(None, c.labels, c.case_sensitive, words=c.words, lexicon=True)
            else:
                lm = LanguageModel(lm_path(c), c.labels, c.case_sensitive, lexicon=c.restricted)
        _models[key] = lm
    return _models[key]


def decoder(c):
    from end2end_amd import CTCDecoder
    kw = dict(beam_width=c.W, after_logsoftmax=True, blank_idx=c.blank, time_major=c.shape["time_major"], labels=c.labels,
              lmwt=c.lmwt, wip=c.wip, oov_penalty=c.oov, case_sensitive=c.case_sensitive, keep_on_device=c.shape["keep_on_device"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                 # (dropped transcriptions: counted below)
        if c.entries is not None:
            dec = CTCDecoder(transcriptions=c.entries, lm_path=lm_path(c), restrict_to_vocabulary=c.restricted, **kw)
            assert dec._decoder.lm.transcriptions_dropped() == F.table_of(c).dropped
            return dec
    if c.words is not None:
        return CTCDecoder(lexicon=c.words, **kw)
    return CTCDecoder(lm_path=lm_path(c), restrict_to_vocabulary=c.restricted, **kw)


def raw_nbest(c, x, lens, max_out=None):
    """e2e_ctc_beam_nbest (restricted, or every other time: e2e_ctc_beam_nbest_opt) on device tensors -> dict of numpy arrays.
    Every output starts as garbage, so what the call leaves unwritten shows."""
    from end2end_amd import _lib
    L = _lib.load()
    B, T, V = x.shape
    lm = language_model(c)
    xl = torch.as_tensor(np.asarray(lens)).to(DEV, torch.long)
    space_id = c.labels.index(" ") if " " in c.labels else -1
    N = c.W if c.nbest is None else c.nbest
    max_out = T + 1 if max_out is None else max_out
    out = torch.full((B, N, max_out), -7, dtype=torch.long, device=DEV)
    out_len = torch.full((B, N), -7, dtype=torch.long, device=DEV)
    n_hyp = torch.full((B,), -7, dtype=torch.long, device=DEV)
    scores = torch.full((B, N, 3), 7.0, dtype=torch.float64, device=DEV)
    counts = torch.full((B, N, 2), -7, dtype=torch.int32, device=DEV)
    ts = torch.full((B, N, max_out), -7, dtype=torch.long, device=DEV) if c.timesteps else None
    ws = torch.empty(L.e2e_ctc_beam_nbest_workspace_bytes(B, T, V, c.W, 1 if lm is not None else 0, 1 if c.timesteps else 0),
                     dtype=torch.uint8, device=DEV)
    sB, sT, sV = x.stride()
    args = (x.data_ptr(), _lib.dtype_code(x.dtype), sB, sT, sV, xl.data_ptr(), B, T, V, c.blank, c.W, space_id,
            lm.on(DEV).handle if lm is not None else None, c.lmwt, c.wip, c.oov, N, out.data_ptr(), max_out, out_len.data_ptr(),
            n_hyp.data_ptr(), scores.data_ptr(), counts.data_ptr(), ts.data_ptr() if c.timesteps else None,
            ws.data_ptr(), ws.numel(), _lib.stream_ptr(DEV))
    if c.restricted or c.seed % 8 == 5:
        opts = _lib.BeamOpts(1 if c.restricted else 0)
        _lib.check(L.e2e_ctc_beam_nbest_opt(*args, C.byref(opts)))
    else:
        _lib.check(L.e2e_ctc_beam_nbest(*args))
    torch.cuda.synchronize()
    return dict(ids=out.cpu().numpy(), lens=out_len.cpu().numpy(), n_hyp=n_hyp.cpu().numpy(), scores=scores.cpu().numpy(),
                counts=counts.cpu().numpy(), ts=ts.cpu().numpy() if c.timesteps else None)


def layout(x, c):
    """x (B,T,V) on the GPU as the raw call is given it: contiguous, a (B,T,V) view of a time-major tensor, or a view with gaps."""
    x = x.to(DEV)
    if c.shape["time_major"]:
        return x.permute(1, 0, 2).contiguous().permute(1, 0, 2)
    return shaped(x, dict(time_major=False, strided=c.shape["strided"]), DEV)


def run(c):
    """The case's one call -> (dict of numpy arrays, the sentences or None, decode()'s result or None)."""
    x = torch.from_numpy(c.x).to(DTYPES[c.dtype])
    lens = [F.frames_of(c, b) for b in range(len(c.lens))]
    if c.raw:
        return raw_nbest(c, layout(x, c), lens), None, None
    dev = torch.device("cpu") if c.shape["cpu"] else DEV
    xl = torch.tensor(lens)
    if not c.shape["cpu"] and c.seed % 2:
        xl = xl.to(DEV)
    dec = decoder(c)
    xs = shaped(x, c.shape, dev)
    res = dec.decode_nbest(xs, xl, nbest=c.nbest, timesteps=c.timesteps)
    one = dec.decode(xs, xl)
    assert res.decoded_targets.is_cuda == c.shape["keep_on_device"] and (res.timesteps is not None) == c.timesteps
    host = lambda t: t.cpu().numpy()   # noqa: E731
    got = dict(ids=host(res.decoded_targets), lens=host(res.decoded_targets_lengths), n_hyp=host(res.num_hypotheses),
               scores=np.stack([host(res.scores), host(res.ctc_scores), host(res.lm_scores)], -1),
               counts=np.stack([host(res.num_words), host(res.num_oov_words)], -1), ts=host(res.timesteps) if c.timesteps else None)
    return got, (res.decoded_sentences, dec), (host(one.decoded_targets), host(one.decoded_targets_lengths), one.decoded_sentences)


def close(a, b):
    return a == b or abs(a - b) <= ATOL * max(1.0, abs(b))


def check_utterance(got, b, head, what, max_out=None):
    """Utterance b against the head of the restatement's ranking: everything exact but the scores."""
    n = int(got["n_hyp"][b])
    assert n == len(head), (what, n, len(head))
    ids, lens = got["ids"][b], got["lens"][b].tolist()
    width = ids.shape[1]
    for j, w in enumerate(head):
        assert lens[j] == len(w["ids"]), (what, j, lens[j], w["ids"])
        k = min(lens[j], width)                                         # (a short max_out: the needed length, the truncated ids)
        assert tuple(ids[j, :k].tolist()) == w["ids"][:k], (what, j, ids[j, :k].tolist(), w["ids"])
        assert not ids[j, k:].any(), (what, j)
        for i, key in enumerate(("total", "ctc", "lm")):
            assert close(float(got["scores"][b, j, i]), w[key]), (what, j, key, float(got["scores"][b, j, i]), w[key])
        assert got["counts"][b, j].tolist() == [w["words"], w["oov"]], (what, j, got["counts"][b, j].tolist(), w["words"], w["oov"])
        if got["ts"] is not None:
            assert tuple(got["ts"][b, j, :k].tolist()) == w["frames"][:k], (what, j, got["ts"][b, j, :k].tolist(), w["frames"])
            assert (got["ts"][b, j, k:] == -1).all(), (what, j)
    # the empty slots (test_gpu_lexicon, test_gpu_nbest): length 0, scores -inf, -inf, 0, counts 0, timestamps -1
    assert not got["lens"][b, n:].any() and not ids[n:].any(), what
    assert np.isneginf(got["scores"][b, n:, :2]).all() and not got["scores"][b, n:, 2].any(), what
    assert not got["counts"][b, n:].any(), what
    assert got["ts"] is None or (got["ts"][b, n:] == -1).all(), what


def sentence(c, ids, dec=None):
    ids = [k for k in ids if k >= 0]
    if c.entries is None:
        return "".join(c.labels[k] for k in ids)
    lm = F.ref_lm(c)
    name = {lm.word_index(w): w for w, _ in c.entries}
    name[0] = "<unk>"
    words = [name[w] for w in TR.words_of(ids, c.labels, lm, F.table_of(c))]
    if dec is not None:
        assert dec.transcribe(ids) == words, (c.seed, ids)
    return " ".join(words)


def check_case(family, seed):
    c = F.draw(family, seed)
    ref = F.reference(family, seed)
    got, sentences, one = run(c)
    N = c.W if c.nbest is None else c.nbest
    B, T = len(c.lens), c.x.shape[1]
    assert got["scores"].shape[:2] == (B, N) and got["ids"].shape[:2] == (B, N)
    for b in range(B):
        if (seed, b) in F.LEFT_OUT[family]:
            continue
        ranking, gap, _ = ref[b]
        assert gap >= F.MIN_GAP
        head = ranking[:N]                                              # nbest: the head of the full list
        what = (family, seed, b)
        check_utterance(got, b, head, what)
        if sentences is not None:
            assert sentences[0][b] == [sentence(c, r["ids"], sentences[1] if j < 3 else None) for j, r in enumerate(head)], what
            ids, lens, text = one                                       # decode(): hypothesis 0, [-1] for the empty winner
            assert lens[b] == len(head[0]["ids"]) and tuple(ids[b, :lens[b]].tolist()) == head[0]["ids"], what
            assert not ids[b, lens[b]:].any() and text[b] == sentences[0][b][0], what
        n = F.frames_of(c, b)
        if n == 0:                                                      # no frame: the root alone
            assert head[0]["ids"] == (-1,) and len(head) == 1
        elif family == "plain" and not c.masked:
            # pruning only loses mass: the best hypothesis's CTC score never exceeds log P(its labelling)
            seq = [k for k in head[0]["ids"] if k >= 0]
            ll = NB.loglik(c.x[b, :n].astype(np.float64), [seq], c.blank)[0]
            assert float(got["scores"][b, 0, 1]) <= ll + 1e-7, (what, float(got["scores"][b, 0, 1]), ll)
    if c.raw and c.short_out:
        # max_out below the longest hypothesis: the row reports the needed length and holds the truncated ids
        longest = max(len(r["ids"]) for b in range(B) for r in ref[b][0][:N])
        if longest >= 2:
            x = torch.from_numpy(c.x).to(DTYPES[c.dtype])
            short = raw_nbest(c, layout(x, c), [F.frames_of(c, b) for b in range(B)], max_out=longest - 1)
            assert (short["lens"] > longest - 1).any()
            for b in range(B):
                if (seed, b) not in F.LEFT_OUT[family]:
                    check_utterance(short, b, ref[b][0][:N], (family, seed, b, "short"))


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


@pytest.mark.parametrize("seed", range(F.FAMILIES["trans"]))
def test_fuzz_trans(seed):
    check_case("trans", seed)


# ---- greedy ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(F.FAMILIES["greedy"]))
def test_fuzz_greedy(seed):
    from end2end_amd import CTCDecoder
    c = F.draw("greedy", seed)
    x = torch.from_numpy(c.x).to(DTYPES[c.dtype])
    B, T, V = x.shape
    dec = CTCDecoder(beam_width=1, blank_idx=c.blank, time_major=c.shape["time_major"])
    xs = shaped(x, c.shape, DEV)
    res = dec.decode_greedy(xs, torch.tensor(c.lens).to(DEV))
    assert res.decoded_targets.shape == (B, T)
    for b in range(B):
        want = F.greedy_definition(c, b)
        n = int(res.decoded_targets_lengths[b])
        assert n == len(want) and res.decoded_targets[b, :n].tolist() == want, (seed, b)
        assert not res.decoded_targets[b, n:].any(), (seed, b)


def test_the_families_are_the_fuzz_utilitys():
    assert F.FAMILIES == CASES
