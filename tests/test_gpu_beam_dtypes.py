"""-m gpu: every (input dtype, LM kind, streaming or not) instance of both beam kernels is the one the call asked for.

The kernels are built one object per input dtype and handed out through a table per object (lds_kernel<IO> / general_kernel<IO>,
csrc/ctc_beam_common.h); a wrong entry would still decode, plausibly.  Both kernels turn a frame's row into f64 as they load it,
so a call on f16, bf16 or f32 log-probabilities returns, bit for bit, what the same call returns on the f64 tensor that holds the
same numbers: ids, lengths, scores, counts and timestamps of the whole n-best list (np.array_equal, no tolerance).  The models
reach all nine LM kinds: none; the tiny 3-gram model on its signature tables and, with one context unlisted, on its id tables,
each plain or restricted to its lexicon, spelled or with homophones.  The general kernel takes the same cases in a child run
(E2E_BEAM_GENERAL is read once per process)."""
import os
import subprocess
import sys
import warnings

import pytest
import torch

import stream_util as S
from end2end_amd import _lib
from end2end_amd.engines import LanguageModel

pytestmark = pytest.mark.gpu
ARPA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tiny_3gram.arpa")
B, T, V, W, NBEST = 2, 12, 6, 4, 4
XLEN = [12, 9]
SPELLED = ["_", "a", "b", " ", "c", "'"]
TRANSCRIBED = ["_", "p", "q", "r", " ", "s"]
# `ab` and `b` share the transcription "p q": homophones, chosen by the model
ENTRIES = [("a", "p"), ("ab", "p q"), ("b", "p q"), ("ba", "q p"), ("ba", "r")]
KW = dict(lmwt=0.7, wip=0.5, oov_penalty=-3.0)
DTYPES = {"f64": torch.float64, "f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
MODELS = ["none"] + [t + h + r for t in ("signatures", "id-tables") for h in ("", "-homophones") for r in ("", "-restricted")]


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    """name -> (labels, model, restrict)"""
    src = open(ARPA).read()
    pruned = src.replace("-0.6\ta b\t-0.2\n", "").replace("ngram 2=5", "ngram 2=4")     # `a b a` stays: its context is unlisted
    assert pruned != src
    path = str(tmp_path_factory.mktemp("lm") / "pruned.arpa")
    open(path, "w").write(pruned)
    out = {"none": (SPELLED, None, False)}
    for tables, arpa in (("signatures", ARPA), ("id-tables", path)):
        for restrict in (False, True):
            r = "-restricted" if restrict else ""
            out[tables + r] = (SPELLED, LanguageModel(arpa, SPELLED, True, lexicon=restrict), restrict)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                hom = LanguageModel(arpa, TRANSCRIBED, True, transcriptions=ENTRIES, blank_idx=0, lexicon=restrict)
            out[tables + "-homophones" + r] = (TRANSCRIBED, hom, restrict)
    return out


def log_probs():
    """(B,T,V) f64 whose every value is a bf16 number and an f16 number: the four dtypes hold the same numbers"""
    g = torch.Generator().manual_seed(7100)
    lp = torch.log_softmax(torch.randn(B, T, V, generator=g, dtype=torch.float64) * 2.0, -1).to(torch.bfloat16)
    for dt in DTYPES.values():
        assert torch.equal(lp.to(dt).double(), lp.double()), dt
    return lp.double()


_whole = {}


def whole_call(models, model, dtype):
    """The n-best read-out of the whole utterances, once per (model, dtype); the expected kernel took the call."""
    if (model, dtype) not in _whole:
        labels, lm, restrict = models[model]
        general = _lib.load().e2e_ctc_beam_stream_workspace_bytes(B, V, W, 1 if lm is not None else 0) > 0
        assert general == bool(os.environ.get("E2E_BEAM_GENERAL"))
        _whole[model, dtype] = S.reference(log_probs().to(DTYPES[dtype]), XLEN, 0, W, labels, lm, restrict, nbest=NBEST, **KW)
    return _whole[model, dtype]


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_a_call_returns_the_f64_calls_bits(dtype, model, models):
    # (the f64 call is held to the f32 one: every case compares the instances of two objects)
    r, ref = whole_call(models, model, dtype), whole_call(models, model, "f32" if dtype == "f64" else "f64")
    assert (r["n_hyp"] >= 1).all() and (r["n_hyp"] <= NBEST).all() and (r["lens"][:, 0] >= 1).all(), (r["n_hyp"], r["lens"])
    S.same(r, ref, (dtype, model))


@pytest.mark.parametrize("model", ["none", "signatures"])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_a_stream_in_two_chunks_returns_the_f64_calls_bits(dtype, model, models):
    labels, lm, restrict = models[model]
    lp = log_probs().to(DTYPES[dtype])
    s = S.RawStream(B, T, V, W, labels, 0, lm, restrict, **KW)
    s.feed(lp[:, :7], [7, 7], nbest=NBEST)
    r = s.feed(lp[:, 7:], [n - 7 for n in XLEN], nbest=NBEST)
    assert r["done"].tolist() == XLEN
    S.same(r, whole_call(models, model, "f64"), (dtype, model))


def test_both_through_the_general_kernel():
    if os.environ.get("E2E_BEAM_GENERAL"):
        pytest.skip("already inside the child run")
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-k", "f64_calls_bits"],
                         env=dict(os.environ, E2E_BEAM_GENERAL="1"), capture_output=True, text=True, timeout=600,
                         cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
