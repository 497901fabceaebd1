"""-m gpu: the beam search over a model with custom transcriptions (e2e_lm_load_transcriptions).  An identity lexicon and a
relabelling are held bit for bit to the model that spells its words; homophones are held to the checker
tests/transcription_ref.py (the whole n-best list), to the definition (exhaustive beams), through both kernels and both LM
walks, in chunks (bit for bit against the whole call) and through the module.  f64 against f64: nbest_util.ATOL."""
import os
import warnings

import numpy as np
import pytest
import torch

import gpu_util as U
import lexicon_ref as LR
import nbest_util as NB
import oracle_lib as O
import stream_util as S
import test_gpu_lexicon as GL
import transcription_ref as TR
from end2end_amd.engines import LanguageModel

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ARPA = os.path.join(GOLD, "tiny_3gram.arpa")
LABELS4 = ["_", "a", "b", " "]
LABELS5 = ["_", "p", "q", "r", " "]
XLEN3 = [25, 22, 12]
TINY = ["a", "ab", "b", "ba"]
# `ab` and `b` collide on "p q" (the model prefers ab at the start of a sentence, b behind a); ba has two variants; zz is
# outside the model; `q` alone is a prefix and no word
ENTRIES = [("a", "p"), ("ab", "p q"), ("b", "p q"), ("ba", "q p"), ("ba", "r"), ("zz", "q q")]
KEYS = ("ids", "lens", "n_hyp", "scores", "counts", "ts")


def transcribed(path, labels, entries, lexicon=False, case_sensitive=True):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return LanguageModel(path, labels, case_sensitive, transcriptions=entries, blank_idx=0, lexicon=lexicon)


def against_checker(lp, x_len, W, labels, lm, ref_lm, table, restrict, skips, **kw):
    ref, gap = TR.beam(lp.double().numpy(), x_len, 0, W, labels, ref_lm, table, restrict, kw.get("lmwt", 1.0), kw.get("wip", 0.0),
                       kw.get("oov_penalty", -1000.0))
    if not skips.take(gap):
        return None, ref
    r = GL.nbest_opt(lp, x_len, 0, W, labels, lm, restrict, **kw)
    GL.same_as_checker(r, ref, (W, restrict, kw))
    return r, ref


# ---- 1. an identity lexicon is the model that spells its words, bit for bit ----
_identity = {}


def identity_results(model, W, restrict):
    """The plain model's read-out of the shared utterances, once per (model, W, restrict)."""
    key = (model, W, restrict)
    if key not in _identity:
        lm = (LanguageModel(ARPA, LABELS4, True, lexicon=True) if model == "tiny_3gram"
              else LanguageModel(None, LABELS4, True, words=TINY, lexicon=True))
        _identity[key] = GL.nbest_opt(GL.rand_lp(6100, 3, 25, 4), XLEN3, 0, W, LABELS4, lm, restrict, timesteps=True, **IDENTITY_KW)
    return _identity[key]


IDENTITY_KW = dict(lmwt=0.7, wip=0.5, oov_penalty=-3.0)


@pytest.mark.parametrize("restrict", [False, True])
@pytest.mark.parametrize("W", [3, 10, 100])
@pytest.mark.parametrize("model", ["tiny_3gram", "word_list"])
def test_identity_lexicon_changes_nothing(model, W, restrict):
    lm = transcribed(ARPA if model == "tiny_3gram" else None, LABELS4, [(w, list(w)) for w in TINY], lexicon=True)
    got = GL.nbest_opt(GL.rand_lp(6100, 3, 25, 4), XLEN3, 0, W, LABELS4, lm, restrict, timesteps=True, **IDENTITY_KW)
    want = identity_results(model, W, restrict)
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), k
    assert (want["counts"][:, 0, 0] > 0).any()


# ---- 2. the same log-probabilities under other label strings ----
@pytest.mark.parametrize("restrict", [False, True])
def test_relabelling_is_the_same_search(restrict):
    labels = ["_", "X1", "Y2", " "]
    entries = [(w, [{"a": "X1", "b": "Y2"}[c] for c in w]) for w in TINY]
    lm = transcribed(ARPA, labels, entries, lexicon=True)
    lp = GL.rand_lp(6100, 3, 25, 4)
    for W in (3, 10):
        got = GL.nbest_opt(lp, XLEN3, 0, W, labels, lm, restrict, timesteps=True, **IDENTITY_KW)
        want = identity_results("tiny_3gram", W, restrict)
        for k in KEYS:
            assert np.array_equal(got[k], want[k]), (W, k)
    from end2end_amd import CTCDecoder
    kw = dict(beam_width=10, lm_path=ARPA, after_logsoftmax=True, restrict_to_vocabulary=restrict, lmwt=0.7, wip=0.5, oov_penalty=-3.0)
    x, xl = lp.to(U.dev()), torch.tensor(XLEN3)
    spelled = CTCDecoder(labels=LABELS4, **kw).decode_nbest(x, xl, nbest=5)
    worded = CTCDecoder(labels=labels, transcriptions=entries, **kw).decode_nbest(x, xl, nbest=5)
    assert torch.equal(spelled.decoded_targets, worded.decoded_targets) and torch.equal(spelled.scores, worded.scores)
    for row_s, row_w in zip(spelled.decoded_sentences, worded.decoded_sentences):
        assert len(row_s) == len(row_w) > 0
        for s, w in zip(row_s, row_w):
            assert [t if t in TINY else "<unk>" for t in s.split()] == w.split() and w == " ".join(w.split())


# ---- 3. homophones against the checker: the whole ranked list ----
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("restrict", [False, True])
def test_homophones_tiny_3gram(restrict, dtype):
    lm = transcribed(ARPA, LABELS5, ENTRIES, lexicon=restrict)
    olm = O.OracleLM(ARPA)
    table, skips = TR.Table(ENTRIES, LABELS5, olm), GL.Skips()
    assert lm.transcriptions_dropped() == table.dropped == 1
    chosen = set()
    for seed in range(3):
        lp = GL.rand_lp(6300 + seed, 3, 25, 5, dtype=dtype)
        for W in (3, 10):
            for kw in (dict(lmwt=0.7, wip=0.5, oov_penalty=-3.0), dict(lmwt=1.5, wip=0.0, oov_penalty=0.0)):
                r, ref = against_checker(lp, XLEN3, W, LABELS5, lm, olm, table, restrict, skips, **kw)
                for h in ref[0] + ref[1] + ref[2]:
                    chosen |= set(TR.words_of([k for k in h["ids"] if k >= 0], LABELS5, olm, table))
    skips.done()
    assert {olm.word_index("ab"), olm.word_index("b")} <= chosen            # both words of the shared key were chosen somewhere


def order4_entries(words):
    """Two words per transcription over p, q, r: of one, two and three labels, so keys are prefixes of other keys."""
    out = []
    for i, w in enumerate(words):
        k = i // 2
        toks = [k] if k < 3 else [(k - 3) // 3, (k - 3) % 3] if k < 12 else [(k - 12) // 9 % 3, (k - 12) // 3 % 3, (k - 12) % 3]
        out.append((w, [LABELS5[1 + t] for t in toks]))
    return out


@pytest.mark.parametrize("restrict", [False, True])
def test_homophones_order_4_model_takes_the_general_lm_walk(restrict):
    path = os.path.join(GOLD, "lm_order4.arpa")
    entries = order4_entries(LR.arpa_words(path))
    lm = transcribed(path, LABELS5, entries, lexicon=restrict)
    assert lm.order() == 4 and lm.transcriptions_dropped() == 0
    olm = O.OracleLM(path)
    table, skips = TR.Table(entries, LABELS5, olm), GL.Skips()
    assert max(len(v) for v in table.keys.values()) == 2
    g = torch.Generator().manual_seed(6400)
    x = torch.randn(3, 25, 5, generator=g, dtype=torch.float64) * 1.5
    x[:, :, 4] += 1.0
    lp = torch.log_softmax(x, -1)
    for W in (3, 10):
        against_checker(lp, XLEN3, W, LABELS5, lm, olm, table, restrict, skips, lmwt=0.7, wip=0.5, oov_penalty=-2.0)
    skips.done()


@pytest.mark.parametrize("restrict", [False, True])
def test_homophones_unlisted_context_takes_the_id_tables(restrict, tmp_path):
    src = open(ARPA).read()
    pruned = src.replace("-0.6\ta b\t-0.2\n", "").replace("ngram 2=5", "ngram 2=4")
    assert pruned != src
    path = str(tmp_path / "pruned.arpa")
    open(path, "w").write(pruned)
    lm = transcribed(path, LABELS5, ENTRIES, lexicon=restrict)
    olm = O.OracleLM(path)
    table, skips = TR.Table(ENTRIES, LABELS5, olm), GL.Skips()
    lp = GL.rand_lp(6500, 3, 25, 5)
    for W in (3, 10):
        against_checker(lp, XLEN3, W, LABELS5, lm, olm, table, restrict, skips, lmwt=0.7, wip=0.5, oov_penalty=-3.0)
    skips.done()


# ---- 4. exhaustive beams: exactly the labellings rule 4 allows ----
def legal(seq, space_id, table):
    word, inside = (), False
    for k in seq:
        if k == space_id:
            if inside and word not in table.keys:
                return False
            inside = False
        else:
            word = (word if inside else ()) + (k,)
            inside = True
            if word not in table.prefixes:
                return False
    return True


@pytest.mark.parametrize("model", ["word_list", "tiny_3gram"])
@pytest.mark.parametrize("name", GL.SPACE_CASES)
def test_exhaustive_restricted_beam_is_exactly_the_legal_labellings(name, model):
    c = next(c for c in NB.exhaustive_cases() if c["name"] == name)
    W, blank, labels, sp = c["beam_width"], c["blank"], c["labels"], c["space_id"]
    letters = [l for i, l in enumerate(labels) if i not in (blank, sp)]
    x, y = letters[0], letters[-1]
    shapes = [[x], [x, y], [x, y], [y, y], [y, x, x]] if len(letters) > 1 else [[x], [x, x, x], [x, x, x], [x] * 5, [x] * 5]
    if model == "word_list":
        entries = list(zip(["one", "two", "too", "three", "four"], shapes))
        ref_lm = LR.WordListLM([w for w, _ in entries])
        path, kw = None, dict(lmwt=0.0, wip=0.0, oov_penalty=-1.0)
    else:
        entries = list(zip(["a", "ab", "b", "ba", "zz"], shapes))
        ref_lm = O.OracleLM(ARPA)
        path, kw = ARPA, dict(lmwt=0.7, wip=0.5, oov_penalty=-2.0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        lm = LanguageModel(path, labels, True, transcriptions=entries, blank_idx=blank, lexicon=True)
    table = TR.Table(entries, labels, ref_lm)
    want = {s: l for s, l in zip(c["seqs"], c["ll"]) if legal(s, sp, table)}
    assert 3 <= len(want) < len(c["seqs"])
    r = GL.nbest_opt(torch.from_numpy(c["lp"])[None], None, blank, W, labels, lm, True, **kw)
    nh = int(r["n_hyp"][0])
    got = [NB.hypothesis(r, 0, h) for h in range(nh)]
    assert sorted(got) == sorted(want)                                   # every legal labelling exactly once, no other
    for h, seq in enumerate(got):
        tot, ctc, lms = r["scores"][0, h]
        words = TR.words_of(seq, labels, ref_lm, table)
        assert r["counts"][0, h].tolist() == [len(words), sum(w == 0 for w in words)], seq
        assert sum(w == 0 for w in words) <= 1                           # only the last word can be unfinished
        assert np.isfinite(ctc) == np.isfinite(want[seq]), seq
        if np.isfinite(ctc):
            assert abs(ctc - want[seq]) <= NB.ATOL, (seq, ctc, want[seq])
            assert GL.close(tot, ctc + kw["lmwt"] * lms - kw["wip"] * len(words) + kw["oov_penalty"] * sum(w == 0 for w in words)), seq
    tots = r["scores"][0, :nh, 0]
    assert (tots[:-1] >= tots[1:]).all()


# ---- 5. the general kernel, natively ----
# (restricted, as the lexicon test's shapes are: the restriction keeps the Python checker's beam of 100 to 256 members, V
#  candidates each, within a second; unrestricted, the checker affords the general kernel six frames)
@pytest.mark.parametrize("V,W,T,B,restrict", [(100, 100, 20, 2, True), (300, 256, 12, 1, True), (100, 100, 6, 1, False)],
                         ids=["members_in_lds", "members_in_workspace", "unrestricted"])
def test_homophones_general_kernel(V, W, T, B, restrict):
    labels = ["_"] + ["w%d" % i for i in range(V - 2)] + [" "]
    entries = [("a", "w0"), ("ab", "w1 w17"), ("b", "w1 w17"), ("ba", "w17 w1"), ("ba", "w2 w2 w3"), ("ab", "w2 w2 w3"),
               ("a", "w2 w2 w3"), ("b", "w2"), ("zz", "w4")]
    lm = transcribed(ARPA, labels, entries, lexicon=restrict)
    olm = O.OracleLM(ARPA)
    table, skips = TR.Table(entries, labels, olm), GL.Skips()
    assert max(len(v) for v in table.keys.values()) == 3
    g = torch.Generator().manual_seed(6600 + V)
    x = torch.randn(B, T, V, generator=g, dtype=torch.float64)
    x[:, :, [1, 2, 3, 4, 18]] += 3.0                                       # the labels the words are made of
    x[:, :, V - 1] += 3.0
    lp = torch.log_softmax(x, -1)
    r, ref = against_checker(lp, [T, T - 3][:B], W, labels, lm, olm, table, restrict, skips, lmwt=0.7, wip=0.5, oov_penalty=-2.0)
    assert max(h["words"] for h in ref[0]) >= 2 and len(ref[0]) > 10
    skips.done()


# ---- 6. streaming: chunks of 1, 7 and the rest, bit for bit the whole call after every chunk ----
@pytest.mark.parametrize("restrict", [False, True])
def test_streaming_a_homophone_model(restrict):
    lm = transcribed(ARPA, LABELS5, ENTRIES, lexicon=restrict)
    lp = GL.rand_lp(6300, 3, 25, 5)
    chunking, fed = [], [0, 0, 0]
    for size in (1, 7, 25):
        lens = [min(size, n - f) for n, f in zip(XLEN3, fed)]
        chunking.append(lens)
        fed = [f + n for f, n in zip(fed, lens)]
    assert fed == XLEN3
    for W in (3, 10):
        r = S.check_stream(lp, XLEN3, chunking, 0, W, LABELS5, lm=lm, restrict=restrict, oracle=False, lmwt=0.7, wip=0.5,
                           oov_penalty=-3.0)
        assert (r["counts"][:, 0, 0] > 0).any()


# ---- 7. module ----
def test_module_renders_the_chosen_words(tmp_path):
    from end2end_amd import CTCDecoder
    p = tmp_path / "lexicon.txt"
    p.write_text("".join("%s %s\n" % e for e in ENTRIES))
    kw = dict(beam_width=10, labels=LABELS5, lm_path=ARPA, after_logsoftmax=True, lmwt=0.7, wip=0.5, oov_penalty=-3.0)
    with pytest.warns(UserWarning, match="1 of 6 entries dropped"):
        dec = CTCDecoder(transcriptions=str(p), **kw)
    olm = O.OracleLM(ARPA)
    table = TR.Table(ENTRIES, LABELS5, olm)
    name = {olm.word_index(w): w for w in TINY}
    name[0] = "<unk>"

    def rendered(ids):
        ids = [int(k) for k in ids if int(k) >= 0]
        return " ".join(name[w] for w in TR.words_of(ids, LABELS5, olm, table))

    lp = GL.rand_lp(6300, 3, 25, 5)
    peaks = torch.zeros(12, 5, dtype=torch.float64)                       # utterance 2 says `p space p q`: the words a b
    peaks[torch.arange(12), torch.tensor([1, 0, 4, 0, 1, 0, 2, 0, 0, 0, 0, 0])] = 8.0
    lp[2, :12] = torch.log_softmax(peaks, -1)
    lp = lp.to(U.dev())
    xl = torch.tensor(XLEN3)
    one = dec.decode(lp, xl)
    assert one.decoded_sentences[2] == "a b"
    res = dec.decode_nbest(lp, xl, nbest=10)
    assert [row[0] for row in res.decoded_sentences] == one.decoded_sentences
    seen = set()
    for b in range(3):
        for h, s in enumerate(res.decoded_sentences[b]):
            ids = res.decoded_targets[b, h, : int(res.decoded_targets_lengths[b, h])].tolist()
            assert s == rendered(ids) == " ".join(dec.transcribe(ids)), (b, h, ids, s)
            assert len(s.split()) == int(res.num_words[b, h]) and s.split().count("<unk>") == int(res.num_oov_words[b, h])
            seen |= set(s.split())
    assert {"<unk>", "ab", "b"} <= seen                                    # an unfinished last word; both homophones
    # a stream renders the same words after every chunk
    st = dec.open_stream(3, 25)
    st.feed(lp[:, :9], torch.tensor([9, 9, 9]))
    last = st.feed_nbest(lp[:, 9:], torch.tensor([16, 13, 3]), nbest=10)
    assert last.decoded_sentences == res.decoded_sentences
    # restricted to the transcriptions: every word but an unfinished last one is a word of the lexicon
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rdec = CTCDecoder(transcriptions=ENTRIES, restrict_to_vocabulary=True, **kw)
        alone = CTCDecoder(transcriptions=ENTRIES, **{k: v for k, v in kw.items() if k != "lm_path"})
    rr = rdec.decode_nbest(lp, xl, nbest=10)
    assert all("<unk>" not in s.split()[:-1] for row in rr.decoded_sentences for s in row)
    assert rr.decoded_sentences != res.decoded_sentences
    # the other searches refuse transcriptions: Gram-CTC at construction, ASG in e2e_asg_beam_nbest (tests/test_transcriptions_cpu.py)
    from end2end_amd import CTCDecoderError, GramCTCDecoder
    with pytest.raises(CTCDecoderError, match="custom transcriptions"):
        GramCTCDecoder(num_base_labels=3, total_labels=3, transcriptions=ENTRIES)
    # alone: the model that scores nothing, the first listed homophone every time
    words = {w for s in alone.decode(lp, xl).decoded_sentences for w in s.split()}
    assert words and "b" not in words and words <= {"a", "ab", "ba", "zz", "<unk>"}


def test_a_restricted_call_without_the_lexicon_launches_nothing():
    from end2end_amd import _lib
    L = _lib.load()
    lm = transcribed(ARPA, LABELS5, ENTRIES)
    # restricted without e2e_lm_enable_lexicon: E2E_ERR_ARG, nothing launched, nothing written
    r = GL.nbest_opt(GL.rand_lp(6700, 2, 10, 5), None, 0, 5, LABELS5, lm, True, timesteps=True, expect_rc=-1)
    assert (r["ids"] == -7).all() and (r["lens"] == -7).all() and (r["n_hyp"] == -7).all() and (r["scores"] == 7.0).all()
    assert b"no lexicon" in L.e2e_last_error()
