"""-m gpu: the beam search restricted to a vocabulary (e2e_ctc_beam_nbest_opt with restrict_to_lexicon) against the definition
(exhaustive beams), against the checker tests/lexicon_ref.py (pruned beams: the whole n-best list), against the C oracle
where nothing can be forbidden, and through the module.  Every number is f64 against f64: nbest_util.ATOL, relative above 1."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gpu_util as U
import lexicon_ref as LR
import nbest_util as NB
import oracle_lib as O
from end2end_amd.engines import LanguageModel

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ARPA = os.path.join(GOLD, "tiny_3gram.arpa")
ATOL = NB.ATOL
LABELS4 = ["_", "a", "b", " "]
XLEN3 = [25, 22, 12]
TINY = ["a", "ab", "b", "ba"]


def rand_lp(seed, B, T, V, sharp=1.5, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    return torch.log_softmax(torch.randn(B, T, V, generator=g, dtype=torch.float64) * sharp, -1).to(dtype)


def nbest_opt(lp, x_len=None, blank=0, W=100, labels=None, lm=None, restrict=True, lmwt=1.0, wip=0.0, oov_penalty=-1000.0,
              nbest=None, timesteps=False, null_opts=False, expect_rc=0):
    """e2e_ctc_beam_nbest_opt through ctypes -> the dict of nbest_util.c_abi_beam_nbest.  Outputs start as -7 / 7.0."""
    from end2end_amd import _lib
    L = _lib.load()
    d = U.dev()
    lp = lp.to(d)
    B, T, V = lp.shape
    xl = torch.as_tensor(np.asarray([T] * B if x_len is None else x_len)).to(d, torch.long)
    labels = list(labels or [])
    space_id = labels.index(" ") if " " in labels else -1
    N = W if nbest is None else nbest
    max_out = T + 1
    out = torch.full((B, N, max_out), -7, dtype=torch.long, device=d)
    out_len = torch.full((B, N), -7, dtype=torch.long, device=d)
    n_hyp = torch.full((B,), -7, dtype=torch.long, device=d)
    scores = torch.full((B, N, 3), 7.0, dtype=torch.float64, device=d)
    counts = torch.full((B, N, 2), -7, dtype=torch.int32, device=d)
    ts = torch.full((B, N, max_out), -7, dtype=torch.long, device=d) if timesteps else None
    ws = torch.empty(L.e2e_ctc_beam_nbest_workspace_bytes(B, T, V, W, 1, 1 if timesteps else 0), dtype=torch.uint8, device=d)
    opts = _lib.BeamOpts(1 if restrict else 0)
    sB, sT, sV = lp.stride()
    rc = L.e2e_ctc_beam_nbest_opt(lp.data_ptr(), _lib.dtype_code(lp.dtype), sB, sT, sV, xl.data_ptr(), B, T, V, blank,
                                  W, space_id, lm.on(d).handle if lm is not None else None, lmwt, wip, oov_penalty,
                                  N, out.data_ptr(), max_out, out_len.data_ptr(), n_hyp.data_ptr(), scores.data_ptr(),
                                  counts.data_ptr(), ts.data_ptr() if timesteps else None,
                                  ws.data_ptr(), ws.numel(), _lib.stream_ptr(d), None if null_opts else C.byref(opts))
    assert rc == expect_rc, (rc, L.e2e_last_error())
    torch.cuda.synchronize()
    r = dict(ids=out.cpu().numpy(), lens=out_len.cpu().numpy(), n_hyp=n_hyp.cpu().numpy(), scores=scores.cpu().numpy(),
             counts=counts.cpu().numpy(), ts=ts.cpu().numpy() if timesteps else None)
    if rc == 0:
        assert (r["n_hyp"] >= 1).all() and (r["n_hyp"] <= N).all(), r["n_hyp"]
        assert ((r["lens"] >= 0) & (r["lens"] <= max_out)).all()
    return r


def raw_ids(r, b, h):
    return tuple(int(k) for k in r["ids"][b, h, : r["lens"][b, h]])


def close(a, b):
    return a == b or abs(a - b) <= ATOL * max(1.0, abs(b))


def same_as_checker(r, ref, what):
    """The whole list of every utterance: ids, the three scores, the two counts; empty slots behind it."""
    for b, want in enumerate(ref):
        N = r["ids"].shape[1]
        assert r["n_hyp"][b] == min(N, len(want)), (what, b, r["n_hyp"][b], len(want))
        for h, w in enumerate(want[:N]):
            assert raw_ids(r, b, h) == w["ids"], (what, b, h, raw_ids(r, b, h), w["ids"])
            tot, ctc, lms = r["scores"][b, h]
            assert close(tot, w["total"]) and close(ctc, w["ctc"]) and close(lms, w["lm"]), (what, b, h, r["scores"][b, h], w)
            assert r["counts"][b, h].tolist() == [w["words"], w["oov"]], (what, b, h)
        assert (r["lens"][b, len(want):] == 0).all()


class Skips:
    """A call whose smallest positive cut gap is below 1e-9 may be skipped (f64 round-off could order the cut either way); at
    most 2 % of a test's calls."""

    def __init__(self):
        self.calls = self.skipped = 0

    def take(self, gap):
        self.calls += 1
        if gap < 1e-9:
            self.skipped += 1
            return False
        return True

    def done(self):
        assert self.calls > 0 and self.skipped <= 0.02 * self.calls, (self.skipped, self.calls)


def against_checker(lp, x_len, blank, W, labels, lm, ref_lm, lexicon, skips, case_sensitive=True, timesteps=False, **kw):
    ref, gap = LR.beam(lp.double().numpy(), x_len, blank, W, labels, ref_lm, case_sensitive, kw.get("lmwt", 1.0),
                       kw.get("wip", 0.0), kw.get("oov_penalty", -1000.0), lexicon=lexicon)
    if not skips.take(gap):
        return None, ref
    r = nbest_opt(lp, x_len, blank, W, labels, lm, True, timesteps=timesteps, **kw)
    same_as_checker(r, ref, (W, kw))
    return r, ref


# ---- 1. exhaustive beams: exactly the labellings the definition allows ----
def legal(seq, labels, space_id, lx):
    """The rule, from the definition: every prefix of the labelling was created legally."""
    word, inside = b"", False
    for k in seq:
        if k == space_id:
            if inside and lx.fold(word) not in lx.words:
                return False
            inside = False
        else:
            word = (word if inside else b"") + labels[k].encode()
            inside = True
            if lx.fold(word) not in lx.prefixes:
                return False
    return True


def counts_of(seq, labels, space_id, lx):
    words = "".join(labels[k] for k in seq).split()
    return len(words), sum(lx.fold(w.encode()) not in lx.words for w in words)


SPACE_CASES = [c["name"] for c in NB.exhaustive_cases() if c["space_id"] >= 0]


@pytest.mark.parametrize("model", ["word_list", "tiny_3gram"])
@pytest.mark.parametrize("name", SPACE_CASES)
def test_exhaustive_restricted_beam_is_exactly_the_legal_labellings(name, model):
    c = next(c for c in NB.exhaustive_cases() if c["name"] == name)
    W, blank, labels, sp = c["beam_width"], c["blank"], c["labels"], c["space_id"]
    letters = [l for i, l in enumerate(labels) if i not in (blank, sp)]
    if model == "word_list":
        x, y = letters[0], letters[-1]
        words = [x, x + y, y + y, y + x + x] if len(letters) > 1 else [x, x * 3, x * 5]
        lm = LanguageModel(None, labels, True, words=words, lexicon=True)
        kw = dict(lmwt=0.0, wip=0.0, oov_penalty=0.0)
    else:
        words = TINY
        lm = LanguageModel(ARPA, labels, True, lexicon=True)
        kw = dict(lmwt=0.7, wip=0.5, oov_penalty=-2.0)
    lx = LR.Lexicon(words)
    want = {s: l for s, l in zip(c["seqs"], c["ll"]) if legal(s, labels, sp, lx)}
    assert 3 <= len(want) < len(c["seqs"])
    r = nbest_opt(torch.from_numpy(c["lp"])[None], None, blank, W, labels, lm, True, **kw)
    nh = int(r["n_hyp"][0])
    got = [NB.hypothesis(r, 0, h) for h in range(nh)]
    assert sorted(got) == sorted(want)                                   # every legal labelling exactly once, no other
    place = {}
    for h, seq in enumerate(got):
        tot, ctc, lms = r["scores"][0, h]
        nw, no = counts_of(seq, labels, sp, lx)
        assert r["counts"][0, h].tolist() == [nw, no], seq
        assert no <= 1                                                   # only the last word can be unfinished
        assert np.isfinite(ctc) == np.isfinite(want[seq]), seq
        if np.isfinite(ctc):
            assert abs(ctc - want[seq]) <= ATOL, (seq, ctc, want[seq])
            assert close(tot, ctc + kw["lmwt"] * lms - kw["wip"] * nw + kw["oov_penalty"] * no), seq
            place[seq] = h
    tots = r["scores"][0, :nh, 0]
    assert (tots[:-1] >= tots[1:]).all()
    if model == "word_list":                                             # ranked by likelihood alone
        fin = sorted(((l, s) for s, l in want.items() if np.isfinite(l)), key=lambda e: -e[0])
        assert sorted(place.values()) == list(range(len(fin)))
        for (l0, s0), (l1, s1) in zip(fin[:-1], fin[1:]):
            if l0 - l1 > 1e-6:
                assert place[s0] < place[s1], (s0, l0, s1, l1)


def test_exhaustive_through_the_general_kernel():
    if os.environ.get("E2E_BEAM_GENERAL"):
        pytest.skip("already inside the child run")
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-k",
                          "exhaustive_restricted"], env=dict(os.environ, E2E_BEAM_GENERAL="1"), capture_output=True,
                         text=True, timeout=600, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]


# ---- 2. pruned beams: the whole list is the checker's ----
def test_pruned_v4_word_list():
    lm = LanguageModel(None, LABELS4, True, words=TINY, lexicon=True)
    ref_lm, lx, skips = LR.WordListLM(TINY), LR.Lexicon(TINY), Skips()
    for seed in range(5):
        lp = rand_lp(4100 + seed, 3, 25, 4)
        for W in (2, 3, 10, 30):
            for wip in (0.0, 1.0):
                against_checker(lp, XLEN3, 0, W, LABELS4, lm, ref_lm, lx, skips, lmwt=0.0, wip=wip, oov_penalty=0.0)
    skips.done()


def test_pruned_v4_language_model_and_the_restriction_changes_the_result():
    lm = LanguageModel(ARPA, LABELS4, True, lexicon=True)
    ref_lm, lx, skips = O.OracleLM(ARPA), LR.Lexicon(TINY), Skips()
    differ = total = 0
    for seed in range(5):
        lp = rand_lp(4200 + seed, 3, 25, 4)
        for W in (2, 3, 10, 30):
            for lmwt, wip, oov in ((0.7, 0.5, 0.0), (0.0, 0.0, 0.0)):
                kw = dict(lmwt=lmwt, wip=wip, oov_penalty=oov)
                r, _ = against_checker(lp, XLEN3, 0, W, LABELS4, lm, ref_lm, lx, skips, **kw)
                if r is None:
                    continue
                u = nbest_opt(lp, XLEN3, 0, W, LABELS4, lm, False, **kw)
                for b in range(3):
                    total += 1
                    differ += raw_ids(r, b, 0) != raw_ids(u, b, 0)
    skips.done()
    assert differ >= 0.25 * total, (differ, total)                        # not vacuous


def test_pruned_f32_input_and_timestamps():
    lm = LanguageModel(ARPA, LABELS4, True, lexicon=True)
    ref_lm, lx, skips = O.OracleLM(ARPA), LR.Lexicon(TINY), Skips()
    lp = rand_lp(4300, 3, 25, 4, dtype=torch.float32)
    for W in (3, 30):
        r, _ = against_checker(lp, XLEN3, 0, W, LABELS4, lm, ref_lm, lx, skips, timesteps=True, lmwt=0.7, wip=0.5, oov_penalty=0.0)
        for b in range(3):
            for h in range(int(r["n_hyp"][b])):
                n = int(r["lens"][b, h])
                ts = r["ts"][b, h]
                assert (ts[n:] == -1).all()
                if raw_ids(r, b, h) == (-1,):
                    assert ts[0] == -1
                else:
                    assert (ts[:n] >= 0).all() and (ts[:n] < XLEN3[b]).all() and (np.diff(ts[:n]) > 0).all(), (b, h, ts[:n])
    skips.done()


LABELS8 = ["_", "a", "b", "c", "d", "e", "'", " "]


def test_pruned_order_4_model_takes_the_general_lm_walk():
    path = os.path.join(GOLD, "lm_order4.arpa")
    lm = LanguageModel(path, LABELS8, True, lexicon=True)
    assert lm.order() == 4
    ref_lm, lx, skips = O.OracleLM(path), LR.Lexicon(LR.arpa_words(path)), Skips()
    g = torch.Generator().manual_seed(4400)
    x = torch.randn(3, 25, 8, generator=g, dtype=torch.float64) * 1.5
    x[:, :, 7] += 1.0
    lp = torch.log_softmax(x, -1)
    for W in (10, 30):
        against_checker(lp, XLEN3, 0, W, LABELS8, lm, ref_lm, lx, skips, lmwt=0.7, wip=0.5, oov_penalty=0.0)
    skips.done()


def test_pruned_model_with_an_unlisted_context_takes_the_id_tables(tmp_path):
    src = open(ARPA).read()
    pruned = src.replace("-0.6\ta b\t-0.2\n", "").replace("ngram 2=5", "ngram 2=4")
    assert pruned != src
    path = str(tmp_path / "pruned.arpa")
    open(path, "w").write(pruned)
    lm = LanguageModel(path, LABELS4, True, lexicon=True)
    ref_lm, lx, skips = O.OracleLM(path), LR.Lexicon(TINY), Skips()
    lp = rand_lp(4500, 3, 25, 4)
    for W in (3, 30):
        against_checker(lp, XLEN3, 0, W, LABELS4, lm, ref_lm, lx, skips, lmwt=0.7, wip=0.5, oov_penalty=0.0)
    skips.done()


def test_pruned_case_folding():
    labels = ["_", "A", "B", " "]
    lm = LanguageModel(ARPA, labels, False, lexicon=True)
    ref_lm, lx, skips = O.OracleLM(ARPA), LR.Lexicon(TINY, case_sensitive=False), Skips()
    lp = rand_lp(4600, 3, 25, 4)
    for W in (3, 30):
        against_checker(lp, XLEN3, 0, W, labels, lm, ref_lm, lx, skips, case_sensitive=False, lmwt=0.7, wip=0.5, oov_penalty=0.0)
    skips.done()


def test_pruned_without_a_space_label():
    labels = ["_", "a", "b", "c"]
    words = ["ab", "abcab", "ca", "b", "cabbc"]
    lm = LanguageModel(None, labels, True, words=words, lexicon=True)
    ref_lm, lx, skips = LR.WordListLM(words), LR.Lexicon(words), Skips()
    lp = rand_lp(4700, 3, 25, 4)
    for W in (3, 30):
        r, ref = against_checker(lp, XLEN3, 0, W, labels, lm, ref_lm, lx, skips, lmwt=0.0, wip=1.0, oov_penalty=0.0)
        for h in ref[0]:
            assert h["ids"] == (-1,) or "".join(labels[k] for k in h["ids"]).encode() in lx.prefixes
    skips.done()


@pytest.mark.parametrize("V,W,T,B", [(100, 100, 20, 2), (300, 256, 12, 1)], ids=["members_in_lds", "members_in_workspace"])
def test_pruned_general_kernel(V, W, T, B):
    """Alphabets the one-workgroup kernel cannot hold; words of two and three labels `wN`, so a label boundary falls inside
    byte prefixes of other labels (w1 | w17)."""
    labels = ["_"] + ["w%d" % i for i in range(V - 2)] + [" "]
    rng = np.random.RandomState(V)
    words = sorted({"".join("w%d" % k for k in rng.randint(0, 12, size=rng.randint(2, 4))) for _ in range(60)})
    lm = LanguageModel(None, labels, True, words=words, lexicon=True)
    ref_lm, lx, skips = LR.WordListLM(words), LR.Lexicon(words), Skips()
    g = torch.Generator().manual_seed(4800 + V)
    x = torch.randn(B, T, V, generator=g, dtype=torch.float64)
    x[:, :, 1:13] += 3.0                                                   # the labels the words are made of
    x[:, :, V - 1] += 3.0
    lp = torch.log_softmax(x, -1)
    r, ref = against_checker(lp, [T, T - 3][:B], 0, W, labels, lm, ref_lm, lx, skips, lmwt=0.0, wip=0.5, oov_penalty=0.0)
    assert max(h["words"] for h in ref[0]) >= 2 and len(ref[0]) > 10
    skips.done()


# ---- 3. identities pinned to the C oracle ----
@pytest.mark.parametrize("W", [3, 10])
def test_a_lexicon_that_forbids_nothing_changes_nothing(W):
    labels, T = ["_", "a", " "], 40
    words = ["a" * n for n in range(1, T + 1)]
    lm = LanguageModel(None, labels, True, words=words, lexicon=True)
    lp = rand_lp(4900 + W, 3, T, 3)
    xl = [40, 31, 7]
    kw = dict(lmwt=0.0, wip=1.0, oov_penalty=0.0)
    r = nbest_opt(lp, xl, 0, W, labels, lm, True, **kw)
    u = nbest_opt(lp, xl, 0, W, labels, lm, False, **kw)
    for k in ("ids", "lens", "n_hyp", "scores", "counts"):
        assert np.array_equal(r[k], u[k]), k
    o_ids, o_lens, _ = O.ctc_beam(lp.numpy(), xl, 0, W, labels, None, wip=1.0)
    for b in range(3):
        assert list(raw_ids(r, b, 0)) == o_ids[b, : o_lens[b]].tolist()


def test_word_list_model_with_the_flag_off_is_the_search_without_a_model():
    lm = LanguageModel(None, LABELS4, True, words=TINY, lexicon=True)
    lp = rand_lp(5000, 3, 25, 4)
    for W in (3, 30):
        u = nbest_opt(lp, XLEN3, 0, W, LABELS4, lm, False, lmwt=2.0, wip=1.0, oov_penalty=0.0)
        ids, lens = U.c_abi_beam(lp, XLEN3, 0, W, LABELS4, None, wip=1.0)
        o_ids, o_lens, _ = O.ctc_beam(lp.numpy(), XLEN3, 0, W, LABELS4, None, wip=1.0)
        assert lens.tolist() == o_lens.tolist() == u["lens"][:, 0].tolist() and np.array_equal(ids, o_ids)
        assert np.array_equal(u["ids"][:, 0, : ids.shape[1]], ids)
        plain = NB.c_abi_beam_nbest(lp, XLEN3, 0, W, LABELS4, None, wip=1.0)
        assert np.array_equal(plain["scores"][:, :, 0], u["scores"][:, :, 0])          # bit for bit


def test_null_options_are_the_plain_nbest_call():
    plain_lm = LanguageModel(ARPA, LABELS4, True)
    lm = LanguageModel(ARPA, LABELS4, True, lexicon=True)
    lp = rand_lp(5100, 3, 25, 4)
    kw = dict(lmwt=0.7, wip=0.5, oov_penalty=-3.0)
    want = NB.c_abi_beam_nbest(lp, XLEN3, 0, 10, LABELS4, plain_lm, timesteps=True, **kw)
    for got in (nbest_opt(lp, XLEN3, 0, 10, LABELS4, lm, True, timesteps=True, null_opts=True, **kw),
                nbest_opt(lp, XLEN3, 0, 10, LABELS4, lm, False, timesteps=True, **kw),
                nbest_opt(lp, XLEN3, 0, 10, LABELS4, plain_lm, False, timesteps=True, **kw)):
        for k in ("ids", "lens", "n_hyp", "scores", "counts", "ts"):
            assert np.array_equal(got[k], want[k]), k


# ---- 4. module ----
def in_lexicon(sentence, lx):
    words = sentence.split()
    return all(w.encode() in lx.words for w in words[:-1]) and (not words or words[-1].encode() in lx.prefixes)


@pytest.mark.parametrize("keep", [False, True])
def test_module_decodes_inside_the_lexicon(keep, tmp_path):
    from end2end_amd import CTCDecoder
    from end2end_amd.engines import CTCDecoderEngine
    labels = ["_", "a", "b", "c", " ", "d", "'"]
    words = ["ab", "abc", "cab", "d", "dad", "b'd"]
    lx = LR.Lexicon(words)
    p = tmp_path / "lexicon.txt"
    p.write_text("".join("%s  P R O N\n" % w for w in words))
    g = torch.Generator().manual_seed(52)
    logits = (torch.randn(4, 30, 7, generator=g) * 2).to(U.dev())
    xl = torch.tensor([30, 22, 9, 30])
    dec = CTCDecoder(beam_width=8, labels=labels, lexicon=str(p), wip=0.5, keep_on_device=keep)
    one = dec.decode(logits, xl)
    res = dec.decode_nbest(logits, xl, nbest=5, timesteps=True)
    assert one.decoded_targets.is_cuda == keep and res.decoded_targets.is_cuda == keep
    assert [row[0] for row in res.decoded_sentences] == one.decoded_sentences
    assert res.decoded_targets_lengths[:, 0].tolist() == one.decoded_targets_lengths.tolist()
    n = one.decoded_targets.shape[1]
    assert torch.equal(res.decoded_targets[:, 0, :n].cpu(), one.decoded_targets.cpu())
    assert all(in_lexicon(s, lx) for row in res.decoded_sentences for s in row)
    free = CTCDecoder(beam_width=8, labels=labels, wip=0.5).decode(logits, xl)
    assert any(not in_lexicon(s, lx) for s in free.decoded_sentences)                 # the restriction did something
    listed = CTCDecoder(beam_width=8, labels=labels, lexicon=words, wip=0.5).decode(logits, xl)
    assert listed.decoded_sentences == one.decoded_sentences
    if keep:
        return
    # one model, loaded once, serves a restricted and an unrestricted decoder side by side
    labels4 = LABELS4
    shared = LanguageModel(ARPA, labels4, True)
    lp = rand_lp(53, 3, 25, 4).float().to(U.dev())
    kw = dict(lmwt_=0.7, wip_=0.5, oov_penalty_=0.0, case_sensitive=True)
    before = CTCDecoderEngine(0, 8, labels4, **kw).configure(lm=shared).decode(lp, torch.tensor(XLEN3))
    r_eng = CTCDecoderEngine(0, 8, labels4, **kw).configure(restrict_to_vocabulary=True, lm=shared)
    u_eng = CTCDecoderEngine(0, 8, labels4, **kw).configure(lm=shared)
    assert shared.has_lexicon()
    restricted, after = r_eng.decode(lp, torch.tensor(XLEN3)), u_eng.decode(lp, torch.tensor(XLEN3))
    own = CTCDecoderEngine(0, 8, labels4, lm_path=ARPA, **kw).decode(lp, torch.tensor(XLEN3))
    assert before[2] == after[2] == own[2] and torch.equal(before[0], after[0])
    tiny = LR.Lexicon(TINY)
    assert all(in_lexicon(s, tiny) for s in restricted[2]) and restricted[2] != after[2]
    via_path = CTCDecoder(beam_width=8, labels=labels4, lm_path=ARPA, restrict_to_vocabulary=True, after_logsoftmax=True,
                          lmwt=0.7, wip=0.5, oov_penalty=0.0).decode(lp, torch.tensor(XLEN3))
    assert via_path.decoded_sentences == restricted[2]


# ---- 5. argument errors ----
def test_restriction_without_a_lexicon_launches_nothing():
    lp = rand_lp(5400, 2, 10, 4)
    for lm in (None, LanguageModel(ARPA, LABELS4, True)):
        r = nbest_opt(lp, None, 0, 5, LABELS4, lm, True, timesteps=True, expect_rc=-1)
        assert (r["ids"] == -7).all() and (r["lens"] == -7).all() and (r["n_hyp"] == -7).all()
        assert (r["scores"] == 7.0).all() and (r["counts"] == -7).all() and (r["ts"] == -7).all()
