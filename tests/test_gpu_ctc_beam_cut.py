"""GPU: the pruned beam search (CTCDecoder(cutoff_top_n=, cutoff_prob=): e2e_ctc_beam_nbest_cut / e2e_ctc_beam_stream_cut, the
selection kernel ahead of the general kernel) against the restatement label_cut_ref.CutSearch -- lexicon_ref.Search whose
step loops over the frame's kept labels.

Cases (tests/label_cut_ref.py): alphabets of 6, 29 and 300 labels, widths 2, 8 and 32, the cuts (1, 1.0), (3, 1.0),
(V // 2, 0.9), (40, 0.99), each plain, with tests/golden/tiny_3gram.arpa, restricted to its words, restricted to a word list,
and with a transcription lexicon that has homophones; ragged lengths with 0 and 1.  Compared with the comparison and ATOL of
tests/test_gpu_ctc_beam_fuzz.py: the hypotheses and their order, lengths, num_hypotheses, word and OOV counts and timestamps
exactly, the three scores to ATOL; decode() against hypothesis 0.  An utterance whose search margin is below MIN_GAP or that
has a frame within BOUNDARY of cutoff_prob is not compared (LEFT_OUT_UTTS: none; tests/test_label_cut_cpu.py recomputes it).
Streaming: every case is fed in chunks of 1, 7 and all frames, with a zero-length chunk and a mid-stream reset, and equals
the whole pruned call on the frames so far after every chunk (np.array_equal).  A keep-everything cut is the unpruned decoder."""
import warnings

import numpy as np
import pytest
import torch

import ctc_beam_fuzz_util as F
import label_cut_ref as LC
from test_gpu_ctc_beam_fuzz import DTYPES, check_utterance

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
FIELDS = ("decoded_targets", "decoded_targets_lengths", "scores", "ctc_scores", "lm_scores", "num_words", "num_oov_words",
          "num_hypotheses", "timesteps")

_decoders = {}


def decoder(c, cut=True):
    """The case's decoder, pruned or not, once per process."""
    from end2end_amd import CTCDecoder
    key = (c.family, c.V, c.W, c.seed, cut)
    if key not in _decoders:
        kw = dict(beam_width=c.W, after_logsoftmax=True, blank_idx=c.blank, labels=c.labels, lmwt=c.lmwt, wip=c.wip,
                  oov_penalty=c.oov, case_sensitive=c.case_sensitive)
        kw.update(cut_kw(c.cut if cut is True else cut))
        path = F.model_path(c.model) if c.model else None
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                              # (the dropped transcription)
            if c.entries is not None:
                dec = CTCDecoder(transcriptions=c.entries, lm_path=path, restrict_to_vocabulary=c.restricted, **kw)
            elif c.words is not None:
                dec = CTCDecoder(lexicon=c.words, **kw)
            else:
                dec = CTCDecoder(lm_path=path, restrict_to_vocabulary=c.restricted, **kw)
        _decoders[key] = dec
    return _decoders[key]


def inputs(c):
    x = torch.from_numpy(c.x).to(DTYPES[c.dtype]).to(DEV)
    return x, torch.tensor([F.frames_of(c, b) for b in range(len(c.lens))])


def as_dict(res):
    host = lambda t: t.cpu().numpy()   # noqa: E731
    return dict(ids=host(res.decoded_targets), lens=host(res.decoded_targets_lengths), n_hyp=host(res.num_hypotheses),
                scores=np.stack([host(res.scores), host(res.ctc_scores), host(res.lm_scores)], -1),
                counts=np.stack([host(res.num_words), host(res.num_oov_words)], -1), ts=host(res.timesteps))


def same(a, b, what):
    for f in FIELDS:
        assert np.array_equal(getattr(a, f).cpu().numpy(), getattr(b, f).cpu().numpy()), (what, f)
    assert a.decoded_sentences == b.decoded_sentences, what


CASES = [(v,) + k for v in LC.VARIANTS for k in LC.search_cases(v)]


@pytest.mark.parametrize("variant,V,W,ci", CASES)
def test_pruned_search_equals_the_restatement(variant, V, W, ci):
    c = LC.search_case(variant, V, W, ci)
    ref = LC.search_reference(variant, V, W, ci)
    dec = decoder(c)
    assert dec._decoder._cut(V) is not None
    x, xl = inputs(c)
    res = dec.decode_nbest(x, xl, timesteps=True)
    one = dec.decode(x, xl.to(DEV))
    got = as_dict(res)
    compared = 0
    for b in range(len(c.lens)):
        if (V, W, ci, b) in LC.LEFT_OUT_UTTS[variant]:
            continue
        ranking, gap, boundary = ref[b]
        assert gap >= F.MIN_GAP and boundary >= LC.BOUNDARY
        check_utterance(got, b, ranking[:c.W], (variant, V, W, ci, b))
        n = int(one.decoded_targets_lengths[b])                          # decode(): hypothesis 0
        assert n == len(ranking[0]["ids"]) and tuple(one.decoded_targets[b, :n].tolist()) == ranking[0]["ids"]
        assert one.decoded_sentences[b] == res.decoded_sentences[b][0]
        compared += 1
    assert compared


def rows_chunk(x, pos, width):
    """Frames [pos[b], pos[b] + width) of every row b, zero padded: the rows of a stream need not be at the same frame."""
    out = torch.zeros((x.shape[0], width, x.shape[2]), dtype=x.dtype, device=x.device)
    for b, p0 in enumerate(pos):
        n = max(0, min(width, x.shape[1] - p0))
        out[b, :n] = x[b, p0:p0 + n]
    return out


@pytest.mark.parametrize("variant,V,W,ci", CASES)
def test_pruned_stream_equals_the_whole_pruned_call(variant, V, W, ci):
    c = LC.search_case(variant, V, W, ci)
    dec = decoder(c)
    x, xl = inputs(c)
    B, T = x.shape[0], x.shape[1]
    lens = xl.tolist()
    for chunk in (1, 7, T):
        st = dec.open_stream(B, T, timesteps=True)
        pos, step = [0] * B, 0
        while any(p < n for p, n in zip(pos, lens)):
            cl = [max(0, min(n - p, chunk)) for p, n in zip(pos, lens)]
            r = st.feed_nbest(rows_chunk(x, pos, chunk), torch.tensor(cl))
            pos = [p + n for p, n in zip(pos, cl)]
            assert st.frames == pos
            # after every chunk: the whole pruned call on the frames so far (every row's frames start at frame 0 of x)
            same(r, dec.decode_nbest(x[:, :max(pos)], torch.tensor(pos), timesteps=True), (variant, V, W, ci, chunk, pos))
            step += 1
            if chunk == 7 and step == 1:
                # a chunk of no frames moves nothing; then utterance 0 starts anew in mid-stream while the others go on
                same(st.feed_nbest(rows_chunk(x, pos, 3), torch.zeros(B, dtype=torch.long)), r, (variant, V, W, ci, "empty"))
                st.reset([0])
                pos[0] = 0


def cut_kw(cut):
    return {} if cut is False else dict(cutoff_top_n=cut[0], cutoff_prob=cut[1])


@pytest.mark.parametrize("variant", LC.VARIANTS)
def test_keep_everything_cut_is_the_unpruned_decoder(variant):
    for V, W, ci in ((6, 8, 0), (29, 32, 1), (300, 8, 2)):
        c = LC.search_case(variant, V, W, ci)
        x, xl = inputs(c)
        want = decoder(c, cut=False).decode_nbest(x, xl, timesteps=True)
        for cut in ((V, 1.0), (V + 7, 1.0), (None, 1.0)):
            dec = decoder(c, cut=cut)
            assert dec._decoder._cut(V) is None
            same(dec.decode_nbest(x, xl, timesteps=True), want, (variant, V, cut))
    # ... and a cut that prunes is not ignored
    c = LC.search_case(variant, 29, 32, 0)
    x, xl = inputs(c)
    a, b = decoder(c).decode_nbest(x, xl), decoder(c, cut=False).decode_nbest(x, xl)
    assert not np.array_equal(a.scores.numpy(), b.scores.numpy())


def test_wide_alphabet_with_a_model_needs_a_fraction_of_the_workspace():
    """V = 8000 word pieces, width 100, a word-list model: the pruned call runs in the workspace its query names (no answer rows,
    no W * V keys) and returns hypotheses made of kept labels only."""
    from end2end_amd import CTCDecoder, _C
    V, W, B, T = 8000, 100, 2, 6
    rng = np.random.default_rng(74000)
    labels = ["_"] + [chr(0x4e00 + i) for i in range(V - 2)] + [" "]
    lp = F.GF.log_softmax32(rng.standard_normal((B, T, V)).astype(np.float32) * np.float32(3.0))
    dec = CTCDecoder(beam_width=W, after_logsoftmax=True, labels=labels, lexicon=[labels[5] + labels[9], labels[7]],
                     cutoff_top_n=40, cutoff_prob=0.999)
    res = dec.decode_nbest(torch.from_numpy(lp).to(DEV), timesteps=True)
    assert _C.ctc_beam_cut_workspace_bytes(B, T, V, W, True, True, 40) < _C.ctc_beam_nbest_workspace_bytes(B, T, V, W, True, True) / 10
    ids, _, _ = LC.cut(lp.astype(np.float64), [T] * B, 0, 40, 0.999)
    for b in range(B):
        kept = set(ids[b].ravel().tolist())
        assert int(res.num_hypotheses[b]) >= 1
        for j in range(int(res.num_hypotheses[b])):
            n = int(res.decoded_targets_lengths[b, j])
            assert set(res.decoded_targets[b, j, :n].tolist()) - {-1} <= kept
