"""CPU: the test-side restatement of the Gram-CTC beam search with a language model (tests/gram_decode_lm_ref.py) against
enumeration of all paths, the gram walk against the id-by-id rule, and the properties of the fixed-seed cases that the GPU
tests (tests/test_gpu_gram_decode_lm.py) rely on."""
import math
import os
import re

import pytest

import gram_decode_lm_ref as LR
import gram_ref as GR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same_fields(a, b):
    return (a.lm, a.lm_before, a.words, a.oov, a.oov_before, a.word, a.st, a.st_before) == \
           (b.lm, b.lm_before, b.words, b.oov, b.oov_before, b.word, b.st, b.st_before)


@pytest.mark.parametrize("with_lm,case_sensitive", [(True, True), (True, False), (False, True)])
def test_unbounded_restatement_equals_enumeration_on_the_tiny_cases(with_lm, case_sensitive):
    """Ranking identical; total, ac and lm to 1e-12 (both sides are f64 sums of at most 625 products of at most 4 factors)."""
    import torch
    for i in range(len(LR.TINY_GRID)):
        R, V, l2i, x = LR.tiny_case(i)
        lp = torch.log_softmax(torch.from_numpy(x).double(), -1).numpy()
        want = LR.tiny_enumeration(i, with_lm, case_sensitive)
        got, _ = LR.beam_search(lp, GR.grams_of(R, V, l2i), LR.tiny_fields(with_lm, case_sensitive), None)
        assert [r["ids"] for r in got] == [r["ids"] for r in want], i
        for g, w in zip(got, want):
            for k in ("total", "ac", "lm"):
                assert abs(g[k] - w[k]) <= 1e-12 * max(1.0, abs(w[k])), (i, g["ids"], k, g[k], w[k])
            assert (g["words"], g["oov"]) == (w["words"], w["oov"])
        if with_lm:                                               # (the model and the knobs do move the ranking somewhere)
            assert any(r["lm"] != 0.0 for r in want) and all(r["words"] <= len(r["ids"]) for r in want)
    # the tables are the ones the issue names
    tables = [tuple(map(tuple, t)) for t in LR.TINY_TABLES]
    assert all(any(tuple(g) in t for t in tables) for g in (LR.AB, LR.A_SP, LR.SP_B, LR.BA))
    assert max(T for _, T in LR.TINY_GRID) <= 4


@pytest.mark.parametrize("case_sensitive", [True, False])
def test_a_gram_gives_the_same_fields_as_its_ids_one_at_a_time(case_sensitive):
    """Bit for bit, a gram with an inner space included, after every short sequence over the alphabet."""
    import itertools
    F = LR.tiny_fields(True, case_sensitive)
    grams = [LR.AB, LR.A_SP, LR.SP_B, LR.BA, LR.A_SP_B, [3, 3], [1, 2, 1, 3, 2, 2], [3]]
    seqs = [s for n in range(4) for s in itertools.product((1, 2, 3), repeat=n)]
    asked = 0
    for seq in seqs:
        f = F.sequence_fields(seq)
        for g in grams:
            through = F.gram_fields(f, seq[-1] if seq else None, tuple(g))
            assert same_fields(through, F.sequence_fields(seq + tuple(g))), (seq, g)
            asked += 1
    assert asked == 40 * len(grams)
    # ... and without a model the words alone
    N = LR.tiny_fields(False, True)
    assert N.gram_fields(N.root, None, (1, 3, 2)).words == 2 and N.gram_fields(N.root, None, (3, 3)).words == 0
    assert N.total(0.0, N.sequence_fields((1, 3, 2))) == -2 * LR.KNOBS["wip"]


def test_pruned_cases_are_decided_by_more_than_rounding():
    """The smallest gap at any cut and in the final ranking of every fixed-seed pruned case the GPU test runs: >= 1e-6, over
    f64 rounding of sums of a few dozen terms of magnitude <= 1e3 (about 1e-12)."""
    gaps = {}
    for model in LR.PRUNED:
        for W in LR.PRUNED_WIDTHS:
            rows, gaps[(model, W, True)] = LR.pruned_ref(model, W)
            V = LR.pruned_case(model)[1]
            assert [len(r) for r in rows] == [W, W, min(W, V), 1]      # one frame: V sequences; no frame: the empty hypothesis
            assert rows[3][0] == dict(ids=(), total=0.0, ac=0.0, lm=0.0, words=0, oov=0)
        _, gaps[(model, 7, False)] = LR.pruned_ref(model, 7, case_sensitive=False)
    _, gaps[("tiny_3gram.arpa", 7, "no model")] = LR.pruned_ref("tiny_3gram.arpa", 7, with_lm=False)
    assert all(g >= LR.MIN_GAP for g in gaps.values()), gaps
    # a width that one frame cannot fill: fewer candidates than W
    rows, _ = LR.pruned_ref("tiny_3gram.arpa", 32)
    assert len(rows[2]) == 8 < 32
    # the case-insensitive search over upper-case labels finds the same words
    a, b = LR.pruned_ref("lm_order4.arpa", 7)[0], LR.pruned_ref("lm_order4.arpa", 7, case_sensitive=False)[0]
    assert [[r["ids"] for r in u] for u in a] == [[r["ids"] for r in u] for u in b]
    assert any(r["oov"] < len(r["ids"]) and r["lm"] != 0.0 for u in a for r in u)


def test_most_tiny_cases_fit_the_widest_beam():
    """The GPU test runs the unpruned search at width 128 and may skip a case with more labellings than that: at least 4/5
    of the cases fit, the T = 2 cases (V <= 11: at most 121 paths) all among them."""
    fits = []
    for i, (_, T) in enumerate(LR.TINY_GRID):
        n = len(LR.tiny_enumeration(i, True, True))
        fits.append(n <= LR.PATH_CAP)
        if T == 2:
            assert LR.tiny_case(i)[1] <= 11 and n <= LR.PATH_CAP, i
    assert sum(fits) >= 0.8 * len(fits), fits
    assert not all(fits)                                          # (and the skip is exercised)


def test_header_declares_the_lm_entry_points_as_an_additive_part_of_abi_4():
    hdr = open(os.path.join(ROOT, "include", "e2e_ctc.h")).read()
    assert "#define E2E_CTC_ABI_VERSION 4" in hdr
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"size_t\s+e2e_gram_beam_workspace_bytes_lm\s*\(", code)
    assert re.search(r"int\s+e2e_gram_ctc_beam_nbest_lm\s*\(", code)
    # the entry without a model keeps its signature
    assert re.search(r"int\s+e2e_gram_ctc_beam_nbest\s*\([^)]*int beam_width, int nbest,[^)]*double\* scores, void\* workspace", code)


def test_library_exports_and_both_layers_bind_them():
    from end2end_amd import _C, _lib
    L = _lib.load()
    assert hasattr(L, "e2e_gram_ctc_beam_nbest_lm") and hasattr(_C, "gram_ctc_beam_nbest_lm")
    # without a model the workspace is the plain search's; a model adds 16 bytes per (prefix, column) of 2 W prefixes
    for B, T, V, K, W in ((64, 1000, 379, 3, 100), (3, 14, 8, 2, 7)):
        plain = _C.gram_beam_workspace_bytes(B, T, V, K, W)
        assert _C.gram_beam_workspace_bytes_lm(B, T, V, K, W, False) == plain == L.e2e_gram_beam_workspace_bytes_lm(B, T, V, K, W, 0)
        extra = _C.gram_beam_workspace_bytes_lm(B, T, V, K, W, True) - plain
        assert 0 <= extra - B * 2 * W * V * 16 < B * 256
    assert _C.gram_beam_workspace_bytes_lm(1, 10, 379, 3, 129, True) == 0


def test_configure_checks_its_arguments_without_a_gpu(tmp_path):
    from end2end_amd.decoders import GramCTCDecoder
    from end2end_amd.decoders.ctc_decoder import CTCDecoderError
    import pytorch_end2end.decoders as PD
    assert PD.GramCTCDecoder is GramCTCDecoder
    l2i = {4: [1, 2]}
    with pytest.raises(ValueError, match="labels"):
        GramCTCDecoder(0, 4, 5, l2i, beam_width=4).configure(wip=0.4)
    with pytest.raises(ValueError, match="beam_width"):
        GramCTCDecoder(0, 4, 5, l2i, beam_width=1, labels=LR.TINY_LABELS).configure(wip=0.4)
    with pytest.raises(CTCDecoderError, match="Can't find a model"):
        GramCTCDecoder(0, 4, 5, l2i, beam_width=4, labels=LR.TINY_LABELS).configure(lm_path=str(tmp_path / "missing.arpa"))
    d = GramCTCDecoder(0, 4, 5, l2i, beam_width=4, labels=LR.TINY_LABELS)
    assert d._decoder.configured is False
    assert d.configure(wip=0.4) is d and d._decoder.configured and d._decoder.space_id == 3 and d._decoder.lmwt == 0.0
    e = GramCTCDecoder(0, 3, 3, {}, beam_width=4, labels=["_", "a", "b"]).configure()
    assert e._decoder.space_id == -1 and (e._decoder.wip, e._decoder.oov_penalty) == (1.0, -10.0)
    assert math.isfinite(e._decoder.wip)
