"""CPU: the test-side restatement of Gram-CTC decoding (tests/gram_decode_ref.py) against enumeration of all paths, the
margins of the pruned GPU test's fixed-seed inputs, and the checks GramCTCDecoder makes before any GPU work."""
import math

import pytest

import gram_decode_ref as DR
import gram_ref as GR


def test_unbounded_restatement_equals_enumeration_on_the_tiny_cases():
    cases, want = DR.tiny_cases(), DR.tiny_reference()
    assert len(cases) == 300
    for (R, V, l2i, x), enum in zip(cases, want):
        hyps, gap = DR.beam_search(DR.log_softmax(x), GR.grams_of(R, V, l2i), None)
        got = {seq: math.exp(s) for seq, s in hyps}
        assert gap == math.inf and len(got) == len(hyps)
        assert set(got) == {seq for seq, p in enum.items() if p > 0.0}
        for seq, p in got.items():
            assert abs(p - enum[seq]) <= 1e-12 * enum[seq], (seq, p, enum[seq])
        best = max(enum.values())
        assert enum[hyps[0][0]] == best or abs(enum[hyps[0][0]] - best) <= 1e-12 * best


def test_pruned_inputs_are_decided_by_a_margin_not_by_rounding():
    """What lets the GPU test compare the pruned search's sequences exactly and leave nothing out: at no frame of any
    utterance are the last kept and the first dropped hypothesis closer than 1e-8 relative (another seed otherwise)."""
    ref = DR.pruned_reference()
    gaps = [gap for rows in ref.values() for _, gap in rows]
    assert len(gaps) == 32
    print("smallest gap at the cut: %.3g" % min(gaps))
    assert min(gaps) >= 1e-8, sorted(gaps)[:5]


def test_most_tiny_cases_fit_an_unpruned_beam_of_128():
    sizes = [len(e) for e in DR.tiny_reference()]
    small = sum(1 for n in sizes if n <= 128)
    print("tiny cases with <= 128 labellings: %d of %d, largest %d" % (small, len(sizes), max(sizes)))
    assert small >= 0.85 * len(sizes)


def test_key_is_the_headers():
    assert DR.key_of(()) == 0xcbf29ce484222325
    assert DR.key_of((1,)) == ((0xcbf29ce484222325 ^ 1) * 0x100000001b3) % 2 ** 64
    assert DR.key_of((3, 2)) == ((DR.key_of((3,)) ^ 2) * 0x100000001b3) % 2 ** 64


def test_wrapper_checks_need_no_gpu():
    from end2end_amd import _C
    from end2end_amd.decoders import GramCTCDecoder
    from end2end_amd.engines import gram_table
    import pytorch_end2end.decoders as upstream_name
    assert upstream_name.GramCTCDecoder is GramCTCDecoder
    l2i = {4: [1, 2], 5: [3, 3, 1]}
    GramCTCDecoder(0, 4, 6, l2i, beam_width=16, labels=["_", "a", "b", "c"])
    # a bad table raises what gram_table raises
    for bad in ({4: [1, 2]}, {4: [1, 2], 5: [1, 2]}, {4: [1, 9], 5: [1]}, {4: [], 5: [1, 1]}, {4: [1] * 9, 5: [2, 2]}):
        with pytest.raises(ValueError) as want:
            gram_table(4, 6, bad)
        with pytest.raises(ValueError) as got:
            GramCTCDecoder(0, 4, 6, bad)
        assert str(got.value) == str(want.value)
    with pytest.raises(NotImplementedError):
        GramCTCDecoder(1, 4, 6, l2i)
    # the width limit is the library's, at construction
    assert _C.gram_beam_max_width(379, 3) >= 100 and _C.gram_beam_max_width(8000, 3) >= 16
    for V in (2, 21, 379, 1024, 8000, 131072):
        assert _C.gram_beam_max_width(V, 8) >= min(128, 131072 // V)
    cap = _C.gram_beam_max_width(6, 3)
    GramCTCDecoder(0, 4, 6, l2i, beam_width=cap)
    with pytest.raises(ValueError, match="beam_width"):
        GramCTCDecoder(0, 4, 6, l2i, beam_width=cap + 1)
    with pytest.raises(ValueError, match="beam_width"):
        GramCTCDecoder(0, 4, 6, l2i, beam_width=0)
    assert _C.gram_beam_workspace_bytes(2, 50, 6, 3, cap) > 0 and _C.gram_beam_workspace_bytes(2, 50, 6, 3, cap + 1) == 0
    # nbest must be in [1, beam_width]: refused before the logits are looked at
    dec = GramCTCDecoder(0, 4, 6, l2i, beam_width=8, after_logsoftmax=True)
    import torch
    x = torch.zeros(1, 3, 6)
    for n in (0, 9, -1):
        with pytest.raises(ValueError, match="nbest"):
            dec.decode_nbest(x, nbest=n)
    # labels are the R base-label strings
    with pytest.raises(ValueError, match="labels"):
        GramCTCDecoder(0, 4, 6, l2i, labels=["_", "a", "b", "c", "ab", "cca"])
