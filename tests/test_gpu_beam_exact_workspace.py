"""-m gpu: a workspace of exactly the queried size is enough.  Every form of the CTC beam search, through the C ABI (_lib), in a
buffer of exactly what its workspace query says, with 4 KB of 0xA5 on either side: the call succeeds, both guards still hold
0xA5 after it, and every output is, bit for bit, that of the same call in a workspace 1 MB larger.  The pointer is handed over
once 256-aligned and once moved up by 8 bytes -- the 256 bytes of slack in every query are for exactly that.  A guard that
changes is a failing assertion inside one allocation, not a fault.

Each form runs without a model and with the word-list model (e2e_lm_load_words: no file) restricted to its words, which makes
the model's parts of the layout appear.  e2e_ctc_beam has no options, so there the model is not restricted; the n-best form
with the model is e2e_ctc_beam_nbest_opt, the same call with the option."""
import ctypes as C
import os

import pytest
import torch

import gpu_util as U
from end2end_amd.engines import LanguageModel

pytestmark = pytest.mark.gpu

GUARD, FILL = 4096, 0xA5
WORDS = ["a", "ab", "b", "ba"]
SMALL = dict(B=2, T=6, V=5, W=4)                 # the smallest shape that has a beam to cut: the one-workgroup kernel
WIDE = dict(B=2, T=6, V=300, W=256)              # the smallest (V, W) the CPU tests use for the unpruned general kernel
# form: (entry, shape, timesteps, cutoff_top_n or None, the kernel it takes)
FORMS = {
    "beam": ("beam", SMALL, False, None, "lds"),
    "nbest": ("nbest", SMALL, False, None, "lds"),
    "nbest_timesteps": ("nbest", SMALL, True, None, "lds"),
    "nbest_cut": ("nbest", SMALL, False, 2, "general"),
    "nbest_cut_timesteps": ("nbest", SMALL, True, 2, "general"),
    "stream": ("stream", SMALL, True, None, "lds"),
    "stream_cut": ("stream", SMALL, True, 2, "general"),
    "nbest_general": ("nbest", WIDE, False, None, "general"),
    "stream_general": ("stream", WIDE, True, None, "general"),
}


def labels_of(V):
    return ["_", "a", "b", " "] + ["%s%d" % (chr(99 + i % 24), i // 24) for i in range(V - 4)]


def query(L, entry, B, T, V, W, lm, ts, top_n):
    if entry == "beam":
        return L.e2e_ctc_beam_workspace_bytes_lm(B, T, V, W, lm)
    if entry == "nbest":
        return (L.e2e_ctc_beam_cut_workspace_bytes(B, T, V, W, lm, ts, top_n) if top_n
                else L.e2e_ctc_beam_nbest_workspace_bytes(B, T, V, W, lm, ts))
    return (L.e2e_ctc_beam_cut_stream_workspace_bytes(B, T // 2, V, W, lm, top_n) if top_n
            else L.e2e_ctc_beam_stream_workspace_bytes(B, V, W, lm))


def run(L, _lib, form, lp, model, ws_ptr, ws_bytes):
    """The form's call (a stream: its two chunks, a read-out after each) with this workspace -> {name: CPU tensor} of all it wrote."""
    entry, shape, ts, top_n, _ = FORMS[form]
    B, T, V, W = (shape[k] for k in "BTVW")
    d = lp.device
    N, mo = min(W, 3), T + 1
    lm = model.on(d).handle if model is not None else None
    opts = C.byref(_lib.BeamOpts(1)) if model is not None else None
    o = dict(out=torch.full((B, N, mo), -7, dtype=torch.long, device=d), out_len=torch.full((B, N), -7, dtype=torch.long, device=d),
             n_hyp=torch.full((B,), -7, dtype=torch.long, device=d), scores=torch.full((B, N, 3), 7.0, dtype=torch.float64, device=d),
             counts=torch.full((B, N, 2), -7, dtype=torch.int32, device=d), ts=torch.full((B, N, mo), -7, dtype=torch.long, device=d))
    knobs = (0, W, 3, lm, 1.0, 0.5, 0.0)                                  # blank, width, space, model, lmwt, wip, oov_penalty
    nb = (N, o["out"].data_ptr(), mo, o["out_len"].data_ptr(), o["n_hyp"].data_ptr(), o["scores"].data_ptr(), o["counts"].data_ptr(),
          o["ts"].data_ptr() if ts else None)
    tail = (ws_ptr, ws_bytes, _lib.stream_ptr(d))
    cut = (top_n, 1.0)

    def head(x, xl):
        return (x.data_ptr(), _lib.dtype_code(x.dtype), *x.stride(), xl.data_ptr(), x.shape[0], x.shape[1], V)
    x_len = torch.tensor([T, T - 1], device=d)
    if entry == "beam":
        rc = L.e2e_ctc_beam(*head(lp, x_len), *knobs, o["out"].data_ptr(), N * mo, o["out_len"].data_ptr(), *tail)
    elif entry == "nbest":
        if top_n:
            rc = L.e2e_ctc_beam_nbest_cut(*head(lp, x_len), *knobs, *nb, *tail, opts, *cut)
        elif model is not None:
            rc = L.e2e_ctc_beam_nbest_opt(*head(lp, x_len), *knobs, *nb, *tail, opts)
        else:
            rc = L.e2e_ctc_beam_nbest(*head(lp, x_len), *knobs, *nb, *tail)
    else:
        row_bytes = L.e2e_ctc_beam_stream_row_bytes(T, V, W, lm is not None, 1)
        state = torch.zeros((B, row_bytes), dtype=torch.uint8, device=d)
        o["frames_done"] = torch.full((2, B), -77, dtype=torch.long, device=d)
        first = {}
        for i, lens in enumerate(([T // 2, T // 2], [T - T // 2, T - T // 2 - 1])):
            chunk, cl = lp[:, i * (T // 2): i * (T // 2) + max(lens)], torch.tensor(lens, device=d)
            st = (state.data_ptr(), row_bytes, T, 1)
            args = (*head(chunk, cl), *knobs, *st, *nb, o["frames_done"][i].data_ptr(), *tail, opts)
            rc = L.e2e_ctc_beam_stream_cut(*args, *cut) if top_n else L.e2e_ctc_beam_stream(*args)
            assert rc == 0, (form, i, rc, L.e2e_last_error())
            torch.cuda.synchronize()
            if i == 0:
                first = {"chunk0_" + k: v.cpu().clone() for k, v in o.items() if k != "frames_done"}
        o.update(first)
    assert rc == 0, (form, rc, L.e2e_last_error())
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in o.items()}


@pytest.mark.parametrize("with_model", [False, True], ids=["no_model", "word_list"])
@pytest.mark.parametrize("form", list(FORMS))
def test_a_workspace_of_exactly_the_queried_size_is_enough(form, with_model):
    from end2end_amd import _lib
    L = _lib.load()
    d = U.dev()
    entry, shape, ts, top_n, kernel = FORMS[form]
    B, T, V, W = (shape[k] for k in "BTVW")
    model = LanguageModel(None, labels_of(V), True, words=WORDS, lexicon=True) if with_model else None
    if not os.environ.get("E2E_BEAM_GENERAL"):                            # the form takes the kernel it is listed for
        assert (top_n is not None or L.e2e_ctc_beam_stream_workspace_bytes(B, V, W, with_model) > 0) == (kernel == "general")
    g = torch.Generator().manual_seed(4100 + len(form) + V)
    lp = torch.log_softmax(torch.randn(B, T, V, generator=g) * 1.5, -1).to(d)
    need = query(L, entry, B, T, V, W, int(with_model), int(ts), top_n)
    assert (need > 0) == (entry != "stream" or kernel == "general") or os.environ.get("E2E_BEAM_GENERAL")
    roomy = torch.empty(need + (1 << 20), dtype=torch.uint8, device=d)
    want = run(L, _lib, form, lp, model, roomy.data_ptr(), roomy.numel())
    assert (want["n_hyp"] >= 1).all() or entry == "beam"                    # (there is something to compare)
    for shift in (0, 8):
        buf = torch.full((GUARD + need + GUARD,), FILL, dtype=torch.uint8, device=d)
        assert buf.data_ptr() % 256 == 0
        got = run(L, _lib, form, lp, model, buf.data_ptr() + GUARD + shift, need)
        assert bool((buf[:GUARD] == FILL).all()), (form, shift, "the guard below the workspace was written")
        assert bool((buf[GUARD + need:] == FILL).all()), (form, shift, "the guard above the workspace was written")
        assert sorted(got) == sorted(want)
        for k in want:
            assert torch.equal(got[k].view(torch.uint8), want[k].view(torch.uint8)), (form, shift, k)
