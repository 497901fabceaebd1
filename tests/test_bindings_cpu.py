"""CPU: the binding layer is derived from the header and binds what it bound when it was written out by hand.

end2end_amd/csrc/pybind/e2e_C.cpp deduces every wrapper and _C.SIGNATURES from the types of the functions in
include/e2e_ctc.h and e2e_ctc_debug.h; end2end_amd/_lib.py types the ctypes view from SIGNATURES.
tests/golden/bindings_parent.json (make_bindings_golden.py) holds what the last hand-written layer bound."""
import ctypes as C
import json
import os
import re

import pytest

from test_host_cpu import _declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "bindings_parent.json")))

# Arguments that are `int` in the header and were `bool` in the hand-written wrapper; they are `int` now (the library reads
# each of them as zero / non-zero, and a Python bool is an int).  function -> positions, or names where it has names.
BOOL_TO_INT = {
    "ctc_loss_fwd_bwd": ["input_is_logprobs"], "ctc_noblank_fwd_bwd": ["input_is_logprobs"], "gram_ctc_fwd_bwd": ["input_is_logprobs"],
    "gram_beam_workspace_bytes_lm": [5], "gram_beam_stream_row_bytes": [4, 5], "gram_beam_stream_workspace_bytes": [4, 5],
    "gram_ctc_beam_stream": ["scored"], "asg_beam_workspace_bytes": [4], "asg_beam_stream_row_bytes": [3],
    "asg_beam_stream_workspace_bytes": [3], "ctc_beam_workspace_bytes_lm": [4], "ctc_beam_max_width": [1],
    "ctc_beam_nbest_workspace_bytes": [4, 5], "ctc_beam_stream_row_bytes": [3, 4], "ctc_beam_stream_workspace_bytes": [3],
    "ctc_beam_stream": ["with_timesteps"], "ctc_beam_cut_max_width": [1], "ctc_beam_cut_workspace_bytes": [4, 5],
    "ctc_beam_cut_stream_workspace_bytes": [4], "ctc_beam_stream_cut": ["with_timesteps"], "ctc_align_workspace_bytes": [4],
    "ctc_align": ["is_ctc"], "ctc_wordseg_finish": ["last"],
}
BOOL_TO_INT_RETURN = ["ctc_loss_takes_dtype"]

# What load() types otherwise than the hand-written statements did: symbol -> (position or "restype", was, is, why).
LIB_CHANGES = {
    "e2e_debug_gram_redo_flags": (5, "LP_c_int", "c_void_p", "widened: a data pointer outside e2e_lm_*, like its eight untyped siblings"),
    "e2e_debug_noblank_redo_flags": (4, "LP_c_int", "c_void_p", "widened: as e2e_debug_gram_redo_flags"),
    "e2e_lm_free": ("restype", "c_int", None, "the function returns void; it had ctypes' default"),
}


def _split(doc):
    """'name(a: T = d, ...) -> R' -> (name, [[arg name, type, default or None], ...], R)"""
    line = doc.strip().split("\n")[0]
    m = re.fullmatch(r"(\w+)\((.*)\) -> (.+)", line)
    args = [list(re.fullmatch(r"(\w+): (.+?)(?: = (.+))?", a).groups()) for a in m.group(2).split(", ") if a]
    return m.group(1), args, m.group(3)


def test_C_has_the_parents_functions_and_attributes():
    import inspect
    from end2end_amd import _C
    funcs = {n for n in dir(_C) if inspect.isbuiltin(getattr(_C, n))}
    assert funcs == set(GOLDEN["C"]["functions"])
    others = sorted(n for n in dir(_C) if not n.startswith("__") and n not in funcs)
    assert others == sorted(GOLDEN["C"]["attributes"] + ["SIGNATURES"])
    lm = {n: getattr(_C.LanguageModel, n).__doc__ for n in dir(_C.LanguageModel) if not n.startswith("__") or n == "__init__"}
    assert lm == GOLDEN["C"]["LanguageModel"]


def test_C_signatures_equal_the_parents_but_for_the_listed_flags():
    from end2end_amd import _C
    assert set(BOOL_TO_INT) | set(BOOL_TO_INT_RETURN) <= set(GOLDEN["C"]["functions"])
    for name, doc in sorted(GOLDEN["C"]["functions"].items()):
        _, was, was_ret = _split(doc)
        int_type = _split(GOLDEN["C"]["functions"]["ctc_greedy"])[1][1][1]           # (how this pybind11 spells `int`)
        for which in BOOL_TO_INT.get(name, []):
            hit = [a for i, a in enumerate(was) if which in (i, a[0])]
            assert len(hit) == 1 and hit[0][1] == "bool", (name, which, "was no bool in the parent: the list is stale")
            hit[0][1] = int_type
        if name in BOOL_TO_INT_RETURN:
            assert was_ret == "bool"
            was_ret = "int"
        assert _split(getattr(_C, name).__doc__) == (name, was, was_ret), name


def test_signatures_cover_exactly_the_declared_symbols():
    from end2end_amd import _C, _lib
    assert set(_C.SIGNATURES) == _declared()
    L = _lib.load()
    for name in sorted(_declared()):
        fn, (ret, _, params) = getattr(L, name), _C.SIGNATURES[name].partition(":")
        assert fn.argtypes is not None and len(fn.argtypes) == len(params), name
    # one of each kind, against the header read by eye
    assert _C.SIGNATURES["e2e_ctc_greedy"] == "i:piqqqQiiiiQQp"
    assert _C.SIGNATURES["e2e_lm_load_transcriptions"] == "i:sSIIiSiiM"
    assert _C.SIGNATURES["e2e_lm_transcribe"] == "i:mQqiUiI"
    assert _C.SIGNATURES["e2e_lm_score"] == "d:mUiu" and _C.SIGNATURES["e2e_lm_word_string"] == "s:mu"
    assert _C.SIGNATURES["e2e_lm_free"] == "v:m" and _C.SIGNATURES["e2e_last_error"] == "s:"
    assert _C.SIGNATURES["e2e_debug_occupy"] == "i:iiilp" and _C.SIGNATURES["e2e_ctc_loss_workspace_bytes"] == "z:iiiiii"
    assert _C.SIGNATURES["e2e_ctc_beam_nbest_cut"][-5:] == "zpCid" and _C.SIGNATURES["e2e_asg_beam_stream"][-2:] == "pA"
    assert _C.SIGNATURES["e2e_gram_ctc_beam_nbest_opt"][-2:] == "pG" and _C.SIGNATURES["e2e_asg_fwd_bwd"][-2:] == "pO"
    typed = {n: (getattr(L, n).restype, getattr(L, n).argtypes) for n in _declared()}
    assert typed["e2e_debug_fast_state"] == (C.c_int, [C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 2)
    assert typed["e2e_debug_occupy"] == (C.c_int, [C.c_int] * 3 + [C.c_longlong, C.c_void_p])
    assert typed["e2e_debug_loss_route"] == (C.c_int, [C.c_int] * 7 + [C.c_int64] * 3 + [C.c_void_p] * 2)
    assert typed["e2e_ctc_abi_version"] == (C.c_int, []) and typed["e2e_last_error"] == (C.c_char_p, [])


def test_lib_types_equal_the_parents_but_for_the_listed_changes():
    from end2end_amd import _lib
    L = _lib.load()
    name_of = lambda t: None if t is None else t.__name__
    assert len([n for n, r in GOLDEN["lib"].items() if r["argtypes"] is not None]) == 76
    seen = set()
    for name, rec in sorted(GOLDEN["lib"].items()):
        fn = getattr(L, name)
        want_ret, want_args = rec["restype"], rec["argtypes"]
        if name in LIB_CHANGES:
            at, was, now, _ = LIB_CHANGES[name]
            if at == "restype":
                assert want_ret == was
                want_ret = now
            else:
                assert want_args[at] == was
                want_args = want_args[:at] + [now] + want_args[at + 1:]
            seen.add(name)
        assert name_of(fn.restype) == want_ret, name
        if want_args is not None:
            assert [name_of(t) for t in fn.argtypes] == want_args, name
    assert seen == set(LIB_CHANGES)
    # the structs of options still go by reference, a handle comes back through byref
    assert L.e2e_ctc_loss_fwd_bwd_opt.argtypes[-1] is C.POINTER(_lib.LossOpts)
    assert list(L.e2e_lm_load_arpa.argtypes) == [C.c_char_p, C.POINTER(C.c_char_p), C.c_int, C.c_int, C.POINTER(C.c_void_p)]


def test_lib_and_runtime_share_their_helpers_and_constants():
    from end2end_amd import _C, _lib, _runtime
    assert _lib.dtype_code is _runtime.dtype_code and _lib.require_gpu is _runtime.require_gpu
    assert (_lib.F32, _lib.F64, _lib.F16, _lib.BF16) == (_C.F32, _C.F64, _C.F16, _C.BF16) == (0, 1, 2, 3)
    assert (_lib.ALGO_AUTO, _lib.ALGO_EXACT, _lib.ALGO_FAST) == (0, 1, 2)
    assert (_lib.REDUCE_NONE, _lib.REDUCE_SUM, _lib.REDUCE_MEAN, _lib.CHAINS_F64, _lib.CHAINS_F32) == (0, 1, 2, 0, 1)
    assert _lib.ABI_VERSION == _C.ABI_VERSION == 4 and os.path.exists(_lib.LIB_PATH)
    for public in ("load", "check", "stream_ptr", "E2EError", "LossOpts", "BeamOpts", "AsgBeamOpts", "GramBeamOpts"):
        assert hasattr(_lib, public)


def test_flags_that_became_int_still_take_bools_and_keywords():
    from end2end_amd import _C
    assert _C.ctc_beam_max_width(29, True) == _C.ctc_beam_max_width(29, 1) > 0
    assert _C.ctc_beam_max_width(29, False) == _C.ctc_beam_max_width(29, 0) > 0
    assert _C.ctc_loss_takes_dtype(_C.F32, _C.ALGO_AUTO, 50, 28, 30, 1400, 28, 1, 0, 0) == 1
    with pytest.raises(ValueError, match="space_idx 7 is neither -1 nor in"):
        _C.ctc_noblank_fwd_bwd(0, _C.F32, False, 1, 1, 1, 0, 0, 0, 0, 1, 1, 4, 0, 7, 0, 0, 0, 0, 0)
    with pytest.raises(ValueError, match="radix 9 is not in"):
        _C.gram_ctc_fwd_bwd(0, _C.F32, False, 1, 1, 1, 0, 0, 0, 0, 1, 1, 4, 0, 0, 0, 0, 9, 1, 0, 0, 0, 0, 0)
    with pytest.raises(ValueError, match="asg_fwd_bwd: dtype must be F32 or F64"):
        _C.asg_fwd_bwd(0, _C.F16, 1, 1, 1, 0, 0, 0, 0, 0, 1, 1, 4, 0, 0, 0, 0, 0, 0, 0)
    with pytest.raises(_C.E2EError):                      # by keyword, the struct's fields spread, refused before any launch
        _C.ctc_beam_nbest(lp=0, dtype=9, sB=1, sT=1, sV=1, x_len=0, B=1, T=1, V=4, blank=0, beam_width=2, space_id=-1, lm=0,
                          lmwt=0.0, wip=0.0, oov_penalty=0.0, nbest=1, out=0, max_out=2, out_len=0, n_hyp=0, scores=0, counts=0,
                          timesteps=0, workspace=0, workspace_bytes=0, stream=0, restrict_to_lexicon=False)
