"""ctypes view of libe2e_ctc.so: the raw C ABI of include/e2e_ctc.h, symbol by symbol.

This is what the parity tests (tests/gpu_util.py), bench.py's C-ABI leg and tools/diag call, so that what they
exercise is the boundary itself -- plain pointers and sizes, return codes, e2e_last_error().  The product's engines
(end2end_amd/engines.py) reach the same entry points through the pybind11 layer end2end_amd._C instead.
There is no CPU fallback.  Nothing here touches oracle/.
"""
import ctypes as C
import os
import threading

import torch

from ._runtime import _C, ABI_VERSION, dtype_code, require_gpu       # noqa: F401  (public names of this module too)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("E2E_CTC_LIB") or os.path.join(_HERE, "csrc", "libe2e_ctc.so")      # (E2E_CTC_LIB: tools/diag A/B builds)

# (the codes are include/e2e_ctc.h's: the pybind layer, which is compiled against the header, carries them)
F32, F64, F16, BF16 = _C.F32, _C.F64, _C.F16, _C.BF16
ALGO_AUTO, ALGO_EXACT, ALGO_FAST = _C.ALGO_AUTO, _C.ALGO_EXACT, _C.ALGO_FAST
REDUCE_NONE, REDUCE_SUM, REDUCE_MEAN = _C.REDUCE_NONE, _C.REDUCE_SUM, _C.REDUCE_MEAN
CHAINS_F64, CHAINS_F32 = _C.CHAINS_F64, _C.CHAINS_F32

_lib = None
_lock = threading.Lock()


class LossOpts(C.Structure):
    """e2e_ctc_loss_opts (include/e2e_ctc.h)."""
    _fields_ = [("grad_scale", C.c_double), ("reduced", C.c_void_p), ("reduction", C.c_int), ("chains", C.c_int)]


class BeamOpts(C.Structure):
    """e2e_ctc_beam_opts (include/e2e_ctc.h)."""
    _fields_ = [("restrict_to_lexicon", C.c_int)]


class AsgBeamOpts(C.Structure):
    """e2e_asg_beam_opts (include/e2e_ctc.h)."""
    _fields_ = [("restrict_to_lexicon", C.c_int), ("timesteps", C.c_void_p)]


class GramBeamOpts(C.Structure):
    """e2e_gram_beam_opts (include/e2e_ctc.h)."""
    _fields_ = [("restrict_to_lexicon", C.c_int), ("timesteps", C.c_void_p)]


class E2EError(RuntimeError):
    """An error reported by the native library (message from e2e_last_error())."""


# One character per type, as end2end_amd._C.SIGNATURES spells the parameters of include/e2e_ctc.h and e2e_ctc_debug.h
# (type_code in csrc/pybind/e2e_C.cpp).  Lower case: values.  Upper case: pointers.
_VALUES = {"v": None, "i": C.c_int, "q": C.c_int64, "z": C.c_size_t, "d": C.c_double, "u": C.c_uint32, "l": C.c_longlong,
           "s": C.c_char_p}
_POINTERS = {"S": C.POINTER(C.c_char_p), "M": C.POINTER(C.c_void_p), "O": C.POINTER(LossOpts), "C": C.POINTER(BeamOpts),
             "A": C.POINTER(AsgBeamOpts), "G": C.POINTER(GramBeamOpts)}


def _ctype(code, host):
    """The ctypes type of one code.  A data pointer (void*, an e2e_lm handle, int64_t* ...) is c_void_p: callers pass
    data_ptr() integers, arrays and byref().  `host`: the typed pointers of the e2e_lm_* calls, which point to host
    arrays, keep their element type (I, Q, U, D: POINTER of i, q, u, d).  A struct of options is POINTER(its Structure),
    so that an instance is passed by reference."""
    if code in _VALUES:
        return _VALUES[code]
    if code in _POINTERS:
        return _POINTERS[code]
    if host and code in "IQUD":
        return C.POINTER(_VALUES[code.lower()])
    assert code in "pmIQUD", "end2end_amd._C.SIGNATURES has a type code that _lib.py does not know: %r" % code
    return C.c_void_p


def load():
    """Load libe2e_ctc.so once; raise loudly if it is absent or has the wrong ABI."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "end2end_amd: native library %s is missing -- run `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C end2end_amd/csrc` (hipcc --offload-arch=gfx950). There is no CPU fallback." % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        # (first of all: a library of another ABI may lack symbols bound below, and would fail with an AttributeError instead)
        if L.e2e_ctc_abi_version() != ABI_VERSION:
            raise ImportError("end2end_amd: %s has ABI %d, expected %d" % (LIB_PATH, L.e2e_ctc_abi_version(), ABI_VERSION))
        for name, sig in _C.SIGNATURES.items():
            fn, (ret, _, params) = getattr(L, name), sig.partition(":")
            fn.restype = _ctype(ret, False)
            fn.argtypes = [_ctype(c, name.startswith("e2e_lm_")) for c in params]
        _lib = L
    return _lib


def check(rc):
    if rc != 0:
        raise E2EError("libe2e_ctc: %s (code %d)" % (load().e2e_last_error().decode(errors="replace"), rc))


def stream_ptr(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
