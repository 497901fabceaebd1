"""Records the binding layer of a build into tests/golden/bindings_parent.json (tests/test_bindings_cpu.py compares):
  C    for every function of end2end_amd._C its pybind11 docstring (names, types, defaults), the names of the other
       attributes, and the docstrings of LanguageModel's members
  lib  for every e2e_* symbol that _lib.load() types, restype and argtypes by name
Run on the commit BEFORE the wrappers and argtypes were derived from the header; needs no GPU."""
import ctypes
import inspect
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "bindings_parent.json")


def type_name(t):
    """c_int, c_void_p, ..., LP_c_char_p, LP_LossOpts, None."""
    return None if t is None else t.__name__


def typed_symbols(L):
    hdr = "".join(open(os.path.join(ROOT, "include", n)).read() for n in ("e2e_ctc.h", "e2e_ctc_debug.h"))
    out = {}
    for name in sorted(set(re.findall(r"\b(e2e_[a-z0-9_]+)\s*\(", hdr))):
        fn = getattr(L, name, None)
        if fn is None or (fn.argtypes is None and fn.restype is ctypes.c_int):        # (an untyped symbol: ctypes' defaults)
            continue
        out[name] = {"restype": type_name(fn.restype),
                     "argtypes": None if fn.argtypes is None else [type_name(t) for t in fn.argtypes]}
    return out


def main():
    from end2end_amd import _C, _lib
    funcs = {n: getattr(_C, n).__doc__ for n in dir(_C) if inspect.isbuiltin(getattr(_C, n))}
    others = sorted(n for n in dir(_C) if not n.startswith("__") and n not in funcs)
    lm = {n: getattr(_C.LanguageModel, n).__doc__ for n in dir(_C.LanguageModel) if not n.startswith("__") or n == "__init__"}
    rec = {"C": {"functions": funcs, "attributes": others, "LanguageModel": lm}, "lib": typed_symbols(_lib.load())}
    with open(OUT, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%s: %d functions, %d attributes, %d typed symbols" % (OUT, len(funcs), len(others), len(rec["lib"])))


if __name__ == "__main__":
    assert ctypes.sizeof(ctypes.c_void_p) == 8
    main()
