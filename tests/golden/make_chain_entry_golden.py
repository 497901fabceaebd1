"""Writes tests/golden/chain_entry_parent.npz, the fixture of tests/test_gpu_chain_entry_exit.py: what the lean halo chain kernel
computes, under ALGO_FAST, for every unflagged case of that test -- losses, log Z of both sides, flag words, a SHA-256 of the
gradient's bytes, and the whole gradient of three cases.  Run once on the GPU against a build of the commit BEFORE a change
to the kernel's entry, producers or exit (the file in the tree is from the commit before the test was added):

    python tests/golden/make_chain_entry_golden.py --lib <libe2e_ctc.so of the parent commit> [--out <file>]

The inputs come from the test module's own case builders (same seeds), so the test rebuilds them exactly.
"""
import argparse
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                       # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))      # the repository


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True)
    ap.add_argument("--out", default=os.path.join(HERE, "chain_entry_parent.npz"))
    a = ap.parse_args()
    from end2end_amd import _lib
    _lib.LIB_PATH = os.path.abspath(a.lib)
    import test_gpu_chain_entry_exit as C
    out = {}
    for name, build in C.UNFLAGGED.items():
        la, ga, flags, logz = C.run(build(), _lib.ALGO_FAST)
        assert flags == [0] * len(la), (name, flags)
        out[name + "/losses"] = la
        out[name + "/logz"] = logz
        out[name + "/flags"] = np.asarray(flags, dtype=np.int32)
        out[name + "/grads_sha256"] = np.array(hashlib.sha256(np.ascontiguousarray(ga).tobytes()).hexdigest())
        if name in C.FULL_GRADS:
            out[name + "/grads"] = ga
        print(name, "losses", la.tolist())
    np.savez_compressed(a.out, **out)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
