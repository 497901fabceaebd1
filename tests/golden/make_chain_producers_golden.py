"""Writes tests/golden/chain_producers_parent.npz, the fixture of tests/test_gpu_chain_producers.py: what the lean halo chain
kernel computes, under ALGO_FAST, for every case of that test -- the flag words of all utterances, and of the utterances whose
word is 0 the losses, a SHA-256 of the gradients' bytes, and the whole gradient of three cases.  Run once on the GPU against a
build of the commit BEFORE a change to the kernel's producers (the file in the tree is from the commit before the test was
added):

    python tests/golden/make_chain_producers_golden.py --lib <libe2e_ctc.so of the parent commit> [--out <file>]

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
    ap.add_argument("--out", default=os.path.join(HERE, "chain_producers_parent.npz"))
    a = ap.parse_args()
    from end2end_amd import _lib
    _lib.LIB_PATH = os.path.abspath(a.lib)
    import test_gpu_chain_producers as C
    out = {}
    for name, build in C.CASES.items():
        flags, la, ga = C.recorded_parts(*C.run(build(), _lib.ALGO_FAST))
        out[name + "/flags"] = flags
        out[name + "/losses"] = la
        out[name + "/grads_sha256"] = np.array(hashlib.sha256(ga.tobytes()).hexdigest())
        if name in C.FULL_GRADS:
            out[name + "/grads"] = ga
        print(name, "flags", flags.tolist(), "losses", la.tolist())
    np.savez_compressed(a.out, **out)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
