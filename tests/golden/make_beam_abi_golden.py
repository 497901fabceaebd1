"""Writes tests/golden/beam_queries_parent.npz and tests/golden/beam_refused_parent.json, the fixtures of
tests/test_beam_abi_cpu.py: what the host side of the three beam searches answers -- every workspace / row / width query over
the grid of tests/beam_abi_cases.py, and the return code and e2e_last_error() text of every call in its list of refused calls.
Needs no GPU.  Run once against a build of the commit BEFORE a change to that host side (the files in the tree are from the
commit before ctc_beam.hip got its one plan and one argument block):

    python tests/golden/make_beam_abi_golden.py --lib <libe2e_ctc.so of the parent commit> [--out-dir <directory>]
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                       # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))      # the repository


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True)
    ap.add_argument("--out-dir", default=HERE)
    a = ap.parse_args()
    from end2end_amd import _lib
    _lib.LIB_PATH = os.path.abspath(a.lib)
    import beam_abi_cases as A
    L = _lib.load()
    grid, values = A.query_grid(), A.run_queries(L)
    out = {}
    for name, rows in grid.items():
        out[name + "/args"] = np.array(rows, dtype=np.int32)
        out[name + "/values"] = np.array(values[name], dtype=np.int64)
        print(name, len(rows), "points,", int(np.count_nonzero(out[name + "/values"])), "non-zero")
    np.savez_compressed(os.path.join(a.out_dir, "beam_queries_parent.npz"), **out)
    refused = A.run_refused(L, _lib)
    with open(os.path.join(a.out_dir, "beam_refused_parent.json"), "w") as f:
        json.dump(refused, f, indent=0, sort_keys=True)
        f.write("\n")
    print(len(refused), "refused calls")


if __name__ == "__main__":
    main()
