"""Kernel durations and the gaps between kernels of the headline step, from a rocprofv3 kernel trace:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- python3 bench.py ...      (or tools/diag/ab_time.py)
    python tools/diag/trace_gaps.py DIR [LABEL]
A step is a launch of the lean halo chain kernel and what follows it up to the next one.  Printed: per position in the step the
kernel, the median and quartiles of its duration, and the median gap between the end of the kernel before it and its start
(for the chain kernel: the end of the step before); and the median period from one chain launch to the next."""
import csv
import glob
import os
import statistics
import sys


def main(d, label):
    path = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))[0]
    rows = [(r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(open(path))]
    rows.sort(key=lambda r: r[1])
    heads = [i for i, r in enumerate(rows) if "ctc_fast_chain_hx_kernel" in r[0]]
    steps = [rows[a:b] for a, b in zip(heads, heads[1:])]
    n = statistics.mode(len(s) for s in steps)
    steps = [(i, s) for i, s in zip(heads, steps) if len(s) == n and i > 0]
    print("# %s: %s, %d steps of %d launches" % (label, os.path.basename(path), len(steps), n))
    q = lambda v: statistics.quantiles(v, n=4)       # noqa: E731
    for k in range(n):
        dur = [(s[k][2] - s[k][1]) / 1e3 for _, s in steps]
        gap = [((s[k][1] - s[k - 1][2]) if k else (s[0][1] - rows[i - 1][2])) / 1e3 for i, s in steps]
        name = steps[0][1][k][0].split("(")[0][-60:]
        print("%-60s duration median %7.1f us (quartiles %.1f .. %.1f)   gap in front median %6.1f us (quartiles %.1f .. %.1f)"
              % (name, statistics.median(dur), q(dur)[0], q(dur)[2], statistics.median(gap), q(gap)[0], q(gap)[2]))
    period = [(b[1][0][1] - a[1][0][1]) / 1e3 for a, b in zip(steps, steps[1:]) if b[0] - a[0] == n]
    print("%-60s median %7.1f us (quartiles %.1f .. %.1f), %d consecutive pairs" % ("chain launch to chain launch", statistics.median(period), q(period)[0], q(period)[2], len(period)))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else sys.argv[1])
