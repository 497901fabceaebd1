"""Host cost of a call through end2end_amd._C, for several builds of the extension side by side.  No GPU is touched: the
three calls are answered by the library on the host --
  ctc_beam_max_width(V, with_lm)            a short query
  ctc_loss_takes_dtype(... 10 arguments)    a longer one
  ctc_beam_stream_cut(... 35 arguments)     B = 0: accepted, and returned from before any launch
usage: binding_call_overhead.py LABEL=DIR [LABEL=DIR ...]     DIR holds a _C*.so and csrc/libe2e_ctc.so beside it
The builds are timed in turn, round after round, in one process; the figure of a build is its best round."""
import glob
import importlib.util
import os
import sys
import timeit

ROUNDS, NUMBER = 25, 20000


def load(label, where):
    path, = glob.glob(os.path.join(where, "_C*.so"))
    spec = importlib.util.spec_from_file_location(label + "._C", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def calls(C):
    stream_cut = (0, C.F32, 0, 0, 1, 0, 0, 16, 29, 0, 8, -1, 0, 0.0, 0.0, 0.0, 0, 8192, 64, False, 1, 0, 17, 0, 0, 0, 0, 0,
                  0, 0, 0, 0, False, 8, 1.0)
    return {"ctc_beam_max_width": lambda f=C.ctc_beam_max_width: f(29, True),
            "ctc_loss_takes_dtype": lambda f=C.ctc_loss_takes_dtype, a=C.F32, b=C.ALGO_AUTO: f(a, b, 1000, 29, 200, 29000, 29, 1, 256, 256),
            "ctc_beam_stream_cut": lambda f=C.ctc_beam_stream_cut: f(*stream_cut)}


def main():
    builds = [a.split("=", 1) for a in sys.argv[1:]]
    mods = {label: calls(load(label, where)) for label, where in builds}
    for fs in mods.values():
        for f in fs.values():
            f()
    best = {(label, name): float("inf") for label in mods for name in mods[label]}
    for _ in range(ROUNDS):
        for label, fs in mods.items():
            for name, f in fs.items():
                best[label, name] = min(best[label, name], timeit.timeit(f, number=NUMBER) / NUMBER)
    names = list(next(iter(mods.values())))
    print("ns per call, best of %d rounds of %d calls, builds interleaved" % (ROUNDS, NUMBER))
    print("%-24s" % "call" + "".join("%12s" % label for label in mods))
    for name in names:
        print("%-24s" % name + "".join("%12.1f" % (best[label, name] * 1e9) for label in mods))


if __name__ == "__main__":
    main()
