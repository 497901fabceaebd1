#!/usr/bin/env python3
"""Are the kernels of two device-assembly dumps the same machine code?

  tools/diag/isa_compare.py A B        A, B: a .s file or a directory of them, from
      hipcc <the Makefile's CXXFLAGS> --cuda-device-only -S source.hip -o source.s

Kernels are matched by demangled name with template arguments, namespaces dropped (a refactor may move a kernel into
another namespace or another source).  Of each kernel two things are compared, line by line:
  * the instruction stream: the function body without comments, with the function's number taken out of its local labels
    (.LBB<function>_<block>: the number is the function's place in its file) and every mangled symbol an instruction names
    replaced by its demangled, namespace-free form;
  * the .amdhsa_* descriptor block (registers, scratch, LDS, next_free_*), as it stands.
  tools/diag/isa_compare.py A B 'REGEX=REPLACEMENT'   the same after renaming on both sides: for a kernel whose name changed
      but whose code should not have (a template argument more, with a default: asg_beam.hip's ST,
      'asg_beam_kernel<(\w+, \w+, \w+), false>\(.*?\)=asg_beam_kernel<\1>(AsgBeamParams)'; ctc_gram_decode.hip's ST, whose
      parameter type is spelled as a nest of conditionals: 'gram_beam_kernel<(\w+, \w+, \w+)(, false)?>\(.*?::type\)=gram_beam_kernel<\1>(P)')
One line per kernel, then the counts; the exit status is 0 only if every kernel is on both sides and identical.
It compares two dumps with each other and nothing more."""
import os
import re
import subprocess
import sys


def dumps(path):
    if os.path.isdir(path):
        return [os.path.join(path, f) for f in sorted(os.listdir(path)) if f.endswith(".s")]
    return [path]


def demangle(symbols):
    symbols = sorted(symbols)
    # (binutils before 2.40 does not read the manglings of _Float16 and __bf16: they go in as two other builtin types, which
    #  shifts no substitution, and come out under their own names)
    known = [s.replace("DF16_", "Dh").replace("DF16b", "Ds") for s in symbols]
    out = subprocess.run(["c++filt"], input="\n".join(known), capture_output=True, text=True, check=True).stdout.split("\n")
    out = [re.sub(r"\bhalf\b", "_Float16", re.sub(r"\bchar16_t\b", "__bf16", d)) for d in out]
    # every qualification goes: `e2e::(anonymous namespace)::f<e2e::T>` -> `f<T>`
    return {s: re.sub(r"(\(anonymous namespace\)|\b[A-Za-z_]\w*)::", "", d) for s, d in zip(symbols, out)}


def kernels(path):
    """{plain name: (instruction lines, descriptor lines)} of every kernel of the dumps under path"""
    raw = {}
    for f in dumps(path):
        lines = open(f).read().split("\n")
        start = {}
        for i, ln in enumerate(lines):
            m = re.match(r"([A-Za-z_$][\w$.]*):", ln)
            if m:
                start[m.group(1)] = i
            m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
            if m:
                sym = m.group(1)
                end = next(j for j in range(i, len(lines)) if lines[j].strip() == ".end_amdhsa_kernel")
                assert sym in start and sym not in raw, "%s: kernel %s has no body before its descriptor, or two" % (f, sym)
                raw[sym] = (lines[start[sym] + 1:i], lines[i + 1:end])
    names = demangle({s for body, _ in raw.values() for ln in body for s in re.findall(r"\b_Z\w+", ln)} | set(raw))
    res = {}
    for sym, (body, desc) in raw.items():
        code = []
        for ln in body:
            ln = ln.split(";")[0].strip()
            if not ln:
                continue
            ln = re.sub(r"\.L(\w*?)\d+_(\d+)", r".L\1_\2", ln)
            code.append(re.sub(r"\b_Z\w+", lambda m: names[m.group(0)], ln))
        assert names[sym] not in res, "two kernels named %s under %s" % (names[sym], path)
        res[names[sym]] = (code, [ln.strip() for ln in desc if ln.strip()])
    return res


def renamed(K, rule):
    """K with the rule REGEX=REPLACEMENT applied to the kernels' names and to the names inside their instructions (the symbols
    of a kernel's LDS variables carry its name)."""
    if not rule:
        return K
    pat, repl = rule.split("=", 1)
    res = {}
    for k, (code, desc) in K.items():
        name = re.sub(pat, repl, k)
        assert name not in res, "the rule names two kernels %s" % name
        res[name] = ([re.sub(pat, repl, ln) for ln in code], desc)
    return res


def main(a, b, rule=None):
    A, B = renamed(kernels(a), rule), renamed(kernels(b), rule)
    same = 0
    for k in sorted(set(A) | set(B)):
        if k not in A or k not in B:
            verdict = "MISSING in %s" % (a if k not in A else b)
        else:
            diff = [what for what, i in (("instructions", 0), ("descriptor", 1)) if A[k][i] != B[k][i]]
            verdict = "DIFFERENT: " + ", ".join(diff) if diff else "identical (%d instruction lines)" % len(A[k][0])
            same += not diff
        print("%-100s %s" % (k, verdict))
    print("%d kernels in %s, %d in %s, %d identical" % (len(A), a, len(B), b, same))
    return 0 if same == len(A) == len(B) else 1


if __name__ == "__main__":
    if len(sys.argv) not in (3, 4):
        sys.exit(__doc__)
    sys.exit(main(*sys.argv[1:]))
