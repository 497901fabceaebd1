"""Static instruction counts of the lean halo chain kernel's loops, from its gfx950 assembly:
    hipcc <the Makefile's flags for ctc_loss_fast_h1.hip> --cuda-device-only -S ctc_loss_fast_h1.hip -o h1.s
    python tools/diag/chain_loop_counts.py h1.s
A loop is a label and the last backward branch to it.  The chain waves' eight-block loops are the outermost loops with 32
v_ldexp_f64 (8 blocks x 2 pairs x 2 cells), one per direction; the producers' three-block loops the outermost ones with
v_exp_f32 and no f64 multiply-add.  Counts are of the text -- spin paths that are never taken included --, per kernel instance.
"fast path" walks a chain loop once the way a wave does that never has to wait: a forward conditional branch is taken if
what it skips holds an s_sleep (a spin), forward unconditional branches are taken, everything else falls through."""
import collections
import re
import sys

CLASSES = (("f64 arithmetic", r"v_(fma|fmac|mul|add)_f64"), ("DPP moves", r"v_mov_b32_dpp"), ("v_ldexp_f64", r"v_ldexp_f64"),
           ("ds_read_b128", r"ds_read_b128"), ("ds_read_b64", r"ds_read_b64"), ("ds_read_b32", r"ds_read_b32"), ("ds_write", r"ds_write"),
           ("s_waitcnt", r"s_waitcnt"), ("plain v_mov_b32", r"v_mov_b32_e32"), ("v_mov_b64", r"v_mov_b64"),
           ("v_readfirstlane", r"v_readfirstlane"), ("scratch", r"scratch_"), ("global / flat", r"(global|flat)_"),
           ("other vector", r"v_"), ("scalar / branch", r"s_"))


def instructions(lines):
    return [ln.split()[0] for ln in lines if ln.startswith("\t") and not ln.startswith("\t.") and not ln.startswith("\t;")]


def loops(body):
    label = {m.group(1): i for i, ln in enumerate(body) for m in [re.match(r"(\.LBB\d+_\d+):", ln)] if m}
    end = {}
    for j, ln in enumerate(body):
        m = re.match(r"\ts_c?branch\w*\s+(\.LBB\d+_\d+)", ln)
        if m and m.group(1) in label and label[m.group(1)] < j:
            end[label[m.group(1)]] = j
    spans = sorted(end.items())
    return [(a, b) for a, b in spans if not any(c < a and b < d for c, d in spans)]      # outermost


def fast_path(lines):
    label = {m.group(1): i for i, ln in enumerate(lines) for m in [re.match(r"(\.LBB\d+_\d+):", ln)] if m}
    i, n = 0, 0
    while i < len(lines):
        ln = lines[i]
        if ln.startswith("\t") and not ln.startswith("\t.") and not ln.startswith("\t;"):
            n += 1
            m = re.match(r"\ts_(c?)branch\w*\s+(\.LBB\d+_\d+)", ln)
            if m and label.get(m.group(2), -1) > i:
                j = label[m.group(2)]
                if not m.group(1) or any("s_sleep" in x for x in lines[i + 1:j]):
                    i = j
                    continue
        i += 1
    return n


def main(path):
    text = open(path).read().split("\n")
    starts = [i for i, ln in enumerate(text) if re.match(r"_Z\w*ctc_fast_chain_hx_kernel\w*:", ln)]
    for s in starts:
        e = next(i for i in range(s, len(text)) if text[i].startswith("\t.end_amdhsa_kernel") or text[i].startswith(".Lfunc_end"))
        body = text[s:e]
        print("%s: %d instructions" % (text[s].rstrip(":"), len(instructions(body))))
        for a, b in loops(body):
            ins = instructions(body[a:b + 1])
            n_ldexp = sum(i == "v_ldexp_f64" for i in ins)
            n_exp = sum(i == "v_exp_f32_e32" or i == "v_exp_f32" for i in ins)
            n_fma64 = sum(i.startswith("v_fma") and "f64" in i for i in ins)
            if n_ldexp == 32:
                what = "chain wave, eight blocks"
            elif n_exp and not n_fma64:
                what = "producer loop (%d v_exp_f32)" % n_exp
            else:
                continue
            c = collections.Counter()
            for i in ins:
                c[next(name for name, pat in CLASSES if re.match(pat, i))] += 1
            print("  lines %d..%d  %s: %d instructions" % (s + a + 1, s + b + 1, what, len(ins))
                  + (", fast path %d = %.1f per step" % (fast_path(body[a:b + 1]), fast_path(body[a:b + 1]) / 64.0) if n_ldexp == 32 else ""))
            print("    " + ", ".join("%s %d" % (name, c[name]) for name, _ in CLASSES if c[name]))


if __name__ == "__main__":
    main(sys.argv[1])
