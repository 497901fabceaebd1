"""Static instruction counts of the lean halo chain kernel's loops, from its gfx950 assembly:
    hipcc <the Makefile's flags for ctc_loss_fast_h1.hip> --cuda-device-only -S ctc_loss_fast_h1.hip -o h1.s
    python tools/diag/chain_loop_counts.py h1.s
A loop is a label and the last backward branch to it.  The chain waves' eight-block loops are the outermost loops with 32
v_ldexp_f64 (8 blocks x 2 pairs x 2 cells), one per direction; the producers' three-block loops the outermost ones with
v_exp_f32 and no f64 multiply-add.  Counts are of the text -- spin paths that are never taken included --, per kernel instance.
"fast path" walks a chain loop once the way a wave does that never has to wait: a forward conditional branch is taken if
what it skips holds an s_sleep (a spin), forward unconditional branches are taken, everything else falls through.

    python tools/diag/chain_loop_counts.py --producers h1.s
counts the producers' EXECUTED path instead (hx_prep_wave): from every loop head whose round trip fills probability blocks, the
instructions a wave issues from one pass over the head to the next when it never waits and the logits are fused -- at a
conditional branch the walk avoids the side from which every way on runs, within three branches, into a spin (s_sleep, the
readers' progress words read 16 bytes at a time) or the log-probability form's exponential (v_rndne_f32), never takes s_cbranch_execz, always takes
s_cbranch_execnz, and otherwise falls through.  A block ends with the store of the producer's progress word (ds_write_b32);
the count is per block, split by what the instructions are for, the split being by opcode and by where in the block an
instruction stands (see CATEGORIES): approximate at the seams -- the scheduler moves a neighbour's instruction across one
now and then --, exact in the total.  Loops are told apart by the number of column groups (global loads per block), by whether
they store to ytab (the alpha side) and by the input's width; the headline's are NV = 4, 32-bit loads."""
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


CATEGORIES = ("global loads and their address arithmetic", "live and row selects", "the ring-space look", "max, sum and their DPP",
              "exponentials and normalisation", "lpmin", "f64 conversion and LDS stores", "the blank pair", "ytab address and stores",
              "progress words", "loop and register rotation")
AVOID = re.compile(r"\t(s_sleep|v_rndne_f32|ds_read_b128)")
FLOAT_OP = re.compile(r"v_(max|max3|exp|fma|fmac|fmamk|mul|add|sub|min|min3|rcp|cmp_\w+)_f32")


def is_ins(ln):
    return ln.startswith("\t") and not ln.startswith("\t.") and not ln.startswith("\t;")


def stretch(body, i):
    """the instructions from line i up to and including the next branch, and the line after it"""
    out = []
    while i < len(body):
        if is_ins(body[i]):
            out.append(body[i])
            if re.match(r"\ts_c?branch", body[i]):
                break
        i += 1
    return out, i + 1


def avoided(body, label, i, depth=3):
    """whether every way on from line i runs into a spin or the log-probability form within `depth` branches"""
    st, nxt = stretch(body, i)
    if any(AVOID.match(x) for x in st):
        return True
    m = re.match(r"\ts_(c?)branch\w*\s+(\.LBB\d+_\d+)", st[-1]) if st else None
    if depth == 0 or not m or m.group(2) not in label:
        return False
    there = avoided(body, label, label[m.group(2)], depth - 1)
    return there if not m.group(1) else there and avoided(body, label, nxt, depth - 1)


def walk(body, label, head):
    """the executed path from the loop head back to it (None if the walk does not come back within 4000 instructions)"""
    path, i = [], head + 1
    while len(path) < 4000:
        if i >= len(body):
            return None
        ln = body[i]
        if i == head:
            return path
        if not is_ins(ln):
            i += 1
            continue
        path.append(ln)
        m = re.match(r"\ts_(c?)branch(_\w+)?\s+(\.LBB\d+_\d+)", ln)
        if m and m.group(3) in label:
            j = label[m.group(3)]
            if not m.group(1):
                take = True
            elif m.group(2) in ("_execz", "_execnz"):
                take = m.group(2) == "_execnz"
            else:
                take = avoided(body, label, i + 1) and not avoided(body, label, j)
            if take:
                if j == head:
                    return path
                i = j
                continue
        i += 1
    return None


def classify(block):
    """block: the instructions of one probability block on the path, the progress word's store last"""
    ops = [ln.split()[0] for ln in block]
    first_float = next((k for k, ln in enumerate(block) if FLOAT_OP.match(ln.split()[0])), len(block))
    last_load = max([k for k in range(first_float) if ops[k].startswith("global_load")], default=-1)
    first_store = next((k for k in range(first_float, len(block)) if ops[k] in ("v_cvt_f64_f32_e32", "s_and_saveexec_b64")), len(block))
    blank = max([k for k, o in enumerate(ops) if o == "ds_write_b128"], default=first_store)
    last_ytab = max([k for k, o in enumerate(ops) if o.startswith("global_store")], default=-1)
    seen_rcp, seen_vector, c = False, False, collections.Counter()
    for k, (o, ln) in enumerate(zip(ops, block)):
        seen_rcp |= o.startswith("v_rcp")
        if k <= last_load:
            cat = 10 if re.match(r"s_(cmp|c?branch|mov)", o) else 0
        elif k < first_float and not seen_vector and not o.startswith(("v_", "ds_", "global_")):
            cat = 2
        elif k < first_store:
            seen_vector = True
            if re.match(r"v_(cmp_\w+_f32|sub_f32|min_f32|min3_f32)", o) or (o.startswith("v_cndmask") and re.search(r"v\d+, 0, v\d+", ln) and not seen_rcp):
                cat = 5
            elif re.match(r"v_(max|max3)_f32|v_mov_b32_dpp|v_add_f32|s_nop", o):
                cat = 3
            elif re.match(r"v_(exp|fma|fmac|fmamk|mul|rcp)_f32", o):
                cat = 4
            elif re.match(r"v_cndmask|v_cmp_\w+_[iu]32|s_and_b64|s_lshl_b32|v_or_b32|v_subrev|v_lshl_or|s_cbranch_vcc", o):
                cat = 1
            elif o == "s_waitcnt":
                cat = 0
            elif re.match(r"s_(and_b32|mul_i32)|v_add_u32", o):
                cat = 6
            else:
                cat = 10
        elif k <= blank:
            if o.startswith("v_cndmask") and re.search(r"v\d+, 0, v\d+", ln):
                cat = 1
            elif re.match(r"v_cndmask|v_mul_f64|v_lshl_add_u32|ds_write_b128", o) or (o == "v_cvt_f64_f32_e32" and "ds_write_b128" in ops[k + 1:k + 4]):
                cat = 7
            else:
                cat = 6
        elif k <= last_ytab:
            cat = 8
        elif re.match(r"ds_write_b32|v_mov_b32|s_add_i32", o):
            cat = 9
        elif o.startswith("s_or_b64") and last_ytab >= 0:
            cat = 8
        else:
            cat = 10
        c[cat] += 1
    return c


def producers(path):
    text = open(path).read().split("\n")
    starts = [i for i, ln in enumerate(text) if re.match(r"_Z\w*ctc_fast_chain_hx_kernel\w*:", ln)]
    for s in starts:
        e = next(i for i in range(s, len(text)) if text[i].startswith("\t.end_amdhsa_kernel") or text[i].startswith(".Lfunc_end"))
        body = text[s:e]
        print(text[s].rstrip(":").split(";")[0])
        label = {m.group(1): i for i, ln in enumerate(body) for m in [re.match(r"(\.LBB\d+_\d+):", ln)] if m}
        heads = sorted({label[m.group(1)] for j, ln in enumerate(body) for m in [re.match(r"\ts_c?branch\w*\s+(\.LBB\d+_\d+)", ln)]
                        if m and m.group(1) in label and label[m.group(1)] < j})
        seen = set()
        for h in heads:
            p = walk(body, label, h)
            if not p or tuple(sorted(p)) in seen:        # (every label on a cycle is a head of the same cycle)
                continue
            seen.add(tuple(sorted(p)))
            ops = [ln.split()[0] for ln in p]
            nb = sum(o == "ds_write_b32" for o in ops)
            if not nb or not any(o.startswith("v_exp_f32") for o in ops) or any(o.startswith("v_ldexp_f64") for o in ops) or "s_sleep" in ops:
                continue
            blocks, cur = [], []
            for ln in p:
                cur.append(ln)
                if ln.split()[0] == "ds_write_b32":
                    blocks.append(cur)
                    cur = []
            blocks[0] = cur + blocks[0]              # (what follows the last progress word belongs to the next pass's first block)
            loads = sum(o.startswith("global_load") for o in ops)
            c = collections.Counter()
            for b in blocks:
                c += classify(b)
            print("  line %d: %d blocks per pass, %d column groups of %s, %s: %d instructions = %.1f per block" % (
                s + h + 1, nb, loads // nb, "16 bits" if any("ushort" in o for o in ops) else "32 bits",
                "ytab stores (alpha)" if any(o.startswith("global_store") for o in ops) else "no ytab stores (beta)", len(p), len(p) / nb))
            for k, name in enumerate(CATEGORIES):
                print("      %-44s %6.1f" % (name, c[k] / nb))


if __name__ == "__main__":
    if sys.argv[1] == "--producers":
        producers(sys.argv[2])
    else:
        main(sys.argv[1])
