"""The banded segment kernel's fallback rate on bench.py's batches (MI355X): per regime, the utterances the call flagged with the
banded form and with the four-pair instance (e2e_debug_segment_band), their flag reasons, the segments whose window did not fit
128 pairs (e2e_debug_band_misses), the time of one call either way (HIP events, median of 9 x 10 calls) and the utterances that
only the banded form flags (a window that does not fit sets flag 8 on its utterance: an empty list shows that every such window
lies in an utterance the four-pair form flags as well).
    python3 tools/diag/band_misses.py"""
import ctypes as C, os, statistics, sys
root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, root)
import torch
import bench
from end2end_amd import _lib
L = _lib.load()
dev = torch.device("cuda", 0)
w = bench.WORKLOAD
B, T, V, S = w["B"], w["T"], w["V"], w["S"]

def batches():
    host, _ = bench.make_batch(1000, B, T, V, S, dev)
    yield "headline", host
    gr = torch.Generator().manual_seed(2000)
    yield "ragged_lengths", (host[0], host[1], torch.randint(T // 2, T + 1, (B,), generator=gr), host[3])
    for boost in (6.0, 10.0, 14.0):
        ab = bench.aligned_batch(int(boost), B, T, V, S, boost)
        yield "trained_regime boost %g" % boost, ab
        if boost == 10.0:
            x, tg, xl, tl = ab
            tg2, tl2 = tg.clone(), tl.clone()
            for k in range(8):
                tg2[32 * k], tl2[32 * k] = tg[32 * k + 1], tl[32 * k + 1]
            yield "label_noise", (x, tg2, xl, tl2)
    # a blank that dominates (an untrained model): the regime in which the bound from the group exponents alone is too wide
    for bias, scale, seed in ((2.0, 0.1, 91), (4.0, 0.1, 92), (6.0, 0.1, 93), (6.0, 1.0, 94), (8.0, 1.0, 95)):
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(B, T, V, generator=g) * scale
        x[:, :, 0] += bias
        tg = torch.randint(1, V, (B, S), generator=g)
        tl = torch.randint(S // 2, S + 1, (B,), generator=g)
        yield "blank + %g, randn x %g" % (bias, scale), (x, tg, torch.full((B,), T, dtype=torch.long), tl)
    for name, seed, scale in (("fallback_regime (x3)", 77, 3.0), ("sharp_unrelated (x8)", 78, 8.0)):
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(B, T, V, generator=g) * scale
        tg = torch.randint(1, V, (B, S), generator=g)
        tl = torch.randint(S // 2, S + 1, (B,), generator=g)
        yield name, (x, tg, torch.full((B,), T, dtype=torch.long), tl)

def one(hp):
    for _ in range(3): hp.call(hp.means[0, :1])
    ts = []
    for _ in range(9):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10): hp.call(hp.means[0, :1])
        e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / 10 * 1e3)
    fl = (C.c_int * B)(); lz = (C.c_double * (2 * B))(); n = C.c_int(-1)
    L.e2e_debug_fast_state(hp.ws.data_ptr(), B, T, V, S, fl, lz)
    L.e2e_debug_band_misses(hp.ws.data_ptr(), B, T, V, S, C.byref(n))
    reasons = {}
    for v in fl:
        for bit in (1, 2, 4, 8, 16, 32, 64):
            if v & bit: reasons[bit] = reasons.get(bit, 0) + 1
    return statistics.median(ts), sum(1 for v in fl if v), reasons, n.value, {i for i, v in enumerate(fl) if v}

print("%-26s %28s | %s | %s" % ("batch (B=256 T=1000 V=29)", "banded: us flagged reasons misses", "four-pair: us flagged reasons",
                               "utterances flagged by the banded form only"))
for name, host in batches():
    hp = bench.HotPath(tuple(t.to(dev) for t in host))
    L.e2e_debug_segment_band(1); a = one(hp)
    L.e2e_debug_segment_band(0); b = one(hp)
    L.e2e_debug_segment_band(1)
    print("%-26s %8.1f %4d %-16s %5d | %8.1f %4d %s | %s" % (name, a[0], a[1], a[2], a[3], b[0], b[1], b[2], sorted(a[4] - b[4])))
    del hp
