"""GPU: CTCLossSegmented and word_segments (e2e_ctc_wordseg_plan / _gather / _finish) against upstream's own results
(tests/golden/segmented.npz, made by tests/golden/make_segmented_golden.py) and against the test-side f64 restatement
(tests/segmented_ref.py) at the shapes where these kernels can go wrong.  Tolerances are the project's own for the loss:
rtol 1e-4 plus atol 2e-6 against the f64 checker; segment tables are compared exactly."""
import numpy as np
import pytest
import torch

import golden_util as G
import segmented_ref as SR

pytestmark = pytest.mark.gpu

FIX = G.npz("segmented.npz")
CASES = sorted({k.split("/")[0] for k in FIX.files})
DEV = torch.device("cuda", 0)
RTOL, ATOL = 1e-4, 2e-6


def case(name):
    return {k.split("/", 1)[1]: FIX[k] for k in FIX.files if k.split("/")[0] == name}


def run_module(x, tg, xl, tl, space, blank=0, minw=3, w=None, device=DEV):
    """-> (losses, d (losses * w).sum() / d logits, the module) as CPU tensors in the dtype they came in"""
    from end2end_amd import CTCLossSegmented
    mod = CTCLossSegmented(space_idx=space, blank_idx=blank, min_word_length=minw)
    xd = x.detach().to(device).requires_grad_()
    loss = mod(xd, tg.to(device), xl.to(device), tl.to(device))
    (loss.sum() if w is None else (loss * w.to(loss.device, loss.dtype)).sum()).backward()
    return loss.detach().cpu(), xd.grad.cpu(), mod


def table_of(x, tg, xl, tl, space, blank=0, minw=3):
    from end2end_amd.utils.segmentation import word_segments
    s = word_segments(x.to(DEV), tg, xl, tl, space, blank, minw)
    assert all(not t.is_cuda for t in s)
    return [(int(s.utterance[i]), int(s.start[i]), int(s.length[i]), int(s.kind[i]),
             [int(v) for v in s.targets[i, :int(s.targets_lengths[i])]]) for i in range(len(s.utterance))]


def checker(x, tg, xl, tl, space, blank=0, minw=3, with_losses=True):
    """The restatement on the log-softmax the GPU aligns (computed there, so that the two Viterbi passes see the same
    numbers): (segments, losses f64, gradient f64); an utterance out of range is NaN throughout."""
    xd = x.to(DEV)
    if xd.dtype not in (torch.float32, torch.float64):
        xd = xd.float()
    lp = torch.log_softmax(xd, 2).cpu().double().numpy()
    xn, tgn, xln, tln = xd.cpu().numpy(), tg.numpy().reshape(len(xl), -1), xl.numpy(), tl.numpy()
    good = [SR.utterance_valid(tgn[b], int(xln[b]), int(tln[b]), x.shape[1], x.shape[2], tgn.shape[1]) for b in range(len(xln))]
    a = SR.alignment(lp, np.where(np.array(good)[:, None], tgn, 0) if tgn.size else tgn, np.where(good, xln, 1), np.where(good, tln, 0), blank)
    segs = SR.plan(xn, a, tgn, xln, tln, space, blank, minw)
    if not with_losses:
        return segs, a, SR.argmax_first(xn)
    loss, grad = SR.losses_and_grads(xn, [s for s in segs if good[s[0]]], blank)
    for b, ok in enumerate(good):
        if not ok:
            loss[b], grad[b] = np.nan, np.nan
    return segs, loss, grad


def assert_close(got, want, rtol=RTOL, atol=ATOL, what=""):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what + ": NaN pattern differs"
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok]) - (atol + rtol * np.abs(want[ok]))
    print("%s: largest error %.3e (allowed: %.0e relative + %.0e)" % (what, np.max(np.abs(got[ok] - want[ok]), initial=0.0), rtol, atol))
    assert np.all(err <= 0), (what, float(err.max()))


# ---- upstream's own results ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_golden_cases_through_the_module_and_word_segments(name):
    c = case(name)
    x, tg, xl, tl = (torch.from_numpy(c[k]) for k in ("logits", "targets", "x_len", "t_len"))
    space, minw = int(c["space_idx"]), int(c["min_word_length"])
    got = table_of(x, tg, xl, tl, space, 0, minw)
    want = [(int(c["seg_utt"][i]), int(c["seg_start"][i]), int(c["seg_x_len"][i]),
             [int(v) for v in c["seg_targets"][i, :c["seg_t_len"][i]]]) for i in range(len(c["seg_utt"]))]
    assert [(b, s, n, t) for b, s, n, _, t in got] == want
    loss, grad, mod = run_module(x, tg, xl, tl, space, 0, minw)
    assert mod.last_plan["segments"] == len(want)
    assert_close(loss, c["losses"], what="losses")
    assert_close(grad, c["grad"], what="gradient")


# ---- fuzz against the restatement ----------------------------------------------------------------------------------
FUZZ_T = [1, 2, 63, 64, 65, 257]
FUZZ_V = [2, 3, 65, 130]
N_FUZZ = 60


def spelled(rng, n, letters, space, blank, lead_space, trail_space, space_run, min_letters=1):
    """A target and a frame path of exactly n frames that spells it (blank padded)."""
    target, path = [], []

    def put(c):
        reps = int(rng.integers(1, space_run + 1)) if c == space else int(rng.integers(1, 3))
        need_blank = bool(target) and target[-1] == c
        sep = [blank] if need_blank or (path and rng.random() < 0.3) else []
        if len(path) + len(sep) + reps > n:
            return False
        path.extend(sep + [c] * reps)
        target.append(c)
        return True

    use_space = space != blank
    if use_space and lead_space == 0:
        put(space)
    elif use_space and lead_space == 1 and n >= 2:
        path.append(blank)                      # the space sits on frame 1
        put(space)
    while len(path) < n - (1 if trail_space else 0):
        word = [int(rng.choice(letters)) for _ in range(int(rng.integers(min_letters, 5)))] if letters else []
        if not all(put(c) for c in word) or (use_space and not put(space)) or not (word or use_space):
            break
    if use_space and trail_space:
        while len(path) < n - 1:
            path.append(blank)
        if not target or target[-1] != space or path[-1] == blank:
            put(space)
    path += [blank] * (n - len(path))
    return target, path


def fuzz_case(seed):
    rng = np.random.default_rng(1000 + seed)
    T, V = FUZZ_T[seed % 6], FUZZ_V[(seed // 6) % 4]
    B = int(rng.integers(1, 4))
    blank = 0 if seed % 3 else int(rng.integers(0, V))
    space = blank if seed % 10 == 7 else int(rng.choice([c for c in range(V) if c != blank]))
    minw = 0 if seed % 5 == 0 else int(rng.integers(0, 4))
    letters = [c for c in range(V) if c not in (space, blank)][:6]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, V, generator=g) * 0.7
    rows, xl = [], []
    for b in range(B):
        n = T if b == 0 else (1 if seed % 4 == 1 and b == 1 else int(rng.integers(1, T + 1)))
        tgt, path = ([], [blank] * n) if (seed % 7 == 3 and b == B - 1) else spelled(
            rng, n, letters, space, blank, lead_space=(seed + b) % 4, trail_space=(seed + b) % 3 == 0,
            space_run=3 if minw == 0 else 1)
        for t, c in enumerate(path):
            if rng.random() < 0.93:
                x[b, t, c] += 6.0
        rows.append(tgt)
        xl.append(n)
    S = max(max(len(r) for r in rows), 1)
    tg = torch.zeros((B, S), dtype=torch.long)
    for b, r in enumerate(rows):
        tg[b, :len(r)] = torch.tensor(r, dtype=torch.long)
    tl = torch.tensor([len(r) for r in rows])
    if seed % 8 == 5 and B > 1 and len(rows[1]):
        tg[1, 0] = V + 3                        # an out-of-range label next to good utterances
    return x, tg, torch.tensor(xl), tl, space, blank, minw


@pytest.mark.parametrize("seed", range(N_FUZZ))
def test_fuzz_against_the_restatement(seed):
    x, tg, xl, tl, space, blank, minw = fuzz_case(seed)
    segs, want_l, want_g = checker(x, tg, xl, tl, space, blank, minw)
    assert table_of(x, tg, xl, tl, space, blank, minw) == segs
    w = torch.linspace(0.5, 1.5, len(xl))
    loss, grad, mod = run_module(x, tg, xl, tl, space, blank, minw, w=w)
    assert_close(loss, want_l, what="losses")
    assert_close(grad, want_g * w.numpy()[:, None, None], what="gradient")
    for b in range(len(xl)):
        if not np.isnan(want_l[b]):
            assert torch.count_nonzero(grad[b, int(xl[b]):]) == 0          # padded frames: exactly 0


def test_fuzz_covers_the_cases_it_is_there_for():
    seen = dict.fromkeys(["cut", "t_len0", "x_len1", "x_len_below_T", "bad_label", "space_is_blank", "blank_not_0",
                          "space_on_frame0", "space_on_frame1", "space_on_last_frame", "space_runs"], 0)
    shapes = set()
    for seed in range(N_FUZZ):
        x, tg, xl, tl, space, blank, minw = fuzz_case(seed)
        segs, a, p = checker(x, tg, xl, tl, space, blank, minw, with_losses=False)
        shapes.add((x.shape[1], x.shape[2]))
        cut = {b for b, _, _, k, _ in segs if k != SR.WHOLE}
        sp = lambda b, t: 0 <= t < int(xl[b]) and a[b, t] == space == p[b, t]
        seen["cut"] += bool(cut)
        seen["t_len0"] += bool((tl == 0).any())
        seen["x_len1"] += bool((xl == 1).any())
        seen["x_len_below_T"] += bool((xl < x.shape[1]).any())
        seen["bad_label"] += bool((tg >= x.shape[2]).any()) and len(xl) > 1
        seen["space_is_blank"] += space == blank and bool(cut)
        seen["blank_not_0"] += blank != 0 and bool(cut)
        seen["space_on_frame0"] += any(sp(b, 0) for b in cut)
        seen["space_on_frame1"] += any(sp(b, 1) for b in cut)
        seen["space_on_last_frame"] += any(sp(b, int(xl[b]) - 1) for b in cut)
        seen["space_runs"] += minw == 0 and any(sp(b, t) and sp(b, t + 1) for b in cut for t in range(int(xl[b])))
    print(seen)
    assert shapes == {(T, V) for T in FUZZ_T for V in FUZZ_V}
    assert seen["cut"] >= 30 and all(v > 0 for v in seen.values()), seen


# ---- single properties ---------------------------------------------------------------------------------------------
def peaky(seed, B=3, T=70, V=9, space=1, dtype=torch.float32):
    """A batch whose utterances are cut: words of 3..4 letters, every frame recognised but a few."""
    rng = np.random.default_rng(seed)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, V, generator=g, dtype=torch.float64) * 0.7
    rows, xl = [], []
    for b in range(B):
        n = T if b == 0 else int(rng.integers(T // 2, T + 1))
        tgt, path = spelled(rng, n, list(range(2, V)), space, 0, lead_space=3, trail_space=False, space_run=1, min_letters=3)
        for t, c in enumerate(path):
            if rng.random() < 0.95:
                x[b, t, c] += 7.0
        rows.append(tgt)
        xl.append(n)
    tg = torch.zeros((B, max(len(r) for r in rows)), dtype=torch.long)
    for b, r in enumerate(rows):
        tg[b, :len(r)] = torch.tensor(r, dtype=torch.long)
    return x.to(dtype), tg, torch.tensor(xl), torch.tensor([len(r) for r in rows])


def test_nothing_matches_so_the_result_is_ctc_loss_bit_for_bit():
    from end2end_amd import CTCLoss
    g = torch.Generator().manual_seed(3)
    B, T, V = 4, 50, 12
    x = torch.randn(B, T, V, generator=g)
    x[:, :, V - 1] += 30.0                                  # the arg-max is a column no target holds
    tg = torch.randint(1, V - 1, (B, 9), generator=g)
    xl, tl = torch.tensor([50, 41, 50, 33]), torch.tensor([9, 4, 0, 7])
    loss, grad, mod = run_module(x, tg, xl, tl, space=1, minw=0)
    assert mod.last_plan["utterances_cut"] == 0 and mod.last_plan["groups"] == [] and mod.last_plan["whole"] == B
    xd = x.to(DEV).requires_grad_()
    ref = CTCLoss()(xd, tg.to(DEV), xl.to(DEV), tl.to(DEV))
    ref.sum().backward()
    assert torch.equal(loss, ref.detach().cpu()) and torch.equal(grad, xd.grad.cpu())


def test_a_batch_that_needs_three_loss_groups_stays_within_the_input_size():
    # B=2, T=300: about 40 recognised short words, two unrecognised words and an unrecognised tail beside one utterance
    # that is not cut -- upstream would allocate segments * T * V
    B, T, V, space = 2, 300, 12, 1
    rng = np.random.default_rng(5)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, T, V, generator=g) * 0.7
    target, path, wrong = [], [], []
    for w in range(40):
        word = [int(c) for c in rng.choice(np.arange(2, V - 1), size=3, replace=False)]
        target += word + [space]
        path += word + [space]
        wrong += [False] * 4
        if w in (12, 27):                                   # a word the model gets wrong, 25 frames long
            target += [2, 3, 4, 5, space]
            path += [2] * 6 + [3] * 6 + [4] * 6 + [5] * 6 + [space]
            wrong += [True] * 24 + [False]
    tail = [6, 7, 8, 9, 10]
    target += tail
    n_tail = 290 - len(path)
    path += [tail[min(i * 5 // n_tail, 4)] for i in range(n_tail)]
    wrong += [True] * n_tail
    for t, (c, bad) in enumerate(zip(path, wrong)):
        x[0, t, 11 if bad else c] += 8.0
    tg = torch.zeros((B, len(target)), dtype=torch.long)
    tg[0] = torch.tensor(target)
    tg[1, :30] = torch.randint(2, V - 1, (30,), generator=g)
    xl, tl = torch.tensor([len(path), 300]), torch.tensor([len(target), 30])
    segs, want_l, want_g = checker(x, tg, xl, tl, space)
    assert sum(1 for b, _, n, k, _ in segs if b == 0 and k == SR.CHUNK and n <= 4) >= 38 and segs[-1][3] == SR.WHOLE
    assert table_of(x, tg, xl, tl, space) == segs
    loss, grad, mod = run_module(x, tg, xl, tl, space)
    print(mod.last_plan)
    assert len(mod.last_plan["groups"]) >= 3
    assert mod.last_plan["max_buffer_elems"] <= B * T * V
    assert all(n * L * V <= B * T * V for n, L, _ in mod.last_plan["groups"])
    assert sum(n for n, _, _ in mod.last_plan["groups"]) == mod.last_plan["whole"] + mod.last_plan["chunk"]
    assert_close(loss, want_l, what="losses")
    assert_close(grad, want_g, what="gradient")


def test_gradient_equals_torch_autograd_in_f64_over_the_same_segments():
    x, tg, xl, tl = peaky(11, dtype=torch.float64)
    segs = table_of(x, tg, xl, tl, 1)
    assert any(k == SR.CHUNK for _, _, _, k, _ in segs) and any(k == SR.FRAME for _, _, _, k, _ in segs)
    x64 = x.clone().requires_grad_()
    total = 0.0
    per_utt = torch.zeros(len(xl), dtype=torch.float64)
    for b, s, n, _, t in segs:
        lp = torch.log_softmax(x64[b, s:s + n], -1).unsqueeze(1)
        l = torch.nn.functional.ctc_loss(lp, torch.tensor([t or [0]]), torch.tensor([n]), torch.tensor([len(t)]), blank=0,
                                         reduction="sum")
        total = total + l
        per_utt[b] += l.detach()
    total.backward()
    loss, grad, _ = run_module(x, tg, xl, tl, 1)
    assert loss.dtype == torch.float64 and grad.dtype == torch.float64
    assert_close(loss, per_utt, rtol=1e-9, atol=1e-11, what="f64 losses")
    assert_close(grad, x64.grad, rtol=0, atol=1e-9, what="f64 gradient")


def test_grad_output_per_utterance_and_backward_twice():
    from end2end_amd import CTCLossSegmented
    x, tg, xl, tl = peaky(12)
    _, want_l, want_g = checker(x, tg, xl, tl, 1)
    w = torch.tensor([2.0, -0.5, 1.0])
    xd = x.to(DEV).requires_grad_()
    loss = CTCLossSegmented(space_idx=1)(xd, tg.to(DEV), xl.to(DEV), tl.to(DEV))
    out = (loss * w.to(DEV)).sum()
    out.backward(retain_graph=True)
    first = xd.grad.clone()
    xd.grad = None
    out.backward()
    assert torch.equal(first, xd.grad)
    assert_close(first.cpu(), want_g * w.numpy()[:, None, None], what="scaled gradient")


def test_strided_logits_and_cpu_tensors():
    x, tg, xl, tl = peaky(13)
    segs, want_l, want_g = checker(x, tg, xl, tl, 1)
    view = x.permute(1, 0, 2).contiguous().to(DEV).permute(1, 0, 2)              # a time-major tensor seen batch-major
    assert not view.is_contiguous()
    assert table_of(view, tg, xl, tl, 1) == segs
    loss, grad, _ = run_module(view, tg, xl, tl, 1)
    assert_close(loss, want_l, what="losses (strided)")
    assert_close(grad, want_g, what="gradient (strided)")
    loss, grad, _ = run_module(x, tg, xl, tl, 1, device=torch.device("cpu"))      # moved to the GPU and back
    assert not loss.is_cuda and not grad.is_cuda
    assert_close(loss, want_l, what="losses (CPU tensors)")
    assert_close(grad, want_g, what="gradient (CPU tensors)")


def test_bf16_input_equals_the_f32_call_on_the_upcast_tensor():
    x, tg, xl, tl = peaky(14)
    xb = x.to(torch.bfloat16)
    loss_b, grad_b, mod = run_module(xb, tg, xl, tl, 1)
    assert mod.last_plan["utterances_cut"] > 0
    loss_f, grad_f, _ = run_module(xb.float(), tg, xl, tl, 1)
    assert loss_b.dtype == torch.bfloat16 and grad_b.dtype == torch.bfloat16
    assert torch.equal(loss_b, loss_f.to(torch.bfloat16)) and torch.equal(grad_b, grad_f.to(torch.bfloat16))


def test_two_identical_calls_agree_bit_for_bit():
    x, tg, xl, tl = peaky(15, B=4, T=129, V=29)
    a = run_module(x, tg, xl, tl, 1)
    b = run_module(x, tg, xl, tl, 1)
    assert a[2].last_plan["utterances_cut"] > 0
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_readme_example():
    from pytorch_end2end.modules.ctc_loss_segmented import CTCLossSegmented
    x, targets, xl, tl = peaky(16)
    sp = 1
    logits = x.to(DEV).requires_grad_()
    loss = CTCLossSegmented(space_idx=sp)(logits, targets, xl, tl); loss.sum().backward()
    assert loss.shape == (3,) and logits.grad.shape == logits.shape and bool(torch.isfinite(loss).all())
