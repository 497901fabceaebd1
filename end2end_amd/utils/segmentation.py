"""Word boundaries of a batch, found on the MI355X: the plan of CTCLossSegmented (e2e_ctc_wordseg_plan; the definition:
include/e2e_ctc.h).

    seg = word_segments(logits, targets, logits_lengths, targets_lengths, space_idx, blank_idx=0, min_word_length=3)

An utterance is force-aligned; a word whose frames the model's arg-max reproduces one for one, between two such spaces,
is well recognised; the utterance is cut at the spaces around those words.  `seg` holds CPU tensors, one entry per
segment, utterance-major and in frame order:

    seg.utterance, seg.start, seg.length   which frames
    seg.kind                               WHOLE (an utterance that was not cut), FRAME (one frame: a boundary space),
                                           CHUNK (the frames between two boundaries)
    seg.targets (N,S), seg.targets_lengths what the segment is trained against
"""
import collections

import numpy as np
import torch

from .. import _runtime as R
from .._runtime import _C
from .alignment import get_alignment_3d

WHOLE, FRAME, CHUNK = _C.WORDSEG_WHOLE, _C.WORDSEG_FRAME, _C.WORDSEG_CHUNK
_HDR = _C.WORDSEG_HEADER

WordSegments = collections.namedtuple("WordSegments", "utterance start length kind targets targets_lengths")


class Plan:
    """What e2e_ctc_wordseg_plan left on the device for one batch, and the tensors it was made from."""
    __slots__ = ("dev", "x", "targets", "xl", "tl", "align", "table", "pool", "ws", "B", "T", "V", "Smax")


def _as_long(t, device):
    return torch.as_tensor(t).to(device=device, dtype=torch.long).contiguous()


def check_indices(space_idx, blank_idx, V):
    """ValueError unless both indices are columns of a V-column alphabet."""
    if not 0 <= int(space_idx) < V:
        raise ValueError("space_idx %d outside the alphabet of %d columns" % (space_idx, V))
    if not 0 <= int(blank_idx) < V:
        raise ValueError("blank_idx %d outside the alphabet of %d columns" % (blank_idx, V))


def check_shapes(logits, targets, logits_lengths, targets_lengths):
    """The argument checks that need no device: ValueError for shapes that do not describe one batch."""
    if logits.dim() != 3:
        raise ValueError("logits must be (batch, time, alphabet)")
    B = logits.shape[0]
    targets = torch.as_tensor(targets)
    if targets.dim() != 2 or targets.shape[0] != B:
        raise ValueError("targets must be (batch, max_target_length)")
    if torch.as_tensor(logits_lengths).numel() != B or torch.as_tensor(targets_lengths).numel() != B:
        raise ValueError("lengths must have one entry per utterance")
    if logits.shape[1] < 1 or logits.shape[2] < 1:
        raise ValueError("logits need at least one frame and one column")


def make_plan(logits, targets, logits_lengths, targets_lengths, space_idx, blank_idx, min_word_length, mark=None):
    """log-softmax (plumbing), e2e_ctc_align, e2e_ctc_wordseg_plan -- everything asynchronous, nothing read back.  `logits`
    is f32 or f64 (others are up-cast to f32), moved to the GPU if it is not there.  `mark`: called with a phase's name
    when the phase has been issued (tools/diag/segmented_time.py records an event there)."""
    check_shapes(logits, targets, logits_lengths, targets_lengths)
    check_indices(space_idx, blank_idx, logits.shape[2])
    p = Plan()
    p.dev = dev = R.compute_device(logits)
    x = logits.detach().to(dev)
    if x.dtype not in (torch.float32, torch.float64):
        x = x.to(torch.float32)
    p.x = x
    p.B, p.T, p.V = B, T, V = x.shape
    tg = _as_long(targets, dev)
    p.Smax = tg.shape[1]
    if p.Smax == 0:
        tg = torch.zeros((B, 1), dtype=torch.long, device=dev)      # (an address to hand over; never read)
    p.targets = tg
    p.xl, p.tl = _as_long(logits_lengths, dev), _as_long(targets_lengths, dev)
    n_table = _C.ctc_wordseg_table_elems(B, T)
    nbytes = _C.ctc_wordseg_workspace_bytes(B, T)
    if not n_table or not nbytes:
        raise ValueError("word segmentation: a batch of %d x %d frames is more than the segment table indexes" % (B, T))
    with torch.cuda.device(dev):
        p.align = get_alignment_3d(torch.log_softmax(x, 2), tg, p.xl, p.tl, is_ctc=True,
                                   blank_idx=int(blank_idx), keep_on_device=True)
        if mark:
            mark("align")
        p.table = torch.empty(n_table, dtype=torch.int32, device=dev)
        p.pool = torch.empty((B, T), dtype=torch.long, device=dev)
        # (its own buffer, not the cached workspace: it carries the plan to the finish, across the loss calls in between)
        p.ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        sB, sT, sV = x.stride()
        _C.ctc_wordseg_plan(x.data_ptr(), R.dtype_code(x.dtype), sB, sT, sV, p.align.data_ptr(), tg.data_ptr(),
                            tg.stride(0), p.xl.data_ptr(), p.tl.data_ptr(), B, T, V, p.Smax, int(blank_idx),
                            int(space_idx), int(min_word_length), p.table.data_ptr(), p.table.numel(),
                            p.pool.data_ptr(), p.ws.data_ptr(), p.ws.numel(), R.stream_handle(dev))
        if mark:
            mark("plan")
    return p


def read_plan(plan, fields=3):
    """ONE device-to-host copy of the table's head: the summary, the utterances' first segments and the first `fields` of
    the per-segment arrays (length, target length, kind, utterance, start) -> (summary dict, first (B+1), arrays (fields, N))."""
    cap = plan.B * plan.T
    head = plan.table[: _HDR + plan.B + 1 + fields * cap].cpu().numpy()
    n = int(head[0])
    summary = dict(segments=n, whole=int(head[1]), frame=int(head[2]), chunk=int(head[3]), max_length=int(head[4]),
                   max_target_length=int(head[5]), utterances_cut=int(head[6]))
    first = head[_HDR: _HDR + plan.B + 1]
    arrays = head[_HDR + plan.B + 1:].reshape(fields, cap)[:, :n]
    return summary, first, arrays


def plan_groups(lengths, budget):
    """The segments to gather, as lists of positions into `lengths`: sorted by length (stable), cut into consecutive groups
    such that no group's padded buffer -- its count times its longest member -- exceeds `budget` frames.  A segment longer
    than the budget is a group of its own."""
    lengths = np.asarray(lengths, dtype=np.int64)
    order = np.argsort(lengths, kind="stable")
    srt = lengths[order]
    groups, lo = [], 0
    while lo < len(order):
        # (ascending: count * longest member grows with every newcomer, so the group's end is a binary search)
        padded = np.arange(1, len(order) - lo + 1, dtype=np.int64) * srt[lo:]
        hi = lo + max(int(np.searchsorted(padded, budget, side="right")), 1)
        groups.append(order[lo:hi])
        lo = hi
    return groups


def word_segments(logits, targets, logits_lengths, targets_lengths, space_idx, blank_idx=0, min_word_length=3):
    """The plan as CPU tensors (see the module's docstring).  Synchronises once."""
    plan = make_plan(logits, targets, logits_lengths, targets_lengths, space_idx, blank_idx, min_word_length)
    _, _, (length, tlen, kind, utt, start) = read_plan(plan, fields=5)
    pool = plan.pool.cpu().numpy()
    tg = plan.targets.cpu().numpy()
    n = len(length)
    out = np.zeros((n, max(int(tlen.max()) if n else 0, 1)), dtype=np.int64)
    for i in range(n):
        row = tg[utt[i]] if kind[i] == WHOLE else pool[utt[i], start[i]:]
        out[i, :tlen[i]] = row[:tlen[i]]
    as_long = lambda a: torch.from_numpy(a.astype(np.int64))
    return WordSegments(as_long(utt), as_long(start), as_long(length), as_long(kind), torch.from_numpy(out), as_long(tlen))
