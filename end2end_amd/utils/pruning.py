"""Per-frame label pruning, the kernel alone (e2e_ctc_label_cut; the definition: include/e2e_ctc.h).

    ids, counts = label_cut(log_probs, lengths, cutoff_top_n=40, cutoff_prob=0.99)

`log_probs` is (batch, time, alphabet) AFTER log-softmax, any strides, f32 / f64 / f16 / bf16.  `ids` is an int32 tensor
(batch, time, K + 1), K = min(cutoff_top_n, alphabet): the labels a pruned beam search expands in each frame, ascending,
-1 behind them; `counts` (batch, time) int32 says how many, 0 for frames at or past an utterance's length.  The blank is
always among them.  Results are CPU tensors unless `keep_on_device=True`.
"""
import torch

from .. import _runtime as R
from .._runtime import _C


def label_cut(log_probs, lengths=None, cutoff_top_n=None, cutoff_prob=1.0, blank_idx=0, keep_on_device=False):
    if log_probs.dim() != 3:
        raise ValueError("log_probs must be (batch, time, alphabet)")
    dev = R.compute_device(log_probs)
    x = log_probs.detach()
    if x.dtype not in (torch.float32, torch.float64, torch.float16, torch.bfloat16):
        x = x.to(torch.float32)
    x = x.to(dev)
    B, T, V = x.shape
    top_n = V if cutoff_top_n is None else int(cutoff_top_n)
    if lengths is None:
        lengths = torch.full((B,), T, dtype=torch.long)
    xl = torch.as_tensor(lengths).to(device=dev, dtype=torch.long).contiguous()
    if xl.numel() != B:
        raise ValueError("lengths must have one entry per utterance")
    K = max(min(top_n, V), 0)
    ids = torch.full((B, T, K + 1), -1, dtype=torch.int32, device=dev)
    counts = torch.zeros((B, T), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        ws = R.workspace(dev, _C.ctc_label_cut_workspace_bytes(B, max(T, 1), V, max(top_n, 1)))
        sB, sT, sV = x.stride()
        _C.ctc_label_cut(x.data_ptr(), R.dtype_code(x.dtype), sB, sT, sV, xl.data_ptr(), B, T, V, int(blank_idx),
                         top_n, float(cutoff_prob), ids.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel(),
                         R.stream_handle(dev))
    return (ids, counts) if keep_on_device else (ids.cpu(), counts.cpu())
