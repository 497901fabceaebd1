"""`cpp_gram_ctc_loss` -- the name under which upstream's GramCTCLoss finds its engine
(`import_module("cpp_gram_ctc_loss").GramCTCLossEngine(blank_idx, num_base_labels, total_labels, label2ids)`,
pytorch_end2end/modules/ctc_loss.py:102-106; the pybind module of src/losses/gram_ctc_loss_py.cpp).  Here the class is
the MI355X engine: same constructor keywords, `compute(logits, targets, logits_lengths, targets_lengths) -> (losses,
grads)`, computed by libe2e_ctc.so through the pybind11 layer end2end_amd._C.
"""
from end2end_amd.engines import GramCTCLossEngine

__all__ = ["GramCTCLossEngine"]
