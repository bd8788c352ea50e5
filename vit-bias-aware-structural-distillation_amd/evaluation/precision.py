"""fp32 matmul precision of the evaluation forward.  The reference evaluates in fp32 with
``torch.set_float32_matmul_precision("high")`` (src/eval.py:16; set for the whole process in src/train.py); here it is
scoped: under "high" / "medium" the ViT's fp32 no-grad forward runs on the split-bf16 (bf16x3) kernels
(``models/vit.py``, csrc/eval_f32x3.hip), while the training step keeps the precision the caller set."""
from __future__ import annotations

import contextlib

import torch


@contextlib.contextmanager
def matmul_precision(precision: str = "high"):
    """set ``torch.set_float32_matmul_precision(precision)`` for the block, restore the previous value after it"""
    prev = torch.get_float32_matmul_precision()
    torch.set_float32_matmul_precision(precision)
    try:
        yield
    finally:
        torch.set_float32_matmul_precision(prev)
