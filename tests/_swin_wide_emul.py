"""TEST-ONLY CPU provider for the Swin trunk with windows 9 .. 16: everything ``tests/_swin_emul.py`` emulates plus the
wide window attention entry (``csrc/swin_wide.hip``) restated in plain torch on the roll / reshape formulation of
``tests/_swin_ref.py``, with the call surface, layouts and rounding points of ``basd_amd._native``: the bias arrives as
the fp32 table [(2 ws - 1)^2, heads] and is expanded here, per call, by the reference's entry-by-entry index.  Never
imported by the package."""
from __future__ import annotations

import torch

from tests import _swin_ref as R
from tests._swin_emul import *  # noqa: F401,F403
from tests._swin_emul import handles  # noqa: F401


def window_attention_wide_supported(h, w, ws, shift, heads, c, ld_qkv, ld_out):
    return (9 <= ws <= 16 and 0 <= shift < ws and h >= ws and w >= ws and h % ws == 0 and w % ws == 0 and heads >= 1
            and c == 32 * heads and ld_qkv % 8 == 0 and ld_out % 8 == 0 and ld_qkv >= 3 * c and ld_out >= c)


def window_attention_wide(qkv, table, ws, shift, heads, scale, ld_out=None):
    assert qkv.dtype == torch.bfloat16 and qkv.dim() == 4 and qkv.is_contiguous()
    assert table.dtype == torch.float32 and table.is_contiguous() and table.shape == ((2 * ws - 1) ** 2, heads)
    b, h, w, ld_qkv = qkv.shape
    c = 32 * heads
    ld_out = c if ld_out is None else ld_out
    assert window_attention_wide_supported(h, w, ws, shift, heads, c, ld_qkv, ld_out)
    y = R.window_attention(qkv[..., :3 * c].float(), R.expand_bias(table, ws), ws, shift, heads, scale, round_p=True)
    out = torch.zeros(b, h, w, ld_out, dtype=torch.bfloat16)
    out[..., :c] = y.to(torch.bfloat16)
    return out
