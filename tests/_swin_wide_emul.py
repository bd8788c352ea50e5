"""TEST-ONLY CPU provider for the Swin trunk with windows 9 .. 16: everything ``tests/_swin_emul.py`` emulates plus the
wide window attention entry (``csrc/swin_wide.hip``) restated in plain torch on the roll / reshape formulation of
``tests/_swin_ref.py``, with the call surface, layouts and rounding points of ``basd_amd._native``: the bias arrives as
the fp32 table [(2 ws - 1)^2, heads] and is expanded here, per call, by the reference's entry-by-entry index.  Never
imported by the package."""
from __future__ import annotations

import torch

from tests import _swin_ref as R
from tests._swin_emul import *  # noqa: F401,F403
from tests._swin_emul import handles, partial, window_attention_rows, window_supported  # noqa: F401

window_attention_wide_supported = partial(window_supported, 9, 16)


def window_attention_wide(qkv, table, ws, shift, heads, scale, ld_out=None):
    assert table.dtype == torch.float32 and table.is_contiguous() and table.shape == ((2 * ws - 1) ** 2, heads)
    return window_attention_rows(window_attention_wide_supported, qkv, R.expand_bias(table, ws), ws, shift, heads, scale,
                                 ld_out)
