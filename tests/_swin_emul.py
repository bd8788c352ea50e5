"""TEST-ONLY CPU provider for the Swin trunk: everything ``tests/_convnext_emul.py`` emulates (GEMM, LayerNorms, patch
gather, the centre-tap LayerNorm route) plus the two entries of ``csrc/swin.hip`` restated in plain torch -- on the
roll / reshape formulation of ``tests/_swin_ref.py``, not on the index arithmetic of the kernels -- with the same call
surface, layouts and rounding points as ``basd_amd._native``.  Never imported by the package."""
from __future__ import annotations

from functools import partial

import torch
import torch.nn.functional as F

from tests import _swin_ref as R
from tests._convnext_emul import *  # noqa: F401,F403
from tests._convnext_emul import handles  # noqa: F401

WINDOW_SLOTS = 64


def window_supported(lo, hi, h, w, ws, shift, heads, c, ld_qkv, ld_out):
    """the gate of a window attention entry that takes the windows lo .. hi"""
    return (lo <= ws <= hi and 0 <= shift < ws and h >= ws and w >= ws and h % ws == 0 and w % ws == 0 and heads >= 1
            and c == 32 * heads and ld_qkv % 8 == 0 and ld_out % 8 == 0 and ld_qkv >= 3 * c and ld_out >= c)


window_attention_supported = partial(window_supported, 1, 8)


def window_bias_image(bias):
    heads, n, _ = bias.shape
    img = torch.zeros(heads, WINDOW_SLOTS, WINDOW_SLOTS, dtype=torch.float32)
    img[:, :n, :n] = bias.float()
    return img


def window_attention_rows(supported, qkv, bias, ws, shift, heads, scale, ld_out):
    """what either entry returns, from the expanded bias [heads, ws^2, ws^2] and the entry's gate"""
    assert qkv.dtype == torch.bfloat16 and qkv.dim() == 4 and qkv.is_contiguous() and bias.dtype == torch.float32
    b, h, w, ld_qkv = qkv.shape
    c = 32 * heads
    ld_out = c if ld_out is None else ld_out
    assert supported(h, w, ws, shift, heads, c, ld_qkv, ld_out)
    y = R.window_attention(qkv[..., :3 * c].float(), bias, ws, shift, heads, scale, round_p=True)
    out = torch.zeros(b, h, w, ld_out, dtype=torch.bfloat16)
    out[..., :c] = y.to(torch.bfloat16)
    return out


def window_attention(qkv, bias_img, ws, shift, heads, scale, ld_out=None):
    assert bias_img.shape == (heads, WINDOW_SLOTS, WINDOW_SLOTS)
    return window_attention_rows(window_attention_supported, qkv, bias_img[:, :ws * ws, :ws * ws], ws, shift, heads, scale,
                                 ld_out)


def patch_merge_ln_supported(c, ld_in, h=2, w=2):
    return c % 8 == 0 and 8 <= 4 * c <= 4096 and ld_in % 8 == 0 and c <= ld_in and h >= 2 and w >= 2 and h % 2 == 0 and w % 2 == 0


def patch_merge_ln(x, c, gamma, beta, eps):
    assert x.dtype == torch.bfloat16 and x.dim() == 4 and x.is_contiguous()
    assert gamma.dtype == beta.dtype == torch.float32 and gamma.shape == beta.shape == (4 * c,)
    assert patch_merge_ln_supported(c, x.shape[3], x.shape[1], x.shape[2])
    return F.layer_norm(R.patch_merge(x[..., :c].float()), (4 * c,), gamma, beta, eps).to(torch.bfloat16)
