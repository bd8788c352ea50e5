"""TEST-ONLY CPU provider for the ConvNeXt-V2 trunk: everything ``tests/_emul.py`` emulates plus the entries of
``csrc/convnext.hip`` restated in plain torch (gather, conv2d, layer_norm) with the same call surface, layouts and
rounding points as ``basd_amd._native``.  Never imported by the package."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from tests._emul import *  # noqa: F401,F403
from tests._emul import handles  # noqa: F401


def dwconv7_ln_supported(c, ld_in, ld_out):
    return c % 8 == 0 and 8 <= c <= 2048 and ld_in % 8 == 0 and ld_out % 8 == 0 and c <= ld_in and c <= ld_out <= 2 * c


def dwconv7_ln(x, w49, bias, gamma, beta, eps, ld_out=None):
    b, h, w, ld_in = x.shape
    c = w49.shape[1]
    ld_out = ld_in if ld_out is None else ld_out
    assert x.dtype == torch.bfloat16 and w49.dtype == torch.bfloat16 and w49.shape == (49, c)
    assert dwconv7_ln_supported(c, ld_in, ld_out)
    wt = w49.float().t().reshape(c, 1, 7, 7)                              # tap-major [dy * 7 + dx, c] -> [c, 1, dy, dx]
    y = F.conv2d(x[..., :c].float().permute(0, 3, 1, 2), wt, bias.float(), padding=3, groups=c).permute(0, 2, 3, 1)
    y = F.layer_norm(y, (c,), gamma.float(), beta.float(), eps)
    out = torch.zeros(b, h, w, ld_out, dtype=torch.bfloat16)
    out[..., :c] = y.to(torch.bfloat16)
    return out


def grn_supported(c):
    return c % 8 == 0 and 8 <= c <= 4096


def grn_(x, weight, bias, eps=1e-6):
    assert x.dtype == torch.bfloat16 and x.dim() == 3 and x.is_contiguous()
    xf = x.float()
    g = (xf * xf).sum(dim=1, keepdim=True).sqrt()
    n = g / (g.mean(dim=-1, keepdim=True) + eps)
    x.copy_((xf + (bias.float() + weight.float() * (xf * n))).to(torch.bfloat16))
    return x


def patchify(x, p, k_pad):
    assert x.dtype == torch.bfloat16 and x.dim() == 4
    b, c, h, w = x.shape
    assert h % p == 0 and w % p == 0 and k_pad % 8 == 0 and k_pad >= c * p * p
    g = x.reshape(b, c, h // p, p, w // p, p).permute(0, 2, 4, 3, 5, 1)    # [b, oh, ow, i, j, c]
    out = torch.zeros(b * (h // p) * (w // p), k_pad, dtype=torch.bfloat16)
    out[:, :c * p * p] = g.reshape(-1, p * p * c)
    return out
