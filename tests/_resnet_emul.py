"""TEST-ONLY CPU provider for the ResNet trunk: everything ``tests/_convnext_emul.py`` emulates (the GEMM and the patch
gather among it) plus the entries of ``csrc/resnet.hip`` restated in plain torch with the same call surface, layouts
and rounding points as ``basd_amd._native``: bf16 operands, fp32 accumulation, one rounding to bf16 at the store.
Never imported by the package."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from tests._convnext_emul import *  # noqa: F401,F403
from tests._convnext_emul import handles  # noqa: F401

STEM_K_PAD = 160


def conv3x3_supported(c, ld_in, ld_out, stride=1):
    return (c % 64 == 0 and 64 <= c <= 512 and stride in (1, 2) and ld_in % 8 == 0 and ld_out % 8 == 0 and c <= ld_in
            and c <= ld_out <= 2 * c)


def conv3x3(x, w9, bias, stride=1, relu_in=False, relu_out=False, ld_out=None):
    b, h, w, ld_in = x.shape
    c = w9.shape[0]
    ld_out = ld_in if ld_out is None else ld_out
    assert x.dtype == w9.dtype == bias.dtype == torch.bfloat16 and w9.shape == (c, 9 * c) and bias.shape == (c,)
    assert conv3x3_supported(c, ld_in, ld_out, stride)
    xin = x[..., :c].float().permute(0, 3, 1, 2)                           # the pad columns are never read
    if relu_in:
        xin = F.relu(xin)
    wt = w9.float().reshape(c, 3, 3, c).permute(0, 3, 1, 2)               # [n, (dy, dx, c)] -> [n, c, dy, dx]
    y = F.conv2d(xin, wt, bias.float(), stride=stride, padding=1)
    if relu_out:
        y = F.relu(y)
    out = torch.zeros(b, y.shape[2], y.shape[3], ld_out, dtype=torch.bfloat16)
    out[..., :c] = y.permute(0, 2, 3, 1).to(torch.bfloat16)
    return out


def conv7x7s2_relu_supported(ld_out):
    return ld_out % 8 == 0 and 64 <= ld_out <= 128


def conv7x7s2_relu(x, w, bias, ld_out=128):
    assert x.dtype == w.dtype == bias.dtype == torch.bfloat16 and x.shape[1] == 3
    assert w.shape[0] == 64 and w.shape[1] >= STEM_K_PAD and w.shape[1] % 8 == 0 and conv7x7s2_relu_supported(ld_out)
    wt = w[:, :147].float().reshape(64, 7, 7, 3).permute(0, 3, 1, 2)      # column (dy 7 + dx) 3 + c
    y = F.relu(F.conv2d(x.float(), wt, bias.float(), stride=2, padding=3))
    out = torch.zeros(x.shape[0], y.shape[2], y.shape[3], ld_out, dtype=torch.bfloat16)
    out[..., :64] = y.permute(0, 2, 3, 1).to(torch.bfloat16)
    return out


def maxpool3x3s2_supported(c, ld_in, ld_out):
    return c % 8 == 0 and c >= 8 and ld_in % 8 == 0 and ld_out % 8 == 0 and c <= ld_in and c <= ld_out


def maxpool3x3s2(x, c, ld_out=None):
    b, h, w, ld_in = x.shape
    ld_out = ld_in if ld_out is None else ld_out
    assert x.dtype == torch.bfloat16 and maxpool3x3s2_supported(c, ld_in, ld_out)
    y = F.max_pool2d(x[..., :c].float().permute(0, 3, 1, 2), 3, stride=2, padding=1)
    out = torch.zeros(b, y.shape[2], y.shape[3], ld_out, dtype=torch.bfloat16)
    out[..., :c] = y.permute(0, 2, 3, 1).to(torch.bfloat16)
    return out


def add_relu_supported(c, ld_y, ld_r):
    return c % 8 == 0 and c >= 8 and ld_y % 8 == 0 and ld_r % 8 == 0 and c <= ld_y and c <= ld_r


def add_relu_(y, r, c=None):
    assert y.dtype == r.dtype == torch.bfloat16 and y.dim() == 2 and r.dim() == 2 and y.shape[0] == r.shape[0]
    c = y.shape[1] if c is None else c
    assert add_relu_supported(c, y.shape[1], r.shape[1])
    y[:, :c] = F.relu(y[:, :c].float() + r[:, :c].float()).to(torch.bfloat16)
    return y
