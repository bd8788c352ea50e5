"""Plain-torch fp64 restatement of the pre-norm ViT training forward (test helper).

Written from the definition of the model, not from ``basd_amd.models``: patch embedding as unfold @ W^T + b, CLS token
and position embedding, LayerNorm (eps 1e-6), packed qkv in (3, heads, head_dim) order, softmax(Q K^T hd^-1/2) V, proj,
exact-erf GELU MLP; every residual branch is multiplied by an explicit per-sample stochastic-depth scale; final norm
and the head on the CLS row.  Parameter names follow the model's ``state_dict`` keys.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F


def leaf_params(state_dict, device="cpu"):
    """fp64 leaf copies (requires_grad) of a state_dict's tensors"""
    return {k: v.detach().to(device=device, dtype=torch.float64).clone().requires_grad_(True)
            for k, v in state_dict.items()}


def _layer_norm(x, weight, bias, eps=1e-6):
    mean = x.mean(dim=-1, keepdim=True)
    var = (x - mean).square().mean(dim=-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * weight + bias


def _gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def vit_forward(params, images, *, heads, scales=None, taps=()):
    """-> (logits [B, classes], {i: output of block i without its CLS row [B, T - 1, D]} for i in ``taps``).

    ``params``: name -> fp64 tensor (``leaf_params``); ``scales``: [2 * depth, B] per-sample multipliers of the two
    residual branches of every block (row 2 i: attention branch of block i, row 2 i + 1: its MLP branch), or None."""
    x = images.to(torch.float64)
    b = x.shape[0]
    w = params["patch_embed.proj.weight"]
    d, p = w.shape[0], w.shape[-1]
    depth = 1 + max(int(k.split(".")[1]) for k in params if k.startswith("blocks."))
    patches = F.unfold(x, kernel_size=p, stride=p).transpose(1, 2)               # [B, N, C p p], (c, kh, kw) order
    h = patches @ w.reshape(d, -1).t() + params["patch_embed.proj.bias"]
    h = torch.cat([params["cls_token"].expand(b, 1, d), h], dim=1) + params["pos_embed"]
    t = h.shape[1]
    hd = d // heads
    out = {}
    for i in range(depth):
        pre = f"blocks.{i}."

        def P(name):
            return params[pre + name]

        z = _layer_norm(h, P("norm1.weight"), P("norm1.bias"))
        qkv = (z @ P("attn.qkv.weight").t() + P("attn.qkv.bias")).reshape(b, t, 3, heads, hd)
        q, k, v = (qkv[:, :, j].transpose(1, 2) for j in range(3))               # [B, H, T, hd]
        att = torch.softmax((q @ k.transpose(-2, -1)) * hd ** -0.5, dim=-1) @ v
        a = att.transpose(1, 2).reshape(b, t, d) @ P("attn.proj.weight").t() + P("attn.proj.bias")
        if scales is not None:
            a = a * scales[2 * i].to(torch.float64).view(b, 1, 1)
        h = h + a
        z = _layer_norm(h, P("norm2.weight"), P("norm2.bias"))
        m = _gelu(z @ P("mlp.fc1.weight").t() + P("mlp.fc1.bias")) @ P("mlp.fc2.weight").t() + P("mlp.fc2.bias")
        if scales is not None:
            m = m * scales[2 * i + 1].to(torch.float64).view(b, 1, 1)
        h = h + m
        if i in taps:
            out[i] = h[:, 1:]
    z = _layer_norm(h, params["norm.weight"], params["norm.bias"])
    logits = z[:, 0] @ params["head.weight"].t() + params["head.bias"]
    return logits, out


def drop_path_scales(depth, batch, keep, generator):
    """fp32 [2 * depth, B] scales 0 or 1 / keep with at least one dropped and one kept sample in every row"""
    rows = []
    for _ in range(2 * depth):
        while True:
            m = (torch.rand(batch, generator=generator) < keep).float()
            if 0 < float(m.sum()) < batch:
                break
        rows.append(m / keep)
    return torch.stack(rows)
