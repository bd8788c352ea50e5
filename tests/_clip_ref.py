"""Plain-torch fp64 forward of the image-text ViT teachers (test helper).

Written from the public definition of the CLIP / SigLIP vision towers, not from ``basd_amd.models``: patch embedding as
unfold @ W^T (+ b when the model has one), optional CLS token, position embedding, optional ``norm_pre``, then pre-norm
blocks -- LayerNorm, packed qkv in (3, heads, head_dim) order, softmax(Q K^T hd^-1/2) V, proj, MLP with the named
activation -- and per block the head-averaged token importance the reference's attention hook yields
(src/models/teacher.py:27-39 builds softmax(QK^T / sqrt(hd)); src/losses/relational.py:22-27 reads its CLS row without
the CLS column, or its mean over the queries when there is no CLS token).  Parameter names are the ``state_dict`` keys.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F


def layer_norm(x, weight, bias, eps):
    mean = x.mean(dim=-1, keepdim=True)
    var = (x - mean).square().mean(dim=-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * weight + bias


def activation(x, act):
    if act == "gelu":
        return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))
    if act == "quick_gelu":
        return x / (1.0 + torch.exp(-1.702 * x))
    if act == "gelu_tanh":
        return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))
    raise ValueError(act)


def fp64_params(state_dict):
    return {k: v.detach().to(device="cpu", dtype=torch.float64) for k, v in state_dict.items()}


def clip_forward(params, images, *, heads, act, eps):
    """-> (tokens, importance): per block the output [B, T, D] (CLS row included) and the importance [B, N], in fp64.
    ``pre_norm``, the patch bias and the CLS token are taken from which keys ``params`` holds."""
    x = images.to(device="cpu", dtype=torch.float64)
    b = x.shape[0]
    w = params["patch_embed.proj.weight"]
    d, p = w.shape[0], w.shape[-1]
    depth = 1 + max(int(k.split(".")[1]) for k in params if k.startswith("blocks."))
    h = F.unfold(x, kernel_size=p, stride=p).transpose(1, 2) @ w.reshape(d, -1).t()      # [B, N, D]
    if "patch_embed.proj.bias" in params:
        h = h + params["patch_embed.proj.bias"]
    has_cls = "cls_token" in params
    if has_cls:
        h = torch.cat([params["cls_token"].expand(b, 1, d), h], dim=1)
    h = h + params["pos_embed"]
    if "norm_pre.weight" in params:
        h = layer_norm(h, params["norm_pre.weight"], params["norm_pre.bias"], eps)
    t, hd = h.shape[1], d // heads
    tokens, importance = [], []
    for i in range(depth):
        def P(name):
            return params[f"blocks.{i}.{name}"]

        z = layer_norm(h, P("norm1.weight"), P("norm1.bias"), eps)
        qkv = (z @ P("attn.qkv.weight").t() + P("attn.qkv.bias")).reshape(b, t, 3, heads, hd)
        q, k, v = (qkv[:, :, j].transpose(1, 2) for j in range(3))                       # [B, H, T, hd]
        prob = torch.softmax((q @ k.transpose(-2, -1)) * hd ** -0.5, dim=-1)             # [B, H, T, T]
        importance.append(prob[:, :, 0, 1:].mean(dim=1) if has_cls else prob.mean(dim=(1, 2)))
        a = (prob @ v).transpose(1, 2).reshape(b, t, d) @ P("attn.proj.weight").t() + P("attn.proj.bias")
        h = h + a
        z = layer_norm(h, P("norm2.weight"), P("norm2.bias"), eps)
        m = activation(z @ P("mlp.fc1.weight").t() + P("mlp.fc1.bias"), act) @ P("mlp.fc2.weight").t() + P("mlp.fc2.bias")
        h = h + m
        tokens.append(h)
    return tokens, importance
