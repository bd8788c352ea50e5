"""Plain-torch references for the DINOv2 family (test helper): register tokens and the SwiGLU MLP.

Written from the public definition of the DINOv2 forward, not from ``basd_amd.models``: patch embedding as
unfold @ W^T + b, ``cat(cls, patches) + pos_embed``, then R register rows placed behind the CLS row WITHOUT a position
row, pre-norm blocks (LayerNorm, packed qkv in (3, heads, head_dim) order, softmax(Q K^T hd^-1/2) V, proj, LayerScale
when the block has one) whose MLP is fc1 -> erf-GELU -> fc2 or ``w3(silu(x1) * x2)`` with ``x1, x2 = w12(x).chunk(2)``,
and per block the importance the reference reads: the CLS row of the head-averaged attention map without the CLS column
(src/models/teacher.py:27-39, src/losses/relational.py:22-27) -- R + N entries, the registers included, because the
reference strips only the CLS row (teacher.py:151-158).  Parameter names are the ``state_dict`` keys.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from tests._clip_ref import activation, fp64_params, layer_norm  # noqa: F401  (fp64_params: re-exported)


def embed_reg_emulation(patches, cls, reg, pos, gamma=None, beta=None, eps=1e-6):
    """what basd_vit_embed_reg_bf16 is specified to write, as torch ops on bf16 tensors: patches [B, N, D], cls [D] |
    None, reg [R, D] | None (R = 0), pos [1 + N, D] (or [N, D] without a CLS token) -> [B, 1 + R + N, D] bf16.  The
    sums are torch's bf16 adds (fp32 sum, one rounding); the register rows are copied.  With gamma / beta the rounded
    rows are layer-normalised in fp32 and rounded once (the yardstick of the GPU test is fp64, not this)."""
    b, _, d = patches.shape
    x = patches
    if cls is not None:
        x = torch.cat([cls.reshape(1, 1, d).expand(b, -1, -1), x], dim=1)
    x = x + pos.reshape(1, -1, d)
    if reg is not None and reg.numel():
        assert cls is not None, "register rows stand behind a CLS row"
        x = torch.cat([x[:, :1], reg.reshape(1, -1, d).expand(b, -1, -1), x[:, 1:]], dim=1)
    if gamma is None:
        return x
    return F.layer_norm(x.float(), (d,), gamma.float(), beta.float(), eps).to(torch.bfloat16)


def swiglu_unpack_index(h):
    """inverse of the documented row map of basd_gemm_bf16_swiglu: for every hub row s * H + i its packed row
    64 * (i // 32) + 32 * s + i % 32, written out with loops"""
    idx = torch.empty(2 * h, dtype=torch.long)
    for s in range(2):
        for i in range(h):
            idx[s * h + i] = 64 * (i // 32) + 32 * s + i % 32
    return idx


def dinov2_forward(params, images, *, heads, eps=1e-6):
    """-> (tokens, importance, cls_prob): per block the output [B, 1 + R + N, D], the importance [B, R + N] and the
    CLS -> CLS probability [B] (head mean), all fp64.  Registers, SwiGLU and LayerScale are taken from which keys
    ``params`` holds (``reg_token``, ``blocks.i.mlp.w12.weight``, ``blocks.i.ls1.gamma``)."""
    x = images.to(device="cpu", dtype=torch.float64)
    b = x.shape[0]
    w = params["patch_embed.proj.weight"]
    d, p = w.shape[0], w.shape[-1]
    depth = 1 + max(int(k.split(".")[1]) for k in params if k.startswith("blocks."))
    h = F.unfold(x, kernel_size=p, stride=p).transpose(1, 2) @ w.reshape(d, -1).t() + params["patch_embed.proj.bias"]
    h = torch.cat([params["cls_token"].expand(b, 1, d), h], dim=1) + params["pos_embed"]
    if "reg_token" in params:
        h = torch.cat([h[:, :1], params["reg_token"].expand(b, -1, d), h[:, 1:]], dim=1)
    t, hd = h.shape[1], d // heads
    tokens, importance, cls_prob = [], [], []
    for i in range(depth):
        def P(name):
            return params[f"blocks.{i}.{name}"]

        z = layer_norm(h, P("norm1.weight"), P("norm1.bias"), eps)
        qkv = (z @ P("attn.qkv.weight").t() + P("attn.qkv.bias")).reshape(b, t, 3, heads, hd)
        q, k, v = (qkv[:, :, j].transpose(1, 2) for j in range(3))
        prob = torch.softmax((q @ k.transpose(-2, -1)) * hd ** -0.5, dim=-1)
        importance.append(prob[:, :, 0, 1:].mean(dim=1))
        cls_prob.append(prob[:, :, 0, 0].mean(dim=1))
        a = (prob @ v).transpose(1, 2).reshape(b, t, d) @ P("attn.proj.weight").t() + P("attn.proj.bias")
        if f"blocks.{i}.ls1.gamma" in params:
            a = a * P("ls1.gamma")
        h = h + a
        z = layer_norm(h, P("norm2.weight"), P("norm2.bias"), eps)
        if f"blocks.{i}.mlp.w12.weight" in params:
            x1, x2 = (z @ P("mlp.w12.weight").t() + P("mlp.w12.bias")).chunk(2, dim=-1)
            m = (x1 / (1.0 + torch.exp(-x1)) * x2) @ P("mlp.w3.weight").t() + P("mlp.w3.bias")
        else:
            m = activation(z @ P("mlp.fc1.weight").t() + P("mlp.fc1.bias"), "gelu") @ P("mlp.fc2.weight").t() + P("mlp.fc2.bias")
        if f"blocks.{i}.ls2.gamma" in params:
            m = m * P("ls2.gamma")
        h = h + m
        tokens.append(h)
    return tokens, importance, cls_prob
