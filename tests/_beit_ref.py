"""Plain-torch fp64 restatement of the BEiT teacher (test helper), written independently of the kernel's arithmetic.

* ``meshgrid_index``: the [T, T] table-row matrix built the way timm's ``beit.py`` builds its
  ``relative_position_index`` buffer (from memory of timm 1.0.x, without timm at hand): meshgrid of patch coordinates,
  pairwise differences, shift to non-negative, row-major flattening over (2 gh - 1) x (2 gw - 1), then the three CLS
  fills.  The kernel and ``basd_amd._native.relbias_index`` use closed-form arithmetic per pair instead.
* ``biased_attention``: softmax(q k^T * scale + table[index][h]) v from a packed qkv, with the head-averaged CLS-row tap
  (src/losses/relational.py:22-27 reads that row of the reference's attention map without the CLS column).
* ``beit_forward``: the whole pre-norm model -- patch embedding as unfold @ W^T + b, CLS token, no position embedding
  unless the parameters hold one, LayerNorm, qkv with bias cat(q_bias, 0, v_bias), the biased attention, proj,
  LayerScale when the parameters hold ``ls1.gamma`` / ``ls2.gamma``, exact-erf GELU MLP.  Parameter names are the
  ``state_dict`` keys; a model whose keys are those of the plain ViT (``attn.qkv.bias``, no table) runs unbiased.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F


def table_rows(gh: int, gw: int) -> int:
    return (2 * gh - 1) * (2 * gw - 1) + 3


def meshgrid_index(gh: int, gw: int) -> torch.Tensor:
    rows = table_rows(gh, gw)
    coords = torch.stack(torch.meshgrid(torch.arange(gh), torch.arange(gw), indexing="ij"))     # [2, gh, gw]
    flat = coords.flatten(1)                                                                     # [2, N]
    rel = (flat[:, :, None] - flat[:, None, :]).permute(1, 2, 0).contiguous()                    # [N, N, 2]
    rel[:, :, 0] += gh - 1
    rel[:, :, 1] += gw - 1
    rel[:, :, 0] *= 2 * gw - 1
    index = torch.zeros(gh * gw + 1, gh * gw + 1, dtype=torch.int64)
    index[1:, 1:] = rel.sum(-1)
    index[0, 0:] = rows - 3
    index[0:, 0] = rows - 2
    index[0, 0] = rows - 1
    return index


def seeded_table(gh: int, gw: int, heads: int, seed: int, cls=(-3.0, 2.0, 5.0)) -> torch.Tensor:
    """fp32 [R, heads]: patch rows from N(0, 1.5^2), the three CLS rows set to distinct values (per head shifted by
    0.25 h so that a wrong head stride shows there too)"""
    g = torch.Generator().manual_seed(seed)
    table = 1.5 * torch.randn(table_rows(gh, gw), heads, generator=g)
    for i, v in enumerate(cls):
        table[-3 + i] = v + 0.25 * torch.arange(heads)
    return table


def biased_attention(qkv, table, gh: int, gw: int, heads: int, scale: float):
    """qkv [B, T, 3 * heads * hd] (any float dtype), table [R, heads] or None -> (out [B, T, heads * hd], importance
    [B, T - 1]) in fp64"""
    b, t = qkv.shape[0], qkv.shape[1]
    hd = qkv.shape[-1] // (3 * heads)
    q, k, v = (qkv.detach().cpu().double().reshape(b, t, 3, heads, hd)[:, :, j].transpose(1, 2) for j in range(3))
    logits = (q @ k.transpose(-2, -1)) * scale                                               # [B, H, T, T]
    if table is not None:
        assert t == gh * gw + 1 and tuple(table.shape) == (table_rows(gh, gw), heads)
        logits = logits + table.detach().cpu().double()[meshgrid_index(gh, gw)].permute(2, 0, 1)
    prob = torch.softmax(logits, dim=-1)
    return (prob @ v).transpose(1, 2).reshape(b, t, heads * hd), prob[:, :, 0, 1:].mean(dim=1)


def _layer_norm(x, weight, bias, eps):
    mean = x.mean(dim=-1, keepdim=True)
    var = (x - mean).square().mean(dim=-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * weight + bias


def _gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def fp64_params(state_dict):
    return {k: v.detach().to(device="cpu", dtype=torch.float64) for k, v in state_dict.items()}


def beit_forward(params, images, *, heads: int, eps: float = 1e-6):
    """-> (tokens, importance): per block the output [B, T, D] (CLS row included) and the importance [B, T - 1]"""
    x = images.to(device="cpu", dtype=torch.float64)
    b = x.shape[0]
    w = params["patch_embed.proj.weight"]
    d, p = w.shape[0], w.shape[-1]
    gh, gw = x.shape[2] // p, x.shape[3] // p
    depth = 1 + max(int(k.split(".")[1]) for k in params if k.startswith("blocks."))
    h = F.unfold(x, kernel_size=p, stride=p).transpose(1, 2) @ w.reshape(d, -1).t() + params["patch_embed.proj.bias"]
    h = torch.cat([params["cls_token"].expand(b, 1, d), h], dim=1)
    if "pos_embed" in params:
        h = h + params["pos_embed"]
    tokens, importance = [], []
    for i in range(depth):
        def P(name):
            return params.get(f"blocks.{i}.{name}")

        z = _layer_norm(h, P("norm1.weight"), P("norm1.bias"), eps)
        if P("attn.q_bias") is not None:
            qkv_bias = torch.cat([P("attn.q_bias"), torch.zeros_like(P("attn.q_bias")), P("attn.v_bias")])
        else:
            qkv_bias = P("attn.qkv.bias")
        qkv = z @ P("attn.qkv.weight").t() + qkv_bias
        att, imp = biased_attention(qkv, P("attn.relative_position_bias_table"), gh, gw, heads, (d // heads) ** -0.5)
        a = att @ P("attn.proj.weight").t() + P("attn.proj.bias")
        if P("ls1.gamma") is not None:
            a = a * P("ls1.gamma")
        h = h + a
        z = _layer_norm(h, P("norm2.weight"), P("norm2.bias"), eps)
        m = _gelu(z @ P("mlp.fc1.weight").t() + P("mlp.fc1.bias")) @ P("mlp.fc2.weight").t() + P("mlp.fc2.bias")
        if P("ls2.gamma") is not None:
            m = m * P("ls2.gamma")
        h = h + m
        tokens.append(h)
        importance.append(imp)
    return tokens, importance
