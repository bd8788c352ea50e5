"""Plain-torch fp64 restatement of the DINOv3 ViT teacher (test helper) in DINOv3's OWN form, written independently of
``basd_amd.models.dinov3`` and of the kernels, from memory of facebookresearch/dinov3 (no hub code or timm at hand):

* ``dinov3_angles``: ``RopePositionEmbedding`` -- periods base^(2 j / (hd / 2)), patch-centre coordinates in [-1, 1],
  angles 2 pi coord / period as [HW, 2, hd / 4] flattened to [HW, hd / 2] and TILED twice to [HW, hd].  The model keeps
  a per-pair (cos, sin) table instead.
* ``rope_apply``: ``x cos + rotate_half(x) sin`` with ``rotate_half(x) = cat(-x2, x1)`` of the two halves: the pairs are
  (i, i + hd / 2).  The model permutes its weights and rotates interleaved pairs.
* ``dinov3_forward``: patch embedding as unfold @ W^T + b, ``cat(cls, storage_tokens, patches)`` (no position embedding),
  pre-norm blocks: LayerNorm, qkv with the k third of the bias masked to zero, the rotation of q and k of the tokens
  behind the 1 + R prefix ones, softmax(q k^T hd^-1/2) v, proj, LayerScale applied explicitly, erf-GELU MLP, LayerScale;
  per block the CLS row of the head-averaged attention map without its CLS column.  UNPERMUTED weights under the hub's
  key names.
* ``hub_state_dict``: the random tiny model (dim 128, 2 heads of 64, depth 2, patch 16, 4 storage tokens) as a hub
  checkpoint, with what such a checkpoint carries on top: ``bias_mask`` buffers, a NON-ZERO k bias underneath them,
  ``rope_embed.periods``, ``mask_token``; ``timm_names`` renames it the way timm does.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

DIM, HEADS, DEPTH, PATCH, REG, HIDDEN, BATCH = 128, 2, 2, 16, 4, 512, 2
HD = DIM // HEADS
EPS = 1e-5


def dinov3_angles(gh: int, gw: int, hd: int, base: float = 100.0):
    """-> fp64 [gh * gw, hd]: the angle of every channel, the hd / 2 angles of a patch tiled twice"""
    periods = base ** (2 * torch.arange(hd // 4, dtype=torch.float64) / (hd // 2))
    ch = torch.arange(0.5, gh, dtype=torch.float64) / gh
    cw = torch.arange(0.5, gw, dtype=torch.float64) / gw
    coords = torch.stack(torch.meshgrid(ch, cw, indexing="ij"), dim=-1).flatten(0, 1)      # [HW, 2]
    coords = 2.0 * coords - 1.0
    angles = 2 * math.pi * coords[:, :, None] / periods[None, None, :]                     # [HW, 2, hd / 4]
    return angles.flatten(1, 2).tile(2)


def rotate_half(x):
    x1, x2 = x.chunk(2, dim=-1)
    return torch.cat([-x2, x1], dim=-1)


def rope_apply(x, angles):
    """x [..., HW, hd], angles [HW, hd]"""
    return x * angles.cos() + rotate_half(x) * angles.sin()


def _layer_norm(x, weight, bias, eps):
    mean = x.mean(dim=-1, keepdim=True)
    var = (x - mean).square().mean(dim=-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * weight + bias


def _gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def fp64_params(state_dict):
    return {k: v.detach().to(device="cpu", dtype=torch.float64) for k, v in state_dict.items()}


def dinov3_forward(params, images, *, heads: int = HEADS, eps: float = EPS, rotate: bool = True):
    """params: a hub state dict in fp64 -> (tokens, importance): per block the output [B, 1 + R + N, D] and the
    importance [B, R + N] (the reference strips only the CLS row, so the registers stay)"""
    x = images.to(device="cpu", dtype=torch.float64)
    b = x.shape[0]
    w = params["patch_embed.proj.weight"]
    d, p = w.shape[0], w.shape[-1]
    hd = d // heads
    gh, gw = x.shape[2] // p, x.shape[3] // p
    angles = dinov3_angles(gh, gw, hd)
    depth = 1 + max(int(k.split(".")[1]) for k in params if k.startswith("blocks."))
    h = F.unfold(x, kernel_size=p, stride=p).transpose(1, 2) @ w.reshape(d, -1).t() + params["patch_embed.proj.bias"]
    h = torch.cat([params["cls_token"].expand(b, 1, d), params["storage_tokens"].expand(b, -1, d), h], dim=1)
    t, prefix = h.shape[1], 1 + params["storage_tokens"].shape[1]
    tokens, importance = [], []
    for i in range(depth):
        def P(name):
            return params[f"blocks.{i}.{name}"]

        z = _layer_norm(h, P("norm1.weight"), P("norm1.bias"), eps)
        qkv = (z @ P("attn.qkv.weight").t() + P("attn.qkv.bias") * P("attn.qkv.bias_mask")).reshape(b, t, 3, heads, hd)
        q, k, v = (qkv[:, :, j].transpose(1, 2) for j in range(3))
        if rotate:
            q = torch.cat([q[:, :, :prefix], rope_apply(q[:, :, prefix:], angles)], dim=2)
            k = torch.cat([k[:, :, :prefix], rope_apply(k[:, :, prefix:], angles)], dim=2)
        prob = torch.softmax((q @ k.transpose(-2, -1)) * hd ** -0.5, dim=-1)
        importance.append(prob[:, :, 0, 1:].mean(dim=1))
        a = (prob @ v).transpose(1, 2).reshape(b, t, d) @ P("attn.proj.weight").t() + P("attn.proj.bias")
        h = h + a * P("ls1.gamma")
        z = _layer_norm(h, P("norm2.weight"), P("norm2.bias"), eps)
        m = _gelu(z @ P("mlp.fc1.weight").t() + P("mlp.fc1.bias")) @ P("mlp.fc2.weight").t() + P("mlp.fc2.bias")
        h = h + m * P("ls2.gamma")
        tokens.append(h)
    return tokens, importance


def hub_state_dict(seed: int = 5):
    """the tiny model as an fp32 hub checkpoint"""
    g = torch.Generator().manual_seed(seed)

    def rn(*shape, std=1.0, mean=0.0):
        return mean + std * torch.randn(*shape, generator=g)

    s = {"cls_token": rn(1, 1, DIM, std=0.5), "storage_tokens": rn(1, REG, DIM, std=0.5), "mask_token": rn(1, DIM),
         "patch_embed.proj.weight": rn(DIM, 3, PATCH, PATCH, std=0.03), "patch_embed.proj.bias": rn(DIM, std=0.1),
         "rope_embed.periods": 100.0 ** (2 * torch.arange(HD // 4) / (HD // 2)),
         "norm.weight": rn(DIM, std=0.2, mean=1.0), "norm.bias": rn(DIM, std=0.2)}
    for i in range(DEPTH):
        pre = f"blocks.{i}."
        mask = torch.ones(3 * DIM)
        mask[DIM:2 * DIM] = 0.0
        s.update({
            pre + "norm1.weight": rn(DIM, std=0.2, mean=1.0), pre + "norm1.bias": rn(DIM, std=0.2),
            pre + "attn.qkv.weight": rn(3 * DIM, DIM, std=0.12), pre + "attn.qkv.bias": rn(3 * DIM, std=0.3),
            pre + "attn.qkv.bias_mask": mask,
            pre + "attn.proj.weight": rn(DIM, DIM, std=0.08), pre + "attn.proj.bias": rn(DIM, std=0.1),
            pre + "ls1.gamma": rn(DIM, std=0.2, mean=0.7),
            pre + "norm2.weight": rn(DIM, std=0.2, mean=1.0), pre + "norm2.bias": rn(DIM, std=0.2),
            pre + "mlp.fc1.weight": rn(HIDDEN, DIM, std=0.08), pre + "mlp.fc1.bias": rn(HIDDEN, std=0.1),
            pre + "mlp.fc2.weight": rn(DIM, HIDDEN, std=0.04), pre + "mlp.fc2.bias": rn(DIM, std=0.1),
            pre + "ls2.gamma": rn(DIM, std=0.2, mean=0.7),
        })
    return s


def bf16_exact(state, seed: int = 9):
    """the checkpoint with every tensor rounded to bf16 and the LayerScale factors replaced by powers of two: folding
    LayerScale into the projections and casting to bf16 then changes no value, so the fp64 forward of THIS checkpoint is
    the exact-arithmetic result of the frozen bf16 model's own weights (the GPU tests measure kernel error, not weight
    rounding)"""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for key, value in state.items():
        if key.endswith(("ls1.gamma", "ls2.gamma")):
            out[key] = 2.0 ** torch.randint(-2, 1, value.shape, generator=g).float()
        else:
            out[key] = value.to(torch.bfloat16).float()
    return out


def timm_names(state):
    """the same checkpoint under timm's names: ``reg_token``, ``gamma_1`` / ``gamma_2``"""
    out = {}
    for key, value in state.items():
        key = "reg_token" if key == "storage_tokens" else key.replace(".ls1.gamma", ".gamma_1").replace(".ls2.gamma", ".gamma_2")
        out[key] = value.clone()
    return out


def tiny_dinov3(img: int, state=None):
    """the model code's tiny DINOv3 (fp32, CPU, eval) at ``img`` px with the checkpoint loaded the product's way"""
    from basd_amd.models.dinov3 import Dinov3, load_dinov3_state_dict
    model = Dinov3(img_size=img, patch_size=PATCH, embed_dim=DIM, depth=DEPTH, num_heads=HEADS, reg_tokens=REG)
    missing = load_dinov3_state_dict(model, hub_state_dict() if state is None else state)
    assert missing == [], missing
    return model.eval()
