"""BEiT / BEiT-v2 teachers: ViTs whose attention carries a learned relative-position bias instead of an absolute
position embedding (the reference loads them by name through ``timm.create_model``, src/models/teacher.py:118).

The model is the plain ViT of ``models/vit.py`` -- the same ``Block``, ``Mlp``, ``MixedLayerNorm``, ``PatchEmbed`` and
``BasdLinear`` -- with three differences: no ``pos_embed``; LayerScale on both branches (timm's ``gamma_1`` /
``gamma_2``, here ``ls1.gamma`` / ``ls2.gamma`` so that ``fold_layerscale`` folds them and the frozen blocks take the
fused inference path); and ``RelPosAttention``, which adds ``relative_position_bias_table[index(i, j)][head]`` to the
logit of query i and key j.  On the device a frozen bf16 block runs ``basd_attention_fwd_relbias_bf16`` up to 272 tokens
and ``basd_attention_fwd_long_relbias_bf16`` (the tiled kernels) from there to 1024 tokens -- 384 px at patch 16 has
577: the bias is gathered inside the attention kernel from the head's column of the table, the CLS-row tap is a
by-product, and no [T, T] or [H, T, T] bias exists in memory.  Everywhere else (CPU, fp32, gradients, T > 1024, head dim
!= 64) the torch path builds the dense bias from an index buffer; on the device that is a counted library fallback.

WRITTEN WITHOUT timm AT HAND, from memory of timm 1.0.x ``beit.py``: the index rule (``relbias_index`` in
``_native.py``: pairwise coordinate differences shifted to be non-negative, row-major over (2 gh - 1) x (2 gw - 1), then
three extra rows for CLS-to-patch, patch-to-CLS and CLS-to-CLS), the parameter names (``q_bias``, ``v_bias``,
``relative_position_bias_table``, ``gamma_1`` / ``gamma_2``), the absence of a k bias, and the presets below with their
normalisation statistics.  Check them against the installed timm (its ``relative_position_index`` buffer, its
``default_cfgs``) before loading real weights.  Not built: a shared relative-position bias across blocks, ``fc_norm``
and ``head`` (a teacher never uses them), table resampling between resolutions.
"""
from __future__ import annotations

import functools
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..losses._ops import get_ops, library_fallback
from .vit import HALF_MEAN, HALF_STD, IMAGENET_MEAN, IMAGENET_STD, Block, MixedLayerNorm, PatchEmbed, QVBiasAttention

# 0: dense bias + library SDPA + separate tap on the device too (A/B runs: scripts/time_beit_teacher.py flips it inside
# one process)
_FUSED_RELBIAS_ATTENTION = os.environ.get("BASD_FUSED_RELBIAS", "1") == "1"


def relative_position_index(gh: int, gw: int) -> torch.Tensor:
    """[T, T] int64, T = gh * gw + 1: ``relbias_index`` for every pair of tokens, vectorised"""
    rows = (2 * gh - 1) * (2 * gw - 1) + 3
    p = torch.arange(gh * gw)
    y, x = p // gw, p % gw
    index = torch.empty(gh * gw + 1, gh * gw + 1, dtype=torch.int64)
    index[1:, 1:] = (y[:, None] - y[None, :] + gh - 1) * (2 * gw - 1) + (x[:, None] - x[None, :] + gw - 1)
    index[0, 1:], index[1:, 0], index[0, 0] = rows - 3, rows - 2, rows - 1
    return index


class RelPosAttention(QVBiasAttention):
    """timm Beit ``Attention`` (``QVBiasAttention``) with ``relative_position_bias_table``
    [(2 gh - 1)(2 gw - 1) + 3, heads], kept in fp32 whatever the model is cast to."""
    _fp32_name = "relative_position_bias_table"

    def __init__(self, dim: int, num_heads: int, window_size: tuple = (14, 14)):
        super().__init__(dim, num_heads)
        self.window_size = gh, gw = int(window_size[0]), int(window_size[1])
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * gh - 1) * (2 * gw - 1) + 3, num_heads))
        self.register_buffer("relative_position_index", relative_position_index(gh, gw), persistent=False)

    def _dense_bias(self, t: int) -> torch.Tensor:
        """[heads, T, T] fp32 (torch path only)"""
        table = self.relative_position_bias_table
        return table[self.relative_position_index.reshape(-1)].reshape(t, t, -1).permute(2, 0, 1)

    def _importance(self, q, k, has_cls: bool, bias=None):
        """``Attention._importance`` with the bias on the logits"""
        if bias is None:
            return super()._importance(q, k, has_cls)
        if has_cls:
            logits = (q[:, :, :1] @ k.transpose(-2, -1)).float() * self.scale + bias[:, :1].float()     # [B,H,1,T]
            return logits.softmax(dim=-1)[:, :, 0, 1:].mean(dim=1)
        attn = ((q.float() @ k.float().transpose(-2, -1)) * self.scale + bias.float()).softmax(dim=-1)
        return attn.mean(dim=(1, 2))

    def forward(self, x):
        b, t, c = x.shape
        gh, gw = self.window_size
        if t != gh * gw + 1:
            raise ValueError(f"RelPosAttention: {t} tokens, but the bias table is for a {gh} x {gw} grid + CLS "
                             f"({gh * gw + 1} tokens); tables are not resampled")
        qkv_flat = self._qkv(x)
        table = self.relative_position_bias_table
        ops = get_ops()
        on_device = ops.handles(qkv_flat)
        has_cls = self.tap is None or bool(self.tap["has_cls"])
        if (_FUSED_RELBIAS_ATTENTION and on_device and not torch.is_grad_enabled() and qkv_flat.dtype == torch.bfloat16
                and table.dtype == torch.float32 and has_cls):
            # frozen block: fused attention with the bias gathered in the kernel, the tap as a by-product
            # (csrc/attention.hip; past its 272 tokens the tiled kernels of csrc/attention_long.hip)
            out = self._fused_frozen(
                ((ops.attention_fwd_relbias_supported(gh, gw, self.head_dim), ops.attention_fwd_relbias),
                 (ops.attention_fwd_long_relbias_supported(gh, gw, self.head_dim), ops.attention_fwd_long_relbias)),
                qkv_flat, table, gh, gw)
            if out is not None:
                return out
        if on_device:
            library_fallback("attention (relative bias)", f"grid={gh}x{gw} head_dim={self.head_dim} "
                                                          f"dtype={qkv_flat.dtype} grad={torch.is_grad_enabled()}")
        q, k, v = qkv_flat.reshape(b, t, 3, self.num_heads, self.head_dim).permute(2, 0, 3, 1, 4).unbind(0)
        bias = self._dense_bias(t)
        if self.tap is not None:
            self.tap["out"] = self._importance(q, k, self.tap["has_cls"], bias)
        out = F.scaled_dot_product_attention(q, k, v, attn_mask=bias.unsqueeze(0).to(q.dtype))
        return self.proj(out.transpose(1, 2).reshape(b, t, c))


class Beit(nn.Module):
    """timm ``Beit`` without its head: patch embedding, CLS token, pre-norm LayerScale blocks with ``RelPosAttention``,
    final norm.  Parameter names follow timm except ``blocks.i.gamma_1`` / ``gamma_2`` (here ``ls1.gamma`` /
    ``ls2.gamma``; ``load_timm_state_dict`` maps them)."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, num_classes=0, embed_dim=768, depth=12, num_heads=12,
                 mlp_ratio=4.0, init_values=0.1, norm_eps=1e-6):
        super().__init__()
        if num_classes:
            raise ValueError("Beit: only the headless model (num_classes=0) is built: a teacher never uses the head")
        self.embed_dim = self.num_features = embed_dim
        self.num_classes = 0
        self.patch_embed = PatchEmbed(img_size, patch_size, in_chans, embed_dim)
        self.grid = (img_size // patch_size, img_size // patch_size)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        attn_cls = functools.partial(RelPosAttention, window_size=self.grid)
        self.blocks = nn.ModuleList([
            Block(embed_dim, num_heads, mlp_ratio, 0.0, init_values, eps=norm_eps, attn_cls=attn_cls)
            for _ in range(depth)])
        self.norm = MixedLayerNorm(embed_dim, eps=norm_eps)
        for i, blk in enumerate(self.blocks):
            blk._next_norm.append(self.blocks[i + 1].norm1 if i + 1 < depth else self.norm)
        nn.init.normal_(self.cls_token, std=0.02)
        for blk in self.blocks:
            nn.init.normal_(blk.attn.relative_position_bias_table, std=0.02)

    def materialize_qkv_bias(self) -> None:
        for blk in self.blocks:
            blk.attn.materialize_qkv_bias()

    def forward_features(self, x):
        x = self.patch_embed(x)
        x = torch.cat([self.cls_token.expand(x.shape[0], -1, -1).to(x.dtype), x], dim=1)
        for blk in self.blocks:
            x = blk(x)
        return self.norm(x)

    def forward(self, x):
        return self.forward_features(x)[:, 0]


# name -> (embed_dim, depth, heads, patch, layerscale init, mean, std).  Written WITHOUT timm at hand, from memory of
# timm 1.0.x (beit.py model entrypoints and default_cfgs): BEiT-v2 is normalised with ImageNet's statistics, BEiT v1
# with 0.5 / 0.5 -- check both, and the LayerScale inits (which only matter without weights), against the installed
# timm before loading real weights.
BEIT_PRESETS = {
    "beit_base_patch16_224": (768, 12, 12, 16, 0.1, HALF_MEAN, HALF_STD),
    "beit_large_patch16_224": (1024, 24, 16, 16, 1e-5, HALF_MEAN, HALF_STD),
    "beitv2_base_patch16_224": (768, 12, 12, 16, 1e-5, IMAGENET_MEAN, IMAGENET_STD),
    "beitv2_large_patch16_224": (1024, 24, 16, 16, 1e-5, IMAGENET_MEAN, IMAGENET_STD),
    # the 384 px fine-tunes of BEiT v1 (24 x 24 grid, 577 tokens: the tiled attention), from memory of timm like the
    # rest: the architecture and the 0.5 / 0.5 statistics of their 224 px namesakes.  A checkpoint must arrive with the
    # 47 x 47 + 3 row table of that grid (tables are not resampled).  beit_large_patch16_512 (1025 tokens) is not here.
    "beit_base_patch16_384": (768, 12, 12, 16, 0.1, HALF_MEAN, HALF_STD),
    "beit_large_patch16_384": (1024, 24, 16, 16, 1e-5, HALF_MEAN, HALF_STD),
}

# keys of a timm checkpoint that have no counterpart here: the index is rebuilt from the grid, the head is not built
_DROPPED = ("attn.relative_position_index", "fc_norm.", "head.")


def create_beit(name: str, *, img_size: int, patch_size: int | None = None, **overrides) -> Beit:
    """timm.create_model stand-in for the presets above (``overrides``: embed_dim, depth, num_heads, mlp_ratio)"""
    if name not in BEIT_PRESETS:
        raise ValueError(f"unknown BEiT preset {name!r}; known: {sorted(BEIT_PRESETS)}")
    dim, depth, heads, patch, init_values, _, _ = BEIT_PRESETS[name]
    kw = dict(embed_dim=dim, depth=depth, num_heads=heads, mlp_ratio=4.0)
    kw.update({k: v for k, v in overrides.items() if k in kw})
    return Beit(img_size=img_size, patch_size=patch_size or patch, num_classes=0, init_values=init_values, **kw)


def load_timm_state_dict(model: Beit, state: dict):
    """Load a timm Beit state dict: ``blocks.i.gamma_1`` / ``gamma_2`` -> ``ls1.gamma`` / ``ls2.gamma``; the index
    buffers, ``fc_norm.*`` and ``head.*`` are dropped.  A bias table made for another grid is an error (tables are not
    resampled).  -> (missing keys, dropped keys).  The mean-pooled checkpoints carry their final norm as ``fc_norm``
    (from memory of timm): ``norm.*`` is then missing and stays at its identity initialisation, which the teacher's
    per-block taps never read."""
    mapped, dropped = {}, []
    gh, gw = model.grid
    rows = (2 * gh - 1) * (2 * gw - 1) + 3
    for key, value in state.items():
        if any(key.startswith(d) or f".{d}" in key for d in _DROPPED):
            dropped.append(key)
            continue
        if key.endswith(".gamma_1") or key.endswith(".gamma_2"):
            key = key[:-len("gamma_1")] + ("ls1.gamma" if key.endswith("1") else "ls2.gamma")
        if key.endswith("attn.relative_position_bias_table") and value.shape[0] != rows:
            raise ValueError(f"{key}: {value.shape[0]} rows, but a {gh} x {gw} patch grid (img_size "
                             f"{model.patch_embed.img_size}, patch {model.patch_embed.patch_size}) needs "
                             f"(2 * {gh} - 1) * (2 * {gw} - 1) + 3 = {rows}; relative-position tables are not resampled")
        mapped[key] = value
    missing, unexpected = model.load_state_dict(mapped, strict=False)
    if unexpected:
        raise ValueError(f"load_timm_state_dict: keys without a counterpart in Beit: {sorted(unexpected)}")
    return list(missing), dropped
