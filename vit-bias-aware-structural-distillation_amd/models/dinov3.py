"""DINOv3 ViT teachers (S / B / L at patch 16): the successor of the reference's default teacher ``dinov2_vitb14``
(configs/config.yaml:38; the reference loads any name through ``timm.create_model``, src/models/teacher.py:118).  At
/16 and 224 px the 14 x 14 patch grid is the DeiT student's own.

The model is the plain ViT of ``models/vit.py`` -- the same ``Block``, ``Mlp``, ``LayerScale`` (folded into the
projections by ``fold_layerscale``), ``MixedLayerNorm``, ``PatchEmbed`` and ``BasdLinear`` -- with three differences: no
absolute position embedding, a CLS token followed by four register ("storage") tokens, and a rotary embedding of q and k
of the patch tokens inside every attention (``RopeAttention`` of ``models/eva.py`` with DINOv3's angles,
``dinov3_rope_table``).  The qkv layer has a bias whose k third is masked to zero.

ONE ROTATION KERNEL.  DINOv3 rotates the half-split pairs (i, i + hd / 2) of every head: ``x cos + rotate_half(x) sin``
with the hd / 2 angles tiled twice.  The logits q . k do not change when the channels of q and k of a head are permuted
alike, so ``interleave_rope_pairs`` permutes the q and k rows of the qkv weight and bias once after the checkpoint is
loaded, in fp32 before the bf16 cast (new channel 2 i = old i, new channel 2 i + 1 = old i + hd / 2), and zeroes the k
bias in the same step.  The interleaved-pair kernels of EVA-02 (``basd_attention_fwd_rope_bf16`` up to 272 tokens,
``basd_attention_fwd_long_rope_bf16`` up to 1024) then compute DINOv3's attention exactly; v and ``proj`` are untouched.
A state dict of THIS model is therefore not in DINOv3's channel order: ``load_dinov3_state_dict`` takes checkpoints in
DINOv3's own order (the hub's or timm's) only.

On the device the frozen bf16 model assembles its tokens with ``basd_vit_embed_reg_bf16`` and an all-zero position
table (x + 0 is exact), and its blocks run the fused inference path of ``Block``: no library fallback in strict mode
from 2 to 1024 tokens.

WRITTEN WITHOUT the hub code or timm AT HAND, from memory of facebookresearch/dinov3 (``vision_transformer.py``,
``rope_position_encoding.py``, ``LinearKMaskedBias``) and timm 1.0.x: the presets below (width, depth, heads, four
storage tokens, LayerNorm eps 1e-5, LayerScale, GELU MLP of ratio 4, ImageNet statistics for the ``lvd1689m`` weights),
the angle rule (base 100, coordinates in [-1, 1], see ``dinov3_rope_table``), the half-split pairing and the key names
(``storage_tokens`` / ``reg_token``, ``ls1.gamma`` / ``gamma_1``, ``attn.qkv.bias_mask``, ``rope_embed.periods``).  Check
them against the checkpoint before loading real weights.  Not built: the SwiGLU models (S+, H+), the 7B model, the
ConvNeXt DINOv3s, the ``sat493m`` normalisation statistics, the rope augmentations (shift / jitter / rescale: training
only).
"""
from __future__ import annotations

import functools

import torch
import torch.nn as nn

from .._native import dinov3_rope_table
from ..losses._ops import get_ops
from . import eva as _eva
from .eva import RopeAttention
from .vit import IMAGENET_MEAN, IMAGENET_STD, Attention, Block, MixedLayerNorm, PatchEmbed

REG_TOKENS = 4


class Dinov3Attention(RopeAttention):
    """``SelfAttention`` of DINOv3 on ``RopeAttention``'s forward: a qkv layer WITH a bias (k third zero), q and k of
    the patch tokens rotated by the rows of ``rope`` (``dinov3_rope_table``; CLS and registers: identity rows).  The
    forward is right once ``interleave_rope_pairs`` has run.  It skips ``QVBiasAttention.__init__`` and so has no
    ``q_bias`` / ``v_bias``: its ``qkv.bias`` is never None, which is why ``_qkv`` never asks for them."""

    def __init__(self, dim: int, num_heads: int, grid: tuple = (14, 14), rope_base: float = 100.0,
                 prefix_tokens: int = 1 + REG_TOKENS):
        Attention.__init__(self, dim, num_heads, qkv_bias=True)
        self.grid = int(grid[0]), int(grid[1])
        self.register_buffer("rope", dinov3_rope_table(*self.grid, self.head_dim, base=rope_base,
                                                       prefix_tokens=prefix_tokens), persistent=False)
        self.pairs_interleaved = False

    @torch.no_grad()
    def interleave_rope_pairs(self) -> None:
        """the counterpart of ``RopeAttention.materialize_qkv_bias``: q and k rows of every head go from DINOv3's
        half-split order to interleaved pairs (new 2 i = old i, new 2 i + 1 = old i + hd / 2) and the k bias becomes
        zero (DINOv3's ``bias_mask``).  A second call changes nothing."""
        if self.pairs_interleaved:
            return
        dim, hd = self.qkv.in_features, self.head_dim
        within = torch.stack([torch.arange(hd // 2), torch.arange(hd // 2) + hd // 2], dim=1).reshape(-1)    # [hd]
        rows = (torch.arange(2 * self.num_heads)[:, None] * hd + within[None, :]).reshape(-1)               # q, k
        rows = rows.to(self.qkv.weight.device)
        self.qkv.weight[:2 * dim] = self.qkv.weight[rows]
        self.qkv.bias[:2 * dim] = self.qkv.bias[rows]
        self.qkv.bias[dim:2 * dim] = 0
        self.pairs_interleaved = True


class Dinov3(nn.Module):
    """``DinoVisionTransformer`` of DINOv3 without its head: patch embedding, CLS token, ``reg_token`` (timm's name; the
    hub says ``storage_tokens``), pre-norm blocks with ``Dinov3Attention``, a GELU ``Mlp`` and LayerScale, final
    norm.  Token order: CLS, registers, patches."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, num_classes=0, embed_dim=768, depth=12, num_heads=12,
                 mlp_ratio=4.0, init_values=1.0, norm_eps=1e-5, reg_tokens=REG_TOKENS, rope_base=100.0):
        super().__init__()
        if num_classes:
            raise ValueError("Dinov3: only the headless model (num_classes=0) is built: a teacher never uses the head")
        self.embed_dim = self.num_features = embed_dim
        self.num_classes = 0
        self.patch_embed = PatchEmbed(img_size, patch_size, in_chans, embed_dim)
        self.grid = (img_size // patch_size, img_size // patch_size)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.reg_token = nn.Parameter(torch.zeros(1, reg_tokens, embed_dim))
        # the position table of basd_vit_embed_reg_bf16 (CLS row + patch rows): DINOv3 has none, x + 0 is exact
        self.register_buffer("zero_pos", torch.zeros(1, 1 + self.patch_embed.num_patches, embed_dim), persistent=False)
        attn_cls = functools.partial(Dinov3Attention, grid=self.grid, rope_base=rope_base,
                                     prefix_tokens=1 + reg_tokens)
        self.blocks = nn.ModuleList([
            Block(embed_dim, num_heads, mlp_ratio, init_values=init_values, eps=norm_eps, attn_cls=attn_cls)
            for _ in range(depth)])
        self.norm = MixedLayerNorm(embed_dim, eps=norm_eps)
        for i, blk in enumerate(self.blocks):
            blk._next_norm.append(self.blocks[i + 1].norm1 if i + 1 < depth else self.norm)
        nn.init.normal_(self.cls_token, std=0.02)
        nn.init.normal_(self.reg_token, std=0.02)

    def interleave_rope_pairs(self) -> None:
        for blk in self.blocks:
            blk.attn.interleave_rope_pairs()

    def _fused_embed_ok(self, x) -> bool:
        """frozen bf16 model on the device: CLS row, register rows and patch rows in one kernel (csrc/vit_embed.hip)"""
        return (_eva._FUSED_EVA_DISPATCH and not torch.is_grad_enabled() and x.dtype == torch.bfloat16 and x.dim() == 3
                and get_ops().handles(x) and self.cls_token.dtype == torch.bfloat16
                and self.reg_token.dtype == torch.bfloat16 and self.zero_pos.dtype == torch.bfloat16
                and x.shape[1] + 1 == self.zero_pos.shape[1] and get_ops().vit_embed_supported(x.shape[-1]))

    def forward_features(self, x):
        x = self.patch_embed(x)
        if self._fused_embed_ok(x):
            x = get_ops().vit_embed(x, self.cls_token, self.zero_pos, reg=self.reg_token)
        else:
            b = x.shape[0]
            x = torch.cat([self.cls_token.expand(b, -1, -1).to(x.dtype), self.reg_token.expand(b, -1, -1).to(x.dtype), x],
                          dim=1)
        for blk in self.blocks:
            x = blk(x)
        return self.norm(x)

    def forward(self, x):
        return self.forward_features(x)[:, 0]


# name -> (embed_dim, depth, heads, patch, mean, std).  Written WITHOUT the hub code or timm at hand (see the module
# docstring): every model has head dim 64, 1 CLS + 4 register tokens, LayerScale, a GELU MLP of ratio 4, LayerNorm eps
# 1e-5 and rope base 100; the ``lvd1689m`` weights are normalised with ImageNet's statistics.
DINOV3_PRESETS = {
    "vit_small_patch16_dinov3": (384, 12, 6, 16, IMAGENET_MEAN, IMAGENET_STD),
    "vit_base_patch16_dinov3": (768, 12, 12, 16, IMAGENET_MEAN, IMAGENET_STD),
    "vit_large_patch16_dinov3": (1024, 24, 16, 16, IMAGENET_MEAN, IMAGENET_STD),
}
for _hub, _timm in (("dinov3_vits16", "vit_small_patch16_dinov3"), ("dinov3_vitb16", "vit_base_patch16_dinov3"),
                    ("dinov3_vitl16", "vit_large_patch16_dinov3")):
    DINOV3_PRESETS[_hub] = DINOV3_PRESETS[_timm]


def create_dinov3(name: str, *, img_size: int, patch_size: int | None = None, **overrides) -> Dinov3:
    """timm.create_model / torch.hub.load stand-in for the presets above (``overrides``: embed_dim, depth, num_heads,
    mlp_ratio)"""
    if name not in DINOV3_PRESETS:
        raise ValueError(f"unknown DINOv3 preset {name!r}; known: {sorted(DINOV3_PRESETS)}")
    dim, depth, heads, patch, _, _ = DINOV3_PRESETS[name]
    kw = dict(embed_dim=dim, depth=depth, num_heads=heads, mlp_ratio=4.0)
    kw.update({k: v for k, v in overrides.items() if k in kw})
    return Dinov3(img_size=img_size, patch_size=patch_size or patch, num_classes=0, **kw)


# keys of a checkpoint that have no counterpart here: the k-bias mask is applied by interleave_rope_pairs, the periods
# are rebuilt from the preset, the iBOT mask embedding is unused in a forward without masks
_DROPPED_SUFFIXES = (".bias_mask",)
_DROPPED_KEYS = ("rope_embed.periods", "mask_token")
_RENAMED = (("storage_tokens", "reg_token"), (".gamma_1", ".ls1.gamma"), (".gamma_2", ".ls2.gamma"))


def dinov3_state_dict(state: dict) -> dict:
    """A DINOv3 state dict under the hub's or timm's key names -> this model's names (``storage_tokens`` ->
    ``reg_token``, ``gamma_1`` / ``gamma_2`` -> ``ls1.gamma`` / ``ls2.gamma``; ``bias_mask`` buffers,
    ``rope_embed.periods`` and ``mask_token`` dropped).  The values keep DINOv3's channel order."""
    out = {}
    for key, value in state.items():
        if key in _DROPPED_KEYS or key.endswith(_DROPPED_SUFFIXES):
            continue
        for old, new in _RENAMED:
            if key == old or (old.startswith(".") and key.endswith(old)):
                key = new if key == old else key[:-len(old)] + new
                break
        out[key] = value
    return out


def load_dinov3_state_dict(model: Dinov3, state: dict) -> list:
    """``dinov3_state_dict`` + ``load_state_dict`` + ``interleave_rope_pairs`` (of the loaded weights, in their own
    dtype: call it before the bf16 cast); -> missing keys.  A key without a counterpart is an error."""
    missing, unexpected = model.load_state_dict(dinov3_state_dict(state), strict=False)
    if unexpected:
        raise ValueError(f"load_dinov3_state_dict: keys without a counterpart in Dinov3: {sorted(unexpected)}")
    for blk in model.blocks:
        blk.attn.pairs_interleaved = False
    model.interleave_rope_pairs()
    return list(missing)
