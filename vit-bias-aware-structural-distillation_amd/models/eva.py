"""EVA-02 teachers: plain ViTs whose attention rotates q and k of the patch tokens with a 2-D rotary position embedding
(the reference loads them by name through ``timm.create_model``, src/models/teacher.py:118).

The model is the plain ViT of ``models/vit.py`` -- the same ``Block``, ``MixedLayerNorm``, ``PatchEmbed`` and
``BasdLinear`` -- with three differences: ``RopeAttention`` (q / v biases without a k bias as in BEiT, and the pairwise
rotation of q and k by per-token angles; the CLS token is not rotated), ``EvaMlp`` (SwiGLU with separate gate and value
layers ``fc1_g`` / ``fc1_x`` and, for the base model, a LayerNorm between the gate and ``fc2``: "sub-LN") and both an
absolute position embedding and the rotary one.  On the device a frozen bf16 block runs
``basd_attention_fwd_rope_bf16``: q and k are rotated in registers inside the attention kernel from an fp32 (cos, sin)
table, the CLS-row tap is a by-product, and no rotated copy of q or k exists in memory; past that kernel's 272 tokens
(336 and 384 px inputs) ``basd_attention_fwd_long_rope_bf16`` does the same on the tiled kernels, up to 1024 tokens.  The
MLP runs ``basd_gemm_bf16_swiglu`` on a packed [fc1_g; fc1_x] image built once, the LayerNorm kernel and the fc2 GEMM.
Everywhere else (CPU, fp32, gradients, T > 1024, head dim != 64) torch ops rotate q and k in front of SDPA and the MLP
is the unfused composition; on the device both are counted library fallbacks.

WRITTEN WITHOUT timm AT HAND, from memory of timm 1.0.x ``eva.py`` and ``pos_embed_sincos.py``: the angle rule
(``rope_table`` in ``_native.py``), the interleaved pairing (2i, 2i + 1), the parameter names (``q_bias``, ``v_bias``,
``fc1_g``, ``fc1_x``, ``mlp.norm``; ``q_proj`` / ``k_proj`` / ``v_proj`` in the base checkpoint) and the presets below
with their normalisation statistics.  Check them against the installed timm (its ``rope`` embedding, its
``default_cfgs``) before loading real weights.  Not built: ``eva02_large`` (hidden width 2730 fits neither the gated
GEMM nor the LayerNorm kernel), EVA-01 and the EVA-CLIP towers, ``fc_norm`` and ``head``, position-embedding
resampling, half-split rotation.
"""
from __future__ import annotations

import functools
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from .._native import rope_table
from ..losses._ops import get_ops, library_fallback
from .linear import BasdLinear
from .vit import CLIP_MEAN, CLIP_STD, Block, MixedLayerNorm, PatchEmbed, QVBiasAttention

# 0: torch rotation + library SDPA + separate tap, unfused SwiGLU, torch token assembly on the device too (A/B runs:
# scripts/time_eva_teacher.py flips it inside one process)
_FUSED_EVA_DISPATCH = os.environ.get("BASD_FUSED_EVA", "1") == "1"


def apply_rope(x: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
    """x [..., T, hd], table [T, hd / 2, 2] (cos, sin) -> the pairs (x[2i], x[2i + 1]) of every token rotated by its
    angles, computed in fp32 (fp64 for fp64 inputs) and returned in x's dtype (torch path only)"""
    wide = torch.promote_types(x.dtype, torch.float32)
    pairs = x.to(wide).unflatten(-1, (-1, 2))
    a, b = pairs[..., 0], pairs[..., 1]
    c, s = table[..., 0].to(wide), table[..., 1].to(wide)
    return torch.stack([a * c - b * s, b * c + a * s], dim=-1).flatten(-2).to(x.dtype)


class RopeAttention(QVBiasAttention):
    """timm ``EvaAttention`` (``QVBiasAttention``): q and k rotated by the rows of ``rope`` -- fp32
    [prefix + gh gw, hd / 2, 2], a non-persistent buffer kept in fp32 whatever the model is cast to (the angles of a
    16 x 16 grid do not survive 8 bits of mantissa)."""
    _fp32_name = "rope"

    def __init__(self, dim: int, num_heads: int, grid: tuple = (16, 16), ref_grid: tuple | None = None,
                 prefix_tokens: int = 1):
        super().__init__(dim, num_heads)
        self.grid = int(grid[0]), int(grid[1])
        self.register_buffer("rope", rope_table(*self.grid, self.head_dim, ref_grid=ref_grid,
                                                prefix_tokens=prefix_tokens), persistent=False)

    def forward(self, x):
        b, t, c = x.shape
        rope = self.rope
        if t != rope.shape[0]:
            raise ValueError(f"RopeAttention: {t} tokens, but the rotary table is for a {self.grid[0]} x {self.grid[1]} "
                             f"grid + prefix ({rope.shape[0]} tokens)")
        qkv_flat = self._qkv(x)
        ops = get_ops()
        on_device = ops.handles(qkv_flat)
        has_cls = self.tap is None or bool(self.tap["has_cls"])
        if (_FUSED_EVA_DISPATCH and on_device and not torch.is_grad_enabled() and qkv_flat.dtype == torch.bfloat16
                and rope.dtype == torch.float32 and has_cls):
            # frozen block: fused attention with q and k rotated in the kernel, the tap as a by-product
            # (csrc/attention.hip; past its 272 tokens the tiled kernel of csrc/attention_long.hip)
            out = self._fused_frozen(
                ((ops.attention_fwd_rope_supported(t, self.head_dim), ops.attention_fwd_rope),
                 (ops.attention_fwd_long_rope_supported(t, self.head_dim), ops.attention_fwd_long_rope)),
                qkv_flat, rope)
            if out is not None:
                return out
        if on_device:
            library_fallback("attention (rope)", f"T={t} head_dim={self.head_dim} dtype={qkv_flat.dtype} "
                                                 f"grad={torch.is_grad_enabled()}")
        q, k, v = qkv_flat.reshape(b, t, 3, self.num_heads, self.head_dim).permute(2, 0, 3, 1, 4).unbind(0)
        q, k = apply_rope(q, rope), apply_rope(k, rope)
        if self.tap is not None:
            self.tap["out"] = self._importance(q, k, self.tap["has_cls"])       # of the rotated q / k
        out = F.scaled_dot_product_attention(q, k, v)
        return self.proj(out.transpose(1, 2).reshape(b, t, c))


class EvaMlp(nn.Module):
    """timm ``SwiGLU`` (EVA-02): ``fc2(norm(silu(fc1_g(x)) * fc1_x(x)))``, ``norm`` only with ``scale_mlp`` (sub-LN, the
    base model).  Frozen bf16 layer on the device: ONE GEMM over the packed [fc1_g; fc1_x] image with the gate in its
    epilogue (``basd_gemm_bf16_swiglu``; fc1_g is the gated half, w1 of that entry), the LayerNorm kernel, the fc2
    GEMM.  The packed operands are built once (``prepare`` or the first such forward) and kept: the teacher is frozen.
    Anything else is the torch composition -- on the device a counted library fallback."""

    def __init__(self, dim: int, hidden: int, scale_mlp: bool = False, eps: float = 1e-6):
        super().__init__()
        self.fc1_g = BasdLinear(dim, hidden)
        self.fc1_x = BasdLinear(dim, hidden)
        # None (not nn.Identity) without sub-LN: no module and no key the checkpoint does not have
        self.norm = MixedLayerNorm(hidden, eps=eps) if scale_mlp else None
        self.fc2 = BasdLinear(hidden, dim)
        self._packed = None            # (key of the four fc1 tensors, packed weight, packed bias)

    def prepare(self):
        """the packed [fc1_g; fc1_x] operands of the gated GEMM (rebuilt when the fc1 tensors have changed)"""
        ts = (self.fc1_g.weight, self.fc1_g.bias, self.fc1_x.weight, self.fc1_x.bias)
        key = tuple((t.data_ptr(), t._version) for t in ts)
        if self._packed is None or self._packed[0] != key:
            w12 = torch.cat([ts[0].detach(), ts[2].detach()])
            b12 = torch.cat([ts[1].detach(), ts[3].detach()])
            self._packed = (key,) + tuple(get_ops().swiglu_pack(w12, b12))
        return self._packed[1], self._packed[2]

    def _fused_ok(self, x) -> bool:
        ops = get_ops()
        hidden, dim = self.fc2.in_features, self.fc1_g.in_features
        return (_FUSED_EVA_DISPATCH and self.fc1_g.fused_inference_ok(x) and self.fc1_x.fused_inference_ok(x)
                and self.fc2.fused_inference_ok(x) and self.fc1_g.bias is not None and self.fc1_x.bias is not None
                and ops.gemm_swiglu_supported(hidden, dim)
                and (self.norm is None or (self.norm.elementwise_affine and ops.layernorm_supported(hidden))))

    def forward(self, x):
        if self._fused_ok(x):
            h = get_ops().gemm_bf16_swiglu(x, *self.prepare())
            return self.fc2(h if self.norm is None else self.norm(h))
        if get_ops().handles(x):
            library_fallback("SwiGLU MLP (EVA)", f"fc1 {self.fc1_g.in_features}->2x{self.fc2.in_features} "
                                                 f"dtype={x.dtype} grad={torch.is_grad_enabled()}")
        h = F.silu(self.fc1_g(x)) * self.fc1_x(x)
        return self.fc2(h if self.norm is None else self.norm(h))


class Eva(nn.Module):
    """timm ``Eva`` (the EVA-02 configuration) without its head: patch embedding, CLS token, absolute position
    embedding, pre-norm blocks with ``RopeAttention`` and ``EvaMlp`` (no LayerScale), final norm.  Parameter names
    are timm's."""

    def __init__(self, img_size=224, patch_size=14, in_chans=3, num_classes=0, embed_dim=768, depth=12, num_heads=12,
                 mlp_hidden=2048, scale_mlp=True, ref_grid=(16, 16), norm_eps=1e-6):
        super().__init__()
        if num_classes:
            raise ValueError("Eva: only the headless model (num_classes=0) is built: a teacher never uses the head")
        self.embed_dim = self.num_features = embed_dim
        self.num_classes = 0
        self.patch_embed = PatchEmbed(img_size, patch_size, in_chans, embed_dim)
        self.grid = (img_size // patch_size, img_size // patch_size)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.randn(1, self.patch_embed.num_patches + 1, embed_dim) * 0.02)
        attn_cls = functools.partial(RopeAttention, grid=self.grid, ref_grid=ref_grid)
        mlp_cls = functools.partial(EvaMlp, scale_mlp=scale_mlp, eps=norm_eps)
        self.blocks = nn.ModuleList([
            Block(embed_dim, num_heads, eps=norm_eps, attn_cls=attn_cls, mlp_cls=mlp_cls, mlp_hidden=mlp_hidden)
            for _ in range(depth)])
        self.norm = MixedLayerNorm(embed_dim, eps=norm_eps)
        for i, blk in enumerate(self.blocks):
            blk._next_norm.append(self.blocks[i + 1].norm1 if i + 1 < depth else self.norm)
        nn.init.normal_(self.cls_token, std=0.02)

    def materialize_qkv_bias(self) -> None:
        for blk in self.blocks:
            blk.attn.materialize_qkv_bias()

    def prepare_fused(self) -> None:
        """``load_teacher`` calls it on the frozen bf16 device model: the packed SwiGLU operands of every block, once"""
        for blk in self.blocks:
            blk.mlp.prepare()

    def _fused_embed_ok(self, x) -> bool:
        """frozen bf16 model on the device: CLS row and position embedding in one kernel (csrc/vit_embed.hip without
        its LayerNorm)"""
        return (_FUSED_EVA_DISPATCH and not torch.is_grad_enabled() and x.dtype == torch.bfloat16 and x.dim() == 3
                and get_ops().handles(x) and self.pos_embed.dtype == torch.bfloat16
                and self.cls_token.dtype == torch.bfloat16 and x.shape[1] + 1 == self.pos_embed.shape[1]
                and get_ops().vit_embed_supported(x.shape[-1]))

    def forward_features(self, x):
        x = self.patch_embed(x)
        if self._fused_embed_ok(x):
            x = get_ops().vit_embed(x, self.cls_token, self.pos_embed)
        else:
            x = torch.cat([self.cls_token.expand(x.shape[0], -1, -1).to(x.dtype), x], dim=1)
            x = x + self.pos_embed.to(x.dtype)
        for blk in self.blocks:
            x = blk(x)
        return self.norm(x)

    def forward(self, x):
        return self.forward_features(x)[:, 0]


# name -> (embed_dim, depth, heads, patch, MLP hidden width, sub-LN, reference grid, mean, std).  Written WITHOUT timm
# at hand, from memory of timm 1.0.x (eva.py model entrypoints and default_cfgs): hidden = dim * 4 * 2 / 3 (tiny: 512,
# small: 1024, base: 2048), only the base model has scale_mlp and carries q_proj / k_proj / v_proj instead of a fused
# qkv in its checkpoint, all are normalised with OpenAI CLIP's statistics and rotate against a 16 x 16 reference grid --
# check them against the installed timm before loading real weights.
EVA_PRESETS = {
    "eva02_tiny_patch14_224": (192, 12, 3, 14, 512, False, (16, 16), CLIP_MEAN, CLIP_STD),
    "eva02_small_patch14_224": (384, 12, 6, 14, 1024, False, (16, 16), CLIP_MEAN, CLIP_STD),
    "eva02_base_patch14_224": (768, 12, 12, 14, 2048, True, (16, 16), CLIP_MEAN, CLIP_STD),
}

# keys of a timm checkpoint that have no counterpart here: the table is rebuilt from the grid, the head is not built,
# the k bias is a zero buffer
_DROPPED = ("rope.", "fc_norm.", "head.", "attn.k_bias")


def create_eva(name: str, *, img_size: int, patch_size: int | None = None, **overrides) -> Eva:
    """timm.create_model stand-in for the presets above (``overrides``: embed_dim, depth, num_heads, mlp_hidden,
    scale_mlp)"""
    if name not in EVA_PRESETS:
        raise ValueError(f"unknown EVA preset {name!r}; known: {sorted(EVA_PRESETS)}")
    dim, depth, heads, patch, hidden, scale_mlp, ref_grid, _, _ = EVA_PRESETS[name]
    kw = dict(embed_dim=dim, depth=depth, num_heads=heads, mlp_hidden=hidden, scale_mlp=scale_mlp)
    kw.update({k: v for k, v in overrides.items() if k in kw})
    return Eva(img_size=img_size, patch_size=patch_size or patch, num_classes=0, ref_grid=ref_grid, **kw)


def eva_state_dict(model: Eva, state: dict) -> dict:
    """A timm Eva state dict -> this model's names: ``attn.q_proj`` / ``k_proj`` / ``v_proj`` weights (the base
    checkpoint) are concatenated into ``attn.qkv.weight`` and the ``q_proj`` / ``v_proj`` biases become ``q_bias`` /
    ``v_bias``; ``rope.*`` buffers, the zero ``k_bias`` buffer, ``head.*`` and ``fc_norm.*`` are dropped.  A
    ``pos_embed`` with another row count than the model's is an error (position embeddings are not resampled).  Load
    the result with ``load_eva_state_dict``, which also materialises the qkv bias."""
    out, split = {}, {}
    for key, value in state.items():
        if any(key.startswith(d) or f".{d}" in key for d in _DROPPED):
            continue
        if key == "pos_embed" and value.shape[-2] != model.pos_embed.shape[1]:
            raise ValueError(f"pos_embed: {value.shape[-2]} rows, but the model (img_size {model.patch_embed.img_size}, "
                             f"patch {model.patch_embed.patch_size}: a {model.grid[0]} x {model.grid[1]} grid + CLS) has "
                             f"{model.pos_embed.shape[1]}; position embeddings are not resampled")
        for part in ("q_proj", "k_proj", "v_proj"):
            if f".attn.{part}." in key:
                prefix, leaf = key.split(f"{part}.")
                if leaf == "weight":
                    split.setdefault(prefix, {})[part] = value
                else:                                # q_proj.bias / v_proj.bias (k_proj has none)
                    out[f"{prefix}{part[0]}_bias"] = value
                break
        else:
            out[key] = value
    for prefix, parts in split.items():
        if sorted(parts) != ["k_proj", "q_proj", "v_proj"]:
            raise ValueError(f"{prefix}: q_proj / k_proj / v_proj weights go together, found {sorted(parts)}")
        out[f"{prefix}qkv.weight"] = torch.cat([parts["q_proj"], parts["k_proj"], parts["v_proj"]])
    return out


def load_eva_state_dict(model: Eva, state: dict) -> list:
    """``eva_state_dict`` + ``load_state_dict`` + ``materialize_qkv_bias``; -> missing keys.  A key without a
    counterpart is an error."""
    missing, unexpected = model.load_state_dict(eva_state_dict(model, state), strict=False)
    if unexpected:
        raise ValueError(f"load_eva_state_dict: keys without a counterpart in Eva: {sorted(unexpected)}")
    model.materialize_qkv_bias()
    return list(missing)
