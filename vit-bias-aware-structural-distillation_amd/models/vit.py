"""Plain ViT / DeiT / DINOv2-style vision transformer for the BASD train step.

The reference takes its blocks from ``timm==1.0.24`` (``src/train.py:51``,
``src/models/teacher.py:118``), which is not part of the reference repository
and not installed here: this is an own implementation of the public ViT
definition, constrained by what the reference itself assumes of it --
``blocks`` container, ``attn.qkv`` single Linear with ``reshape(B,N,3,nh,hd)``
split order, ``attn.num_heads``, scale ``hd**-0.5``, CLS token at index 0
(teacher.py:33-37,46-50,156-157; trainer.py:29).  Parameter names follow timm
(``cls_token``, ``pos_embed``, ``patch_embed.proj``, ``blocks.i.norm1``,
``attn.qkv``, ``attn.proj``, ``ls1.gamma``, ``mlp.fc1`` ...) so that
``model_state_dict`` files are interchangeable (trainer.py:105-111, eval.py:29-30).

On the device the linear layers, attention (forward and backward, with the
per-block CLS-row importance tap computed from the block's own q/k: no duplicate
QKV GEMM, no [B,H,T,T] map) and LayerNorm run on the library's own gfx950 kernels
(csrc/gemm_bf16.hip, attention*.hip, layernorm.hip) under bf16 autocast; a layer
that has to take a PyTorch-ROCm library kernel instead is counted in
``losses._ops.FALLBACKS`` (an error in strict mode).  Parity of the ViT
arithmetic itself is UNPINNED by the reference (it has no tests and timm is
absent) -- see DESIGN.md.

The image-text teachers (timm's CLIP and SigLIP ViTs) are the same model with three switches: ``pre_norm`` (a LayerNorm
on the assembled tokens in front of block 0, patch embedding without bias), the MLP activation ``act`` ("gelu",
"quick_gelu", "gelu_tanh") and ``norm_eps``.  They exist for FROZEN teachers: the activation rides in the fc1 GEMM's
epilogue (``basd_gemm_bf16_act``) and the token assembly + ``norm_pre`` is one kernel (``basd_vit_embed_bf16``).  A
TRAINED block with a non-erf activation has no backward epilogue: it takes the unfused path and is counted as a library
fallback -- students with these activations or with ``pre_norm`` are out of scope.

The DINOv2 family adds two more: ``reg_tokens`` (R learned rows placed behind the CLS row AFTER the position embedding
has been added, so ``pos_embed`` keeps its 1 + N rows and every block runs on 1 + R + N tokens) and ``mlp="swiglu"``
(ViT-g/14: ``w3(silu(x1) * x2)``, ``x1, x2 = w12(x).chunk(2, -1)``, hub parameter names).  Again for FROZEN teachers:
the gate rides in the w12 GEMM's epilogue (``basd_gemm_bf16_swiglu`` on weights packed once) and the token assembly
with registers is one kernel (``basd_vit_embed_reg_bf16``); a trained SwiGLU runs unfused and is a counted fallback.
The reference strips only the CLS row, so the registers stay among the teacher tokens and in the importance vector.
"""
from __future__ import annotations

import math
import os
from typing import NamedTuple

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.utils.checkpoint import checkpoint

from ..losses._ops import get_ops, library_fallback
from .linear import BasdLinear, _LinearFn, fused_mlp, fused_mlp_ok


class DropPath(nn.Module):
    def __init__(self, p: float = 0.0):
        super().__init__()
        self.p = float(p)

    def forward(self, x):
        if self.p == 0.0 or not self.training:
            return x
        return x * self.scaled_mask(x)

    def scaled_mask(self, x):
        """per-sample keep mask already divided by the keep probability (timm drop_path, scale_by_keep)"""
        keep = 1.0 - self.p
        mask = x.new_empty((x.shape[0],) + (1,) * (x.dim() - 1)).bernoulli_(keep)
        return mask / keep

    def add_to(self, residual, x, mask=None):
        """residual + drop_path(x) in one elementwise kernel (addcmul) instead of mul, div and add;
        ``mask``: a pre-drawn scaled keep mask (the model draws all of a forward's masks in one launch)"""
        if self.p == 0.0 or not self.training:
            return residual + x
        return torch.addcmul(residual, x, self.scaled_mask(x) if mask is None else mask)


class _LayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        ops = get_ops()
        y, mean, rstd = ops.layernorm_fwd(x, weight.detach().float(), bias.detach().float(), eps)
        ctx.save_for_backward(x, mean, rstd)
        ctx.weight, ctx.bias = weight, bias
        return y

    @staticmethod
    def backward(ctx, g):
        ops = get_ops()
        x, mean, rstd = ctx.saved_tensors
        weight, bias = ctx.weight, ctx.bias
        g = g.to(torch.bfloat16)
        gw = gb = None
        if weight.requires_grad:
            sink_w, sink_b = getattr(weight, "_basd_grad", None), getattr(bias, "_basd_grad", None)
            if sink_w is not None and sink_b is not None:      # straight into the flat gradient buffer
                dx = ops.layernorm_bwd(g, x, weight.detach().float(), mean, rstd, sink_w, sink_b)
                for p in (weight, bias):
                    ready = getattr(p, "_basd_ready", None)
                    if ready is not None:
                        ready()
            else:
                gw = torch.zeros_like(weight, dtype=torch.float32)
                gb = torch.zeros_like(bias, dtype=torch.float32)
                dx = ops.layernorm_bwd(g, x, weight.detach().float(), mean, rstd, gw, gb)
                gw, gb = gw.to(weight.dtype), gb.to(bias.dtype)
        else:
            dx = ops.layernorm_bwd(g, x, weight.detach().float(), mean, rstd, None, None)
        return dx, gw, gb, None


class _AddLayerNormFn(torch.autograd.Function):
    """One residual step of a TRAINED pre-norm block: s = residual + drop_path(branch), y = LayerNorm(s), both returned.
    Forward: one kernel (``basd_add_layernorm_fwd_bf16`` with the per-sample stochastic-depth scale); backward: one
    kernel that adds the gradient arriving through the residual connection to the LayerNorm backward and also emits the
    (scaled) gradient of the branch -- instead of addcmul + LayerNorm forward, and LayerNorm backward + add (+ mul)."""

    @staticmethod
    def forward(ctx, branch, residual, scale, weight, bias, eps):
        s, y, mean, rstd = get_ops().add_layernorm_fwd(branch, residual, weight.detach().float(), bias.detach().float(),
                                                       eps, row_scale=scale, want_stats=True)
        ctx.save_for_backward(s, mean, rstd)
        ctx.scale, ctx.weight, ctx.bias = scale, weight, bias
        return s, y

    @staticmethod
    def backward(ctx, g_s, g_y):
        ops = get_ops()
        s, mean, rstd = ctx.saved_tensors
        weight, bias, scale = ctx.weight, ctx.bias, ctx.scale
        dy = torch.zeros_like(s) if g_y is None else g_y.to(torch.bfloat16)
        gw = gb = None
        sink_w = sink_b = None
        if weight.requires_grad:
            sink_w, sink_b = getattr(weight, "_basd_grad", None), getattr(bias, "_basd_grad", None)
            if sink_w is None or sink_b is None:
                gw = torch.zeros_like(weight, dtype=torch.float32)
                gb = torch.zeros_like(bias, dtype=torch.float32)
                sink_w, sink_b = gw, gb
        out = ops.layernorm_bwd(dy, s, weight.detach().float(), mean, rstd, sink_w, sink_b, dres=g_s, row_scale=scale,
                                want_branch=scale is not None)
        d_res, d_branch = out if scale is not None else (out, out)
        if weight.requires_grad and gw is None:
            for p in (weight, bias):
                ready = getattr(p, "_basd_ready", None)
                if ready is not None:
                    ready()
        if gw is not None:
            gw, gb = gw.to(weight.dtype), gb.to(bias.dtype)
        return d_branch, d_res, None, gw, gb, None


class MixedLayerNorm(nn.LayerNorm):
    """nn.LayerNorm (same parameters) running on the fused HIP kernel for bf16 activations: bf16 in,
    bf16 out, fp32 gamma / beta / statistics.  Equal to torch's autocast behaviour (fp32 layer_norm)
    followed by the bf16 rounding the next Linear applies, without the up/down-cast copies and with a
    one-kernel backward.  Other inputs (fp32 activations, CPU) take the stock path."""

    def forward(self, x):
        pre = getattr(x, "_basd_prenorm", None)
        if pre is not None and pre[0] is self:
            return pre[1]               # already produced by the fused residual-add + norm of the previous step
        if (x.dtype == torch.bfloat16 and get_ops().handles(x) and self.elementwise_affine
                and get_ops().layernorm_supported(x.shape[-1])):
            return _LayerNormFn.apply(x, self.weight, self.bias, self.eps)
        return super().forward(x)

    def fused_add(self, x, residual):
        """(x + residual, LayerNorm(x + residual)) in one kernel; inference only."""
        return get_ops().add_layernorm_fwd(x, residual, self.weight.detach().float(), self.bias.detach().float(), self.eps)


class LayerScale(nn.Module):
    def __init__(self, dim: int, init_values: float):
        super().__init__()
        self.gamma = nn.Parameter(init_values * torch.ones(dim))

    def forward(self, x):
        return x * self.gamma


class _PackedFlashAttention(torch.autograd.Function):
    """softmax(QK^T / sqrt(hd)) V on the packed projection [B, T, 3 * H * hd] with a packed gradient.

    Through plain autograd the three gradients of the library's flash-attention backward are stacked
    (unbind backward) and then copied once more into the [B, T, 3, H, hd] order the qkv Linear wants:
    two extra passes over the projection gradient per block.  Here the same library kernels are called
    directly (aten::_scaled_dot_product_flash_attention[_backward]) and their three outputs, which are
    [B, T, H, hd]-contiguous, are interleaved once."""

    @staticmethod
    def forward(ctx, qkv_flat, heads, head_dim):
        b, t, _ = qkv_flat.shape
        qkv = qkv_flat.view(b, t, 3, heads, head_dim)
        q, k, v = (qkv[:, :, i].transpose(1, 2) for i in range(3))              # [B, H, T, hd] views
        res = torch.ops.aten._scaled_dot_product_flash_attention(q, k, v, 0.0, False, False)
        out, lse, cum_q, cum_k, max_q, max_k, seed, offset = res[:8]
        ctx.save_for_backward(qkv_flat, out, lse, cum_q, cum_k, seed, offset)
        ctx.dims = (heads, head_dim, max_q, max_k)
        return out

    @staticmethod
    def backward(ctx, g):
        qkv_flat, out, lse, cum_q, cum_k, seed, offset = ctx.saved_tensors
        heads, head_dim, max_q, max_k = ctx.dims
        b, t, _ = qkv_flat.shape
        qkv = qkv_flat.view(b, t, 3, heads, head_dim)
        q, k, v = (qkv[:, :, i].transpose(1, 2) for i in range(3))
        dq, dk, dv = torch.ops.aten._scaled_dot_product_flash_attention_backward(
            g, q, k, v, out, lse, cum_q, cum_k, max_q, max_k, 0.0, False, seed, offset)
        dqkv = torch.stack((dq.transpose(1, 2), dk.transpose(1, 2), dv.transpose(1, 2)), dim=2)   # [B, T, 3, H, hd]
        return dqkv.view(b, t, 3 * heads * head_dim), None, None


class _FusedAttention(torch.autograd.Function):
    """softmax(Q K^T / sqrt(hd)) V of a TRAINED block on the hand-written kernels: forward = the fused attention
    kernel the frozen teacher uses, with the log-sum-exp written out; backward = ``basd_attention_bwd_bf16`` (P
    recomputed from Q, K and the LSE, gradient delivered already packed as [B, T, 3 * H * hd])."""

    @staticmethod
    def forward(ctx, qkv_flat, heads, head_dim, scale):
        out, _, lse = get_ops().attention_fwd(qkv_flat, heads, head_dim, scale, want_lse=True)
        ctx.save_for_backward(qkv_flat, out, lse)
        ctx.dims = (heads, head_dim, scale)
        return out

    @staticmethod
    def backward(ctx, g):
        qkv_flat, out, lse = ctx.saved_tensors
        heads, head_dim, scale = ctx.dims
        return get_ops().attention_bwd(qkv_flat, out, g, lse, heads, head_dim, scale), None, None, None


_FUSED_TEACHER_ATTENTION = os.environ.get("BASD_FUSED_ATTN", "1") == "1"     # 0: library SDPA + separate tap (A/B runs)
# 0: QuickGELU / tanh-GELU as a torch op behind a bias-only GEMM, torch token assembly + norm_pre (A/B runs:
# scripts/time_clip_teacher.py flips it inside one process)
_FUSED_CLIP_DISPATCH = os.environ.get("BASD_FUSED_CLIP", "1") == "1"
# 0: SwiGLU as a bias-only w12 GEMM + a torch gate, register tokens through the torch assembly (A/B runs:
# scripts/time_dinov2_teacher.py flips it inside one process)
_FUSED_DINOV2_DISPATCH = os.environ.get("BASD_FUSED_DINOV2", "1") == "1"
_packed_attention_ok = True      # cleared on the first failure of the direct library call (other torch builds)


class Attention(nn.Module):
    def __init__(self, dim: int, num_heads: int, qkv_bias: bool = True):
        super().__init__()
        self.num_heads = num_heads
        self.head_dim = dim // num_heads
        self.scale = self.head_dim ** -0.5
        self.qkv = BasdLinear(dim, dim * 3, bias=qkv_bias)
        self.proj = BasdLinear(dim, dim)
        self.tap: dict | None = None       # set by the teacher tap: {"has_cls": bool, "out": tensor}

    def forward(self, x):
        b, t, c = x.shape
        qkv_flat = self.qkv(x)
        if (_FUSED_TEACHER_ATTENTION and not torch.is_grad_enabled() and qkv_flat.dtype == torch.bfloat16
                and get_ops().handles(qkv_flat) and get_ops().attention_fwd_supported(t, self.head_dim)):
            # frozen block: fused attention straight from the packed projection, the tap as a by-product
            # (csrc/attention.hip)
            # the tap: CLS row of the head-averaged map, or (teachers without a CLS token) that map averaged over the
            # queries -- both by-products of the same kernel
            has_cls = self.tap is not None and bool(self.tap["has_cls"])
            want = self.tap is not None and (t >= 2 or not has_cls)
            out_flat, imp = get_ops().attention_fwd(qkv_flat, self.num_heads, self.head_dim, self.scale, want,
                                                    query_mean=want and not has_cls)
            if self.tap is not None:
                if want:
                    self.tap["out"] = imp
                else:
                    q_, k_, _ = qkv_flat.reshape(b, t, 3, self.num_heads, self.head_dim).permute(2, 0, 3, 1, 4).unbind(0)
                    self.tap["out"] = self._importance(q_, k_, self.tap["has_cls"])
            return self.proj(out_flat)
        if (torch.is_grad_enabled() and qkv_flat.requires_grad and qkv_flat.dtype == torch.bfloat16 and self.tap is None
                and get_ops().handles(qkv_flat) and get_ops().attention_fwd_supported(t, self.head_dim)
                and get_ops().attention_bwd_supported(t, self.head_dim)):
            # trained block (the student): hand-written forward (+ LSE) and backward kernels
            return self.proj(_FusedAttention.apply(qkv_flat.contiguous(), self.num_heads, self.head_dim, self.scale))
        qkv = qkv_flat.reshape(b, t, 3, self.num_heads, self.head_dim).permute(2, 0, 3, 1, 4)
        q, k, v = qkv.unbind(0)
        on_device = get_ops().handles(qkv_flat)
        if self.tap is not None:
            ops = get_ops() if on_device else None
            if (ops is not None and self.tap["has_cls"] and qkv_flat.dtype == torch.bfloat16
                    and ops.cls_importance_supported(t, self.head_dim)):
                # fused tap: streams K once from the packed projection (csrc/attn_tap.hip)
                self.tap["out"] = ops.cls_importance(qkv_flat, self.num_heads, self.head_dim, self.scale)
            else:
                if on_device and self.tap["has_cls"]:
                    library_fallback("attention tap", f"T={t} head_dim={self.head_dim} dtype={qkv_flat.dtype}")
                self.tap["out"] = self._importance(q, k, self.tap["has_cls"])
        if on_device:
            library_fallback("attention", f"T={t} head_dim={self.head_dim} dtype={qkv_flat.dtype} "
                                          f"grad={torch.is_grad_enabled() and qkv_flat.requires_grad}")
        global _packed_attention_ok
        out = None
        if (_packed_attention_ok and qkv_flat.is_cuda and qkv_flat.dtype in (torch.bfloat16, torch.float16)
                and torch.is_grad_enabled() and qkv_flat.requires_grad and qkv_flat.is_contiguous()):
            try:
                out = _PackedFlashAttention.apply(qkv_flat, self.num_heads, self.head_dim)
            except (RuntimeError, AttributeError, TypeError):
                _packed_attention_ok = False
        if out is None:
            out = F.scaled_dot_product_attention(q, k, v)
        return self.proj(out.transpose(1, 2).reshape(b, t, c))

    def _importance(self, q, k, has_cls: bool):
        """Head-averaged token importance [B, N]: the only part of softmax(QK^T/sqrt(hd)) the
        loss reads (src/losses/relational.py:22-27; teacher.py:33-37 builds the full map)."""
        if has_cls:
            # q_cls k^T in the activation dtype (bf16 in, fp32 accumulate) like the reference's
            # autocast matmul (teacher.py:36), softmax in fp32; no fp32 copy of K
            logits = (q[:, :, :1] @ k.transpose(-2, -1)).float() * self.scale               # [B,H,1,T]
            return logits.softmax(dim=-1)[:, :, 0, 1:].mean(dim=1)
        attn = ((q.float() @ k.float().transpose(-2, -1)) * self.scale).softmax(dim=-1)
        return attn.mean(dim=(1, 2))

    def _fused_frozen(self, entries, qkv_flat, *pos_args):
        """Frozen block with a position scheme (``RelPosAttention``, ``RopeAttention``): ``entries`` are the eligible
        ``(supported, entry)`` pairs in order, the short kernel first.  Runs the first supported entry on
        ``(qkv_flat, *pos_args, heads, head_dim, scale, want_tap)``, sets the tap (a by-product of the kernel) and
        returns the projected output; None on a miss (the caller counts the library fallback)."""
        for supported, entry in entries:
            if supported:
                out_flat, imp = entry(qkv_flat, *pos_args, self.num_heads, self.head_dim, self.scale,
                                      self.tap is not None)
                if self.tap is not None:
                    self.tap["out"] = imp
                return self.proj(out_flat)
        return None


class QVBiasAttention(Attention):
    """The attention of timm's Beit / Eva: ``qkv`` without a bias parameter, ``q_bias`` / ``v_bias`` separate (the k bias
    is zero), and one fp32 position tensor -- the parameter or buffer named ``_fp32_name`` -- that keeps its fp32 values
    whatever the model is cast to: the kernels read fp32 tables, which gain nothing from (or do not survive) a 16-bit
    copy."""
    _fp32_name: str                                  # set by every subclass

    def __init__(self, dim: int, num_heads: int):
        if not getattr(type(self), "_fp32_name", ""):
            raise TypeError("QVBiasAttention is a base: a subclass names its fp32 tensor in _fp32_name")
        super().__init__(dim, num_heads, qkv_bias=False)
        self.q_bias = nn.Parameter(torch.zeros(dim))
        self.v_bias = nn.Parameter(torch.zeros(dim))

    def _apply(self, fn, recurse=True):
        """``.to(bf16)`` / ``.half()`` move the tensor with the module but leave its values in fp32"""
        keep = getattr(self, self._fp32_name).data
        super()._apply(fn, recurse)
        moved = getattr(self, self._fp32_name)
        if moved.dtype in (torch.bfloat16, torch.float16):
            moved.data = keep.to(moved.device)
        return self

    def _qkv_bias(self) -> torch.Tensor:
        return torch.cat([self.q_bias, torch.zeros_like(self.q_bias), self.v_bias])

    @torch.no_grad()
    def materialize_qkv_bias(self) -> None:
        """frozen teacher: ``cat(q_bias, 0, v_bias)`` becomes the bias of the ``qkv`` layer once, so that the projection
        stays the one fused GEMM call (bias in the epilogue) of every other ViT"""
        self.qkv.bias = nn.Parameter(self._qkv_bias().to(self.qkv.weight.dtype), requires_grad=False)

    def _qkv(self, x):
        """the packed projection, with the bias added here while it is not materialised (a model under training, a CPU
        check)"""
        qkv_flat = self.qkv(x)
        return qkv_flat if self.qkv.bias is not None else qkv_flat + self._qkv_bias().to(qkv_flat.dtype)


class QuickGELU(nn.Module):
    """x * sigmoid(1.702 x): the activation of the OpenAI-weight CLIP towers (timm ``quick_gelu``)"""

    def forward(self, x):
        return x * torch.sigmoid(1.702 * x)


MLP_ACTS = ("gelu", "quick_gelu", "gelu_tanh")


class Mlp(nn.Module):
    """timm Mlp.  ``act``: "gelu" (exact erf), "quick_gelu" or "gelu_tanh".  Only the erf form has a backward epilogue:
    a TRAINED Mlp with another activation runs unfused (a counted library fallback, an error in strict mode)."""

    def __init__(self, dim: int, hidden: int, act: str = "gelu"):
        super().__init__()
        if act not in MLP_ACTS:
            raise ValueError(f"Mlp: unknown activation {act!r}; known: {MLP_ACTS}")
        self.act_name = act
        self.fc1 = BasdLinear(dim, hidden)
        self.act = nn.GELU() if act == "gelu" else nn.GELU(approximate="tanh") if act == "gelu_tanh" else QuickGELU()
        self.fc2 = BasdLinear(hidden, dim)

    def forward(self, x):
        if self.fc1.fused_inference_ok(x):        # frozen block: the activation in the epilogue of the fc1 GEMM
            if self.act_name == "gelu":
                return self.fc2(get_ops().gemm_bf16(x, self.fc1.weight, self.fc1.bias, gelu=True))
            if _FUSED_CLIP_DISPATCH:
                return self.fc2(get_ops().gemm_bf16(x, self.fc1.weight, self.fc1.bias, act=self.act_name))
            return self.fc2(self.act(self.fc1(x)))
        # trained block: GELU forward / backward inside the GEMM epilogues (exact erf only)
        if self.act_name == "gelu" and fused_mlp_ok(x, self.fc1, self.fc2):
            return fused_mlp(x, self.fc1, self.fc2)
        if get_ops().handles(x):
            library_fallback("MLP GELU", f"fc1 {self.fc1.in_features}->{self.fc1.out_features} dtype={x.dtype}")
        return self.fc2(self.act(self.fc1(x)))


MLP_KINDS = ("mlp", "swiglu")


class SwiGLU(nn.Module):
    """The MLP of DINOv2's ViT-g/14 (hub ``SwiGLUFFNFused``; parameter names ``w12`` / ``w3`` as in the hub checkpoint):
    ``w3(silu(x1) * x2)`` with ``x1, x2 = w12(x).chunk(2, -1)``.  Frozen bf16 layer on the device: ONE GEMM over the
    packed w12 with the gate in its epilogue (``basd_gemm_bf16_swiglu``), then the w3 GEMM; the packed operands are
    built on the first such forward (after the bf16 cast) and kept: the teacher is frozen.  Anything else is the torch
    composition -- on the device a counted library fallback (a trained SwiGLU has no backward epilogue)."""

    def __init__(self, dim: int, hidden: int):
        super().__init__()
        self.w12 = BasdLinear(dim, 2 * hidden)
        self.w3 = BasdLinear(hidden, dim)
        self._packed = None            # (key of the w12 tensors, packed weight, packed bias)

    def _packed_operands(self):
        w, b = self.w12.weight, self.w12.bias
        key = (w.data_ptr(), w._version, None if b is None else (b.data_ptr(), b._version))
        if self._packed is None or self._packed[0] != key:
            wp, bp = get_ops().swiglu_pack(w.detach(), None if b is None else b.detach())
            self._packed = (key, wp, bp)
        return self._packed[1], self._packed[2]

    def forward(self, x):
        hidden = self.w3.in_features
        if self.w12.fused_inference_ok(x) and self.w3.fused_inference_ok(x):
            if not _FUSED_DINOV2_DISPATCH:                 # A/B: bias-only GEMM, gate as torch ops
                x1, x2 = self.w12(x).chunk(2, dim=-1)
                return self.w3(F.silu(x1) * x2)
            if get_ops().gemm_swiglu_supported(hidden, self.w12.in_features):
                wp, bp = self._packed_operands()
                return self.w3(get_ops().gemm_bf16_swiglu(x, wp, bp))
        if get_ops().handles(x):
            library_fallback("SwiGLU MLP", f"w12 {self.w12.in_features}->2x{hidden} dtype={x.dtype} "
                                           f"grad={torch.is_grad_enabled()}")
        x1, x2 = self.w12(x).chunk(2, dim=-1)
        return self.w3(F.silu(x1) * x2)


class Block(nn.Module):
    def __init__(self, dim, num_heads, mlp_ratio=4.0, drop_path=0.0, init_values=None, eps=1e-6, act="gelu",
                 attn_cls=None, mlp="mlp", mlp_hidden=None, mlp_cls=None):
        super().__init__()
        self.norm1 = MixedLayerNorm(dim, eps=eps)
        # attn_cls(dim, num_heads): the attention of another model family (models/beit.py); default: Attention
        self.attn = (attn_cls or Attention)(dim, num_heads)
        self.ls1 = LayerScale(dim, init_values) if init_values else nn.Identity()
        self.drop_path1 = DropPath(drop_path)
        self.norm2 = MixedLayerNorm(dim, eps=eps)
        if mlp not in MLP_KINDS:
            raise ValueError(f"Block: unknown MLP {mlp!r}; known: {MLP_KINDS}")
        hidden = int(mlp_hidden) if mlp_hidden else int(dim * mlp_ratio)
        # mlp_cls(dim, hidden): the MLP of another model family (models/eva.py); default: SwiGLU / Mlp by name
        self.mlp = mlp_cls(dim, hidden) if mlp_cls else SwiGLU(dim, hidden) if mlp == "swiglu" else Mlp(dim, hidden, act)
        self.ls2 = LayerScale(dim, init_values) if init_values else nn.Identity()
        self.drop_path2 = DropPath(drop_path)

        self._next_norm = []            # [norm that consumes this block's output]; set by the model, not a submodule
        self.fuse_training = True       # cleared under activation checkpointing (tensor attributes do not survive it)
        self._f32x3 = None              # (weight images, final norm) while the model runs its fp32 "high" forward

    def _fused_inference(self, x) -> bool:
        """frozen pre-norm block on bf16 activations: the residual adds fuse into the following norms"""
        return (not torch.is_grad_enabled() and x.dtype == torch.bfloat16 and get_ops().handles(x)
                and isinstance(self.ls1, nn.Identity) and isinstance(self.ls2, nn.Identity)
                and (not self.training or (self.drop_path1.p == 0.0 and self.drop_path2.p == 0.0))
                and self.norm2.elementwise_affine and get_ops().layernorm_supported(x.shape[-1]))

    def _fused_training(self, x) -> bool:
        """trained pre-norm block on bf16 activations: residual add (+ stochastic depth) fused with the next norm"""
        return (torch.is_grad_enabled() and self.training and x.dtype == torch.bfloat16 and x.requires_grad
                and get_ops().handles(x) and isinstance(self.ls1, nn.Identity) and isinstance(self.ls2, nn.Identity)
                and self.norm2.elementwise_affine and self.fuse_training and get_ops().layernorm_supported(x.shape[-1]))

    def _f32x3_supported(self, t: int) -> bool:
        """every layer of this block has a kernel of the fp32 split-bf16 evaluation forward (T tokens)"""
        ops = get_ops()
        a, d = self.attn, self.attn.qkv.in_features
        lins = (a.qkv, a.proj, self.mlp.fc1, self.mlp.fc2)
        return (type(self.mlp) is Mlp and isinstance(self.mlp.act, nn.GELU) and self.mlp.act.approximate == "none"
                and a.tap is None and (ops.attention_fwd_f32x3_supported(t, a.head_dim)
                                       or ops.attention_fwd_f32x3_long_supported(t, a.head_dim))
                and ops.f32x3_layernorm_supported(d)
                and all(l.bias is not None and l.weight.dtype == torch.float32 and l.bias.dtype == torch.float32
                        and ops.f32x3_gemm_supported(l.out_features, l.in_features) for l in lins)
                and all(isinstance(m, (nn.Identity, LayerScale)) for m in (self.ls1, self.ls2))
                and self.norm1.elementwise_affine and self.norm2.elementwise_affine
                and (not self.training or (self.drop_path1.p == 0.0 and self.drop_path2.p == 0.0)))

    def _forward_f32x3(self, x, images, final_norm):
        """fp32 evaluation forward on split-bf16 products (csrc/eval_f32x3.hip): LayerNorm -> qkv -> attention -> proj ->
        residual add + LayerNorm -> fc1 + GELU -> fc2 -> residual add, with the add fused into the NEXT norm as in
        _fused_inference.  Between the kernels the GEMM inputs travel as split images; the block output is an ordinary
        fp32 [B, T, D] tensor."""
        ops = get_ops()
        b, t, d = x.shape
        a, n1, n2 = self.attn, self.norm1, self.norm2
        w_qkv, w_proj, w_fc1, w_fc2 = images
        pre = getattr(x, "_basd_prenorm_img", None)
        if pre is not None and pre[0] is n1:
            z = pre[1]
        else:
            (z,) = ops.add_layernorm_f32(x, n1.weight.detach().float(), n1.bias.detach().float(), n1.eps)
        qkv = ops.gemm_f32x3(z, w_qkv, a.qkv.bias.detach())
        o = ops.attention_fwd_f32x3(qkv.view(b, t, -1), a.num_heads, a.head_dim, a.scale)
        y = ops.gemm_f32x3(o, w_proj, a.proj.bias.detach()).view(b, t, d)
        g1 = self.ls1.gamma.detach() if isinstance(self.ls1, LayerScale) else None
        g2 = self.ls2.gamma.detach() if isinstance(self.ls2, LayerScale) else None
        x, z = ops.add_layernorm_f32(y, n2.weight.detach().float(), n2.bias.detach().float(), n2.eps, residual=x,
                                     xscale=g1, want_s=True)
        h = ops.gemm_f32x3(z, w_fc1, self.mlp.fc1.bias.detach(), gelu=True, split_out=True)
        m = ops.gemm_f32x3(h, w_fc2, self.mlp.fc2.bias.detach()).view(b, t, d)
        nxt = self._next_norm[0] if self._next_norm else None
        if nxt is None or not nxt.elementwise_affine or not ops.f32x3_layernorm_supported(d):
            return x + (m * g2 if g2 is not None else m)
        final = nxt is final_norm
        out, zn = ops.add_layernorm_f32(m, nxt.weight.detach().float(), nxt.bias.detach().float(), nxt.eps, residual=x,
                                        xscale=g2, want_s=True, want_y=final, want_img=not final)
        if final:
            out._basd_prenorm = (nxt, zn)            # the model's final norm returns it (fp32 [B, T, D])
        else:
            out._basd_prenorm_img = (nxt, zn)        # the next block's norm1 as the image its qkv GEMM reads
        return out

    def forward(self, x, dp_masks=None):
        if self._f32x3 is not None and x.dtype == torch.float32 and not torch.is_grad_enabled():
            return self._forward_f32x3(x, *self._f32x3)
        if self._fused_training(x):
            # (bf16 mask, bf16 mask, fp32 per-sample scale, fp32 per-sample scale): the model draws all of them at once
            m1, m2, sc1, sc2 = dp_masks if dp_masks is not None else (None, None, None, None)
            a = self.attn(self.norm1(x))
            x, z = _AddLayerNormFn.apply(a, x, sc1, self.norm2.weight, self.norm2.bias, self.norm2.eps)
            m = self.mlp(z)
            nxt = self._next_norm[0] if self._next_norm else None
            if nxt is None or not nxt.elementwise_affine:
                return self.drop_path2.add_to(x, m, m2)
            out, zn = _AddLayerNormFn.apply(m, x, sc2, nxt.weight, nxt.bias, nxt.eps)
            out._basd_prenorm = (nxt, zn)
            return out
        if self._fused_inference(x):
            a = self.attn(self.norm1(x))
            x, z = self.norm2.fused_add(x, a)
            m = self.mlp(z)
            nxt = self._next_norm[0] if self._next_norm else None
            if nxt is None or not nxt.elementwise_affine:
                return x + m
            out, zn = nxt.fused_add(x, m)
            out._basd_prenorm = (nxt, zn)
            return out
        m1, m2 = dp_masks[:2] if dp_masks is not None else (None, None)
        x = self.drop_path1.add_to(x, self.ls1(self.attn(self.norm1(x))), m1)
        return self.drop_path2.add_to(x, self.ls2(self.mlp(self.norm2(x))), m2)


class PatchEmbed(nn.Module):
    def __init__(self, img_size, patch_size, in_chans, embed_dim, bias=True):
        super().__init__()
        self.img_size, self.patch_size = img_size, patch_size
        self.num_patches = (img_size // patch_size) ** 2
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=patch_size, stride=patch_size, bias=bias)

    def forward(self, x):
        # non-overlapping patches: the stride-p convolution IS a GEMM on unfolded patches
        # ([B*N, 3*p*p] x [3*p*p, D]).  Going through F.conv2d lands on MIOpen's untuned
        # naive bf16 convolution here (24 ms fwd + 31 ms wrw per call at B=256).
        b, c, h, w = x.shape
        p = self.patch_size
        d, k = self.proj.weight.shape[0], c * p * p
        unfolded = x.reshape(b, c, h // p, p, w // p, p).permute(0, 2, 4, 1, 3, 5)
        ops = get_ops()
        trained = torch.is_grad_enabled() and self.proj.weight.requires_grad
        if ops.handles(x) and self._bf16_compute(x) and ops.gemm_supported(d, k) and (
                not trained or ops.wgrad_supported(d, k)) and (self.proj.bias is not None or self._frozen_bf16_no_bias()):
            # own GEMM (forward) / split-M weight gradient; the unfold and the cast to bf16 are ONE copy kernel
            patches = torch.empty(b, (h // p) * (w // p), k, dtype=torch.bfloat16, device=x.device)
            patches.view(b, h // p, w // p, c, p, p).copy_(unfolded)
            w2 = _matrix_view(self.proj.weight)
            if trained:
                with torch.autocast(device_type=x.device.type, enabled=False):
                    return _LinearFn.apply(patches, w2, self.proj.bias)
            if not torch.is_grad_enabled() and w2.dtype == torch.bfloat16 and (
                    self.proj.bias is None or self.proj.bias.dtype == torch.bfloat16):
                return ops.gemm_bf16(patches, w2, self.proj.bias)
            library_fallback("patch embedding", f"K={k} D={d}: bf16 compute of fp32 frozen weights")
            return F.linear(patches, w2.to(torch.bfloat16), self.proj.bias.to(torch.bfloat16))
        k_pad = (k + 63) // 64 * 64
        if (ops.handles(x) and not torch.is_grad_enabled() and self.proj.weight.dtype == torch.bfloat16
                and (self.proj.bias is None or self.proj.bias.dtype == torch.bfloat16) and ops.gemm_supported(d, k_pad)):
            # frozen bf16 layer whose patch is not a multiple of 64 values (ViT-H/14: 3 x 14 x 14 = 588): K padded with
            # zero columns on both operands (the padded weight is kept: the layer is frozen)
            patches = torch.zeros(b, (h // p) * (w // p), k_pad, dtype=torch.bfloat16, device=x.device)
            patches[..., :k].view(b, h // p, w // p, c, p, p).copy_(unfolded)
            cache = getattr(self, "_w_pad", None)
            if cache is None or cache[0] != self.proj.weight._version or cache[1].device != x.device:
                w_pad = torch.zeros(d, k_pad, dtype=torch.bfloat16, device=x.device)
                w_pad[:, :k].copy_(self.proj.weight.reshape(d, k))
                cache = (self.proj.weight._version, w_pad)
                self._w_pad = cache
            return ops.gemm_bf16(patches, cache[1], self.proj.bias)
        if (ops.handles(x) and trained and self._bf16_compute(x) and self.proj.bias is not None
                and ops.gemm_supported(d, k_pad) and ops.wgrad_supported(d, k_pad)):
            # trained layer with a short patch (BASELINE c1: 3 x 4 x 4 = 48 values): the same zero padding of K, the
            # weight padded per step inside the autograd function, its gradient cut back to [D, K]
            patches = torch.zeros(b, (h // p) * (w // p), k_pad, dtype=torch.bfloat16, device=x.device)
            patches[..., :k].view(b, h // p, w // p, c, p, p).copy_(unfolded)
            with torch.autocast(device_type=x.device.type, enabled=False):
                return _PaddedPatchFn.apply(patches, self.proj.weight.view(d, k), self.proj.bias)
        if ops.handles(x):
            library_fallback("patch embedding", f"K={k} D={d} dtype={x.dtype}")
        return F.linear(unfolded.reshape(b, -1, k), self.proj.weight.reshape(d, -1), self.proj.bias)

    def _frozen_bf16_no_bias(self) -> bool:
        """the patch embedding of a frozen pre-norm teacher (CLIP: ``norm_pre`` carries the offset)"""
        return (self.proj.bias is None and not torch.is_grad_enabled() and self.proj.weight.dtype == torch.bfloat16)

    def _bf16_compute(self, x) -> bool:
        if self.proj.weight.dtype == torch.bfloat16:
            return True                                      # frozen bf16 teacher
        dev = x.device.type
        return torch.is_autocast_enabled(dev) and torch.get_autocast_dtype(dev) == torch.bfloat16


class _PaddedPatchFn(torch.autograd.Function):
    """patches [B, N, K_pad] bf16 (zero beyond K) x weight [D, K] fp32 master + bias: forward on basd_gemm_bf16 with the
    weight zero-padded to K_pad, weight / bias gradient on basd_wgrad_bf16 (the K_pad - K extra columns are dropped).
    The images need no gradient."""

    @staticmethod
    def forward(ctx, patches, weight, bias):
        d, k = weight.shape
        w16 = torch.zeros(d, patches.shape[-1], dtype=torch.bfloat16, device=patches.device)
        w16[:, :k].copy_(weight)
        ctx.save_for_backward(patches)
        ctx.k = k
        return get_ops().gemm_bf16(patches, w16, bias.to(torch.bfloat16))

    @staticmethod
    def backward(ctx, g):
        (patches,) = ctx.saved_tensors
        g16 = g.to(torch.bfloat16).contiguous()
        gw, gb = get_ops().wgrad_bf16(g16.reshape(-1, g16.shape[-1]), patches.reshape(-1, patches.shape[-1]), need_bias=True)
        return None, gw[:, :ctx.k].contiguous(), gb


F32X3_PRECISIONS = ("high", "medium")


def _pad32(k: int) -> int:
    return (k + 31) // 32 * 32


def _matrix_view(weight: torch.Tensor) -> torch.Tensor:
    """[D, C, p, p] convolution weight as the [D, C p p] matrix of the GEMM; the bf16 image, the gradient slot in the
    flat buffer and the data-parallel hook of the parameter (trainer attributes) follow the view"""
    w2 = weight.view(weight.shape[0], -1)
    for name in ("_basd_bf16", "_basd_grad"):
        t = getattr(weight, name, None)
        if t is not None:
            setattr(w2, name, t.view(weight.shape[0], -1))
    ready = getattr(weight, "_basd_ready", None)
    if ready is not None:
        w2._basd_ready = ready
    return w2


class VisionTransformer(nn.Module):
    def __init__(self, img_size=224, patch_size=16, in_chans=3, num_classes=1000, embed_dim=768, depth=12,
                 num_heads=12, mlp_ratio=4.0, drop_path_rate=0.0, init_values=None, class_token=True,
                 pre_norm=False, act="gelu", norm_eps=1e-6, reg_tokens=0, mlp="mlp", mlp_hidden=None):
        super().__init__()
        if reg_tokens and not class_token:
            raise ValueError("VisionTransformer: register tokens stand behind a CLS token (class_token=False given)")
        self.embed_dim = self.num_features = embed_dim
        self.num_classes = num_classes
        self.patch_embed = PatchEmbed(img_size, patch_size, in_chans, embed_dim, bias=not pre_norm)
        n = self.patch_embed.num_patches
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim)) if class_token else None
        self.pos_embed = nn.Parameter(torch.randn(1, n + int(class_token), embed_dim) * 0.02)
        # timm's name (the hub checkpoint says register_tokens); None without registers: no new key in any other model.
        # The registers take no position row: pos_embed keeps its 1 + N rows
        self.reg_token = nn.Parameter(torch.randn(1, reg_tokens, embed_dim) * 0.02) if reg_tokens else None
        dpr = [drop_path_rate * i / max(depth - 1, 1) for i in range(depth)]
        self.blocks = nn.ModuleList([
            Block(embed_dim, num_heads, mlp_ratio, dpr[i], init_values, eps=norm_eps, act=act, mlp=mlp,
                  mlp_hidden=mlp_hidden) for i in range(depth)])
        self.norm = MixedLayerNorm(embed_dim, eps=norm_eps)
        # timm's name; None (not nn.Identity) without pre_norm: the module tree of every other model stays as it was
        self.norm_pre = MixedLayerNorm(embed_dim, eps=norm_eps) if pre_norm else None
        for i, blk in enumerate(self.blocks):
            blk._next_norm.append(self.blocks[i + 1].norm1 if i + 1 < depth else self.norm)
        self.head = nn.Linear(embed_dim, num_classes) if num_classes > 0 else nn.Identity()
        self.grad_checkpointing = False
        if self.cls_token is not None:
            nn.init.normal_(self.cls_token, std=1e-6)

    def set_grad_checkpointing(self, enable: bool = True):
        self.grad_checkpointing = enable
        for blk in self.blocks:
            blk.fuse_training = not enable

    def _f32x3_ok(self, x) -> bool:
        """The fp32 evaluation route: no grad, fp32 device activations, no autocast and
        torch.get_float32_matmul_precision() "high" or "medium" (the reference evaluates under "high": src/eval.py:16,
        src/training/trainer.py:183-188) -- every fp32 product on split-bf16 (bf16x3) MFMAs.  Under "highest" (torch's
        default) every path stays as it was."""
        ops = get_ops()
        if (torch.is_grad_enabled() or x.dtype != torch.float32 or x.dim() != 4 or not ops.handles(x)
                or not hasattr(ops, "gemm_f32x3") or torch.get_float32_matmul_precision() not in F32X3_PRECISIONS
                or torch.is_autocast_enabled(x.device.type)):
            return False
        pe, p = self.patch_embed, self.patch_embed.patch_size
        w = pe.proj.weight
        t = self.pos_embed.shape[1]
        return (self.norm_pre is None and self.reg_token is None and pe.proj.bias is not None and w.dtype == torch.float32 and pe.proj.bias.dtype == torch.float32
                and w.is_contiguous() and x.shape[2] % p == 0 and x.shape[3] % p == 0
                and (x.shape[2] // p) * (x.shape[3] // p) + int(self.cls_token is not None) == t
                and ops.f32x3_gemm_supported(self.embed_dim, _pad32(w[0].numel()))
                and isinstance(self.norm, MixedLayerNorm) and self.norm.elementwise_affine
                and all(isinstance(blk, Block) and blk._f32x3_supported(t) for blk in self.blocks))

    def _forward_features_f32x3(self, x):
        ops = get_ops()
        pe, p, d = self.patch_embed, self.patch_embed.patch_size, self.embed_dim
        b = x.shape[0]
        w = pe.proj.weight.detach().reshape(d, -1)
        kp = _pad32(w.shape[1])
        blocks = list(self.blocks)
        # the images of ALL weights, rebuilt every forward in one launch: the Schedule-Free eval / train switch rewrites
        # the parameters in place (training/optim.py) without moving their _version, so nothing is cached
        entries = [(w, kp)] + [(lin.weight.detach(), lin.in_features) for blk in blocks
                               for lin in (blk.attn.qkv, blk.attn.proj, blk.mlp.fc1, blk.mlp.fc2)]
        images = ops.split_table(entries)
        x = ops.gemm_f32x3(ops.split_patches(x, p, kp), images[0], pe.proj.bias.detach()).view(b, -1, d)
        if self.cls_token is not None:
            x = torch.cat([self.cls_token.expand(b, -1, -1), x], dim=1)
        x = x + self.pos_embed
        for i, blk in enumerate(blocks):
            blk._f32x3 = (images[1 + 4 * i:5 + 4 * i], self.norm)
        try:
            for blk in blocks:
                x = blk(x)              # module calls: forward hooks see the fp32 [B, T, D] block outputs
        finally:
            for blk in blocks:
                blk._f32x3 = None
        return self.norm(x)

    def forward_features(self, x):
        if self._f32x3_ok(x):
            return self._forward_features_f32x3(x)
        x = self.patch_embed(x)
        if self._fused_embed_ok(x):
            # frozen pre-norm and / or register-token teacher: CLS row, position embedding, register rows and norm_pre
            # in one kernel (csrc/vit_embed.hip)
            n = self.norm_pre
            gamma, beta, eps = (None, None, 1e-6) if n is None else (n.weight.detach().float(), n.bias.detach().float(),
                                                                      n.eps)
            if self.reg_token is None:
                x = get_ops().vit_embed(x, self.cls_token, self.pos_embed, gamma, beta, eps)
            else:
                x = get_ops().vit_embed(x, self.cls_token, self.pos_embed, gamma, beta, eps, reg=self.reg_token)
        else:
            if self.cls_token is not None:
                x = torch.cat([self.cls_token.expand(x.shape[0], -1, -1).to(x.dtype), x], dim=1)
            x = x + self.pos_embed.to(x.dtype)
            if self.reg_token is not None:      # behind the CLS row, after the position embedding (the DINOv2 forward)
                x = torch.cat([x[:, :1], self.reg_token.expand(x.shape[0], -1, -1).to(x.dtype), x[:, 1:]], dim=1)
            if self.norm_pre is not None:
                x = self.norm_pre(x)
        masks = self._draw_drop_path_masks(x)
        for i, blk in enumerate(self.blocks):
            dp = None if masks is None else (masks[0][2 * i], masks[0][2 * i + 1], masks[1][2 * i], masks[1][2 * i + 1])
            if self.grad_checkpointing and self.training and torch.is_grad_enabled():
                x = checkpoint(blk, x, dp, use_reentrant=False)
            else:
                x = blk(x, dp)
        return self.norm(x)

    def _fused_embed_ok(self, x) -> bool:
        """frozen bf16 model with ``norm_pre`` or register tokens on the device; every model with neither keeps the
        torch assembly"""
        n, cls, reg = self.norm_pre, self.cls_token, self.reg_token
        if reg is not None:
            if not _FUSED_DINOV2_DISPATCH or cls is None or reg.dtype != torch.bfloat16:
                return False
        elif n is None or not _FUSED_CLIP_DISPATCH:
            return False
        return (not torch.is_grad_enabled() and x.dtype == torch.bfloat16
                and x.dim() == 3 and get_ops().handles(x) and (n is None or n.elementwise_affine)
                and self.pos_embed.dtype == torch.bfloat16 and (cls is None or cls.dtype == torch.bfloat16)
                and x.shape[1] + int(cls is not None) == self.pos_embed.shape[1]
                and get_ops().vit_embed_supported(x.shape[-1]))

    def _draw_drop_path_masks(self, x):
        """All 2 * depth stochastic-depth masks of one forward from ONE bernoulli launch (timm draws one per
        DropPath call: 3 tiny kernels x 24), already divided by the keep probability: ([2 * depth, B, 1, 1] in the
        activation dtype, [2 * depth, B] fp32)."""
        if not self.training:
            return None
        ps = [p for blk in self.blocks for p in (blk.drop_path1.p, blk.drop_path2.p)]
        if not any(p > 0.0 for p in ps):
            return None
        keep = getattr(self, "_dp_keep", None)
        if keep is None or keep.device != x.device or keep.shape[0] != len(ps):
            keep = torch.tensor([1.0 - p for p in ps], device=x.device, dtype=torch.float32).view(-1, 1)
            self._dp_keep = keep
        m = torch.bernoulli(keep.expand(-1, x.shape[0])) / keep          # fp32 [2 * depth, B]: the fused kernels' scales
        return m.to(x.dtype).view(len(ps), x.shape[0], 1, 1), m

    def forward(self, x):
        x = self.forward_features(x)
        x = x[:, 0] if self.cls_token is not None else x.mean(dim=1)
        return self.head(x)


IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
CLIP_MEAN, CLIP_STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
HALF_MEAN, HALF_STD = (0.5, 0.5, 0.5), (0.5, 0.5, 0.5)


class ViTPreset(NamedTuple):
    embed_dim: int
    depth: int
    heads: int
    patch: int
    layerscale: float | None
    pre_norm: bool = False
    act: str = "gelu"
    class_token: bool = True
    norm_eps: float = 1e-6
    mean: tuple = IMAGENET_MEAN          # pretrained_cfg["mean"] / ["std"] of the timm model: the statistics that
    std: tuple = IMAGENET_STD            # normalise the teacher's clean view
    reg_tokens: int = 0                  # DINOv2 register tokens
    mlp: str = "mlp"                     # "mlp" (fc1 -> act -> fc2) or "swiglu" (ViT-g/14)
    mlp_hidden: int | None = None        # hidden width where it is not 4 x embed_dim


# name -> (embed_dim, depth, heads, patch, layerscale init[, pre_norm, act, class_token, norm_eps, mean, std,
#          reg_tokens, mlp, mlp_hidden])
# The CLIP / SigLIP rows were written WITHOUT timm at hand, from memory of timm 1.0.x (vision_transformer.py model
# entrypoints and default_cfgs): check them against the installed timm before loading real weights, and override with
# load_teacher(..., act=..., norm_eps=...) where they differ.  SigLIP's attention-pool head (attn_pool.*) is not built:
# the teacher never uses a head, and load_state_dict(strict=False) drops those keys.
def _dinov2(dim, depth, heads, reg=0, mlp="mlp", hidden=None):
    return (dim, depth, heads, 14, 1.0, False, "gelu", True, 1e-6, IMAGENET_MEAN, IMAGENET_STD, reg, mlp, hidden)


# The rest of the DINOv2 family: the register-token models (4 registers), ViT-g/14 (1536 wide, 40 blocks, 24 heads of 64,
# SwiGLU of hidden width 4096 = the hub's int(4 * 1536 * 2 / 3) rounded up to a multiple of 8) and timm's names for the
# same weights.  Written WITHOUT the hub code or timm at hand, from memory of facebookresearch/dinov2 (hubconf,
# vision_transformer.py, swiglu_ffn.py) and timm 1.0.x: check widths and the chunk order (x1 = the first half is the
# gated one) against the checkpoint before loading real weights.
_DINOV2_MORE = {
    "dinov2_vits14_reg": _dinov2(384, 12, 6, 4),
    "dinov2_vitb14_reg": _dinov2(768, 12, 12, 4),
    "dinov2_vitl14_reg": _dinov2(1024, 24, 16, 4),
    "dinov2_vitg14": _dinov2(1536, 40, 24, 0, "swiglu", 4096),
    "dinov2_vitg14_reg": _dinov2(1536, 40, 24, 4, "swiglu", 4096),
    "vit_small_patch14_reg4_dinov2": _dinov2(384, 12, 6, 4),
    "vit_base_patch14_reg4_dinov2": _dinov2(768, 12, 12, 4),
    "vit_large_patch14_reg4_dinov2": _dinov2(1024, 24, 16, 4),
    "vit_giant_patch14_dinov2": _dinov2(1536, 40, 24, 0, "swiglu", 4096),
    "vit_giant_patch14_reg4_dinov2": _dinov2(1536, 40, 24, 4, "swiglu", 4096),
}

VIT_PRESETS = {
    "deit_tiny_patch16_224": (192, 12, 3, 16, None),
    "deit_small_patch16_224": (384, 12, 6, 16, None),
    "deit_base_patch16_224": (768, 12, 12, 16, None),
    "vit_tiny_patch16_224": (192, 12, 3, 16, None),
    "vit_small_patch16_224": (384, 12, 6, 16, None),
    "vit_base_patch16_224": (768, 12, 12, 16, None),
    "vit_large_patch16_224": (1024, 24, 16, 16, None),
    "vit_huge_patch14_224": (1280, 32, 16, 14, None),
    "dinov2_vits14": (384, 12, 6, 14, 1.0),
    "dinov2_vitb14": (768, 12, 12, 14, 1.0),
    "dinov2_vitl14": (1024, 24, 16, 14, 1.0),
    "vit_base_patch32_clip_224": (768, 12, 12, 32, None, True, "gelu", True, 1e-5, CLIP_MEAN, CLIP_STD),
    "vit_base_patch16_clip_224": (768, 12, 12, 16, None, True, "gelu", True, 1e-5, CLIP_MEAN, CLIP_STD),
    "vit_large_patch14_clip_224": (1024, 24, 16, 14, None, True, "gelu", True, 1e-5, CLIP_MEAN, CLIP_STD),
    "vit_base_patch16_clip_quickgelu_224": (768, 12, 12, 16, None, True, "quick_gelu", True, 1e-5, CLIP_MEAN, CLIP_STD),
    "vit_large_patch14_clip_quickgelu_224": (1024, 24, 16, 14, None, True, "quick_gelu", True, 1e-5, CLIP_MEAN, CLIP_STD),
    "vit_base_patch16_siglip_224": (768, 12, 12, 16, None, False, "gelu_tanh", False, 1e-6, HALF_MEAN, HALF_STD),
    **_DINOV2_MORE,
}


def vit_preset(name: str) -> ViTPreset:
    """the preset's full record (the short rows above take the defaults of a plain ImageNet ViT)"""
    if name not in VIT_PRESETS:
        raise ValueError(f"unknown ViT preset {name!r}; known: {sorted(VIT_PRESETS)}")
    return ViTPreset(*VIT_PRESETS[name])


def create_vit(name: str, *, num_classes: int, img_size: int, drop_path_rate: float = 0.0,
               patch_size: int | None = None, act: str | None = None, norm_eps: float | None = None,
               **overrides) -> VisionTransformer:
    """timm.create_model stand-in for the presets above; ``overrides`` are the reference's
    ``model.arch_overrides`` keys (embed_dim, depth, num_heads, mlp_ratio; src/train.py:57-66); ``act`` / ``norm_eps``
    replace the preset's MLP activation / LayerNorm epsilon."""
    ps = vit_preset(name)
    kw = dict(embed_dim=ps.embed_dim, depth=ps.depth, num_heads=ps.heads, mlp_ratio=4.0)
    kw.update({k: v for k, v in overrides.items() if k in ("embed_dim", "depth", "num_heads", "mlp_ratio")})
    return VisionTransformer(img_size=img_size, patch_size=patch_size or ps.patch, num_classes=num_classes,
                             drop_path_rate=drop_path_rate, init_values=ps.layerscale, class_token=ps.class_token,
                             pre_norm=ps.pre_norm, act=act or ps.act, norm_eps=norm_eps or ps.norm_eps,
                             reg_tokens=ps.reg_tokens, mlp=ps.mlp, mlp_hidden=ps.mlp_hidden, **kw)


def dinov2_state_dict(model: VisionTransformer, state: dict) -> dict:
    """A DINOv2 state dict under the hub's or timm's key names -> this model's names: the hub's ``register_tokens`` is
    ``reg_token`` here (timm's name), ``mask_token`` (the iBOT mask embedding, unused in a forward without masks) is
    dropped, and for a SwiGLU model timm's ``blocks.i.mlp.fc1`` / ``fc2`` (SwiGLUPacked) are the hub's ``w12`` / ``w3``.
    Every other key passes through."""
    swiglu = any(isinstance(blk.mlp, SwiGLU) for blk in model.blocks)
    out = {}
    for key, value in state.items():
        if key == "mask_token":
            continue
        if key == "register_tokens":
            key = "reg_token"
        elif swiglu and ".mlp.fc1." in key:
            key = key.replace(".mlp.fc1.", ".mlp.w12.")
        elif swiglu and ".mlp.fc2." in key:
            key = key.replace(".mlp.fc2.", ".mlp.w3.")
        out[key] = value
    return out
