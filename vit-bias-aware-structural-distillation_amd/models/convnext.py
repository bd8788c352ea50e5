"""ConvNeXt-V2 teacher for the cross-architecture configuration (the reference's
``configs/experiment/basd_imagenet_cross_arch.yaml:6`` names timm's ``convnextv2_tiny.fcmae`` and only ever calls
``forward_features`` on it, ``src/models/teacher.py:184-191``).

timm is not available offline, so the trunk is defined here from the published architecture with timm's parameter
names (stated assumption; the architecture itself is pinned by ``tests/_convnext_ref.py``):

* ``stem.0`` Conv2d 4x4 stride 4 + bias, ``stem.1`` LayerNorm over channels (eps 1e-6)
* ``stages.{i}.downsample.0`` LayerNorm over channels, ``.downsample.1`` Conv2d 2x2 stride 2 + bias (stage 0: identity)
* ``stages.{i}.blocks.{j}``: ``conv_dw`` (depthwise 7x7, padding 3, bias), ``norm`` (LayerNorm over channels),
  ``mlp.fc1`` (C -> 4C), exact GELU, ``mlp.grn.weight / .bias`` [4C], ``mlp.fc2`` (4C -> C), residual add
* ``forward_features`` = stem + the four stages -> ``[B, C_last, H/32, W/32]``

Two forwards of the same parameters, under the protocol and with the image helpers of ``models/fused_trunk.py``:

* plain PyTorch (``nn.Conv2d``, ``F.layer_norm``, ``nn.Linear``): the CPU path, and on the device the path of any
  shape / dtype the kernels refuse -- reported through ``library_fallback`` like every other layer;
* the fused inference path of a frozen bf16 model on the device (``prepare_fused`` once after the weights are loaded):
  activations are channels-last rows ``[B H W, ld]``, the pointwise layers and the strided convolutions are
  ``basd_gemm_bf16`` (GELU in fc1's epilogue), the rest is ``csrc/convnext.hip``.  Widths the GEMM does not tile live
  in zero-padded rows (96 channels in rows of 128).  It enqueues no library GEMM and no convolution.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..losses._ops import get_ops
from .fused_trunk import FusedTrunk, centre_tap_identity, norm_params, padded_image, patch_image, row_width


class LayerNorm2d(nn.LayerNorm):
    """LayerNorm over the channels of an NCHW map."""

    def forward(self, x):
        y = F.layer_norm(x.permute(0, 2, 3, 1).float(), self.normalized_shape, self.weight, self.bias, self.eps)
        return y.to(x.dtype).permute(0, 3, 1, 2)


class GRN(nn.Module):
    """Global response normalisation on channels-last ``[B, H, W, C]``."""

    def __init__(self, dim: int, eps: float = 1e-6):
        super().__init__()
        self.eps = eps
        self.weight = nn.Parameter(torch.zeros(dim))
        self.bias = nn.Parameter(torch.zeros(dim))

    def _apply(self, fn, *args, **kwargs):
        # weight / bias stay fp32 like the LayerNorm parameters of a frozen teacher: a dtype cast of the model
        # (``model.to(torch.bfloat16)``) moves them to the new device but does not round pretrained values
        def keep_dtype(t):
            out = fn(t)
            return t.to(device=out.device) if out.is_floating_point() and out.dtype != t.dtype else out
        return super()._apply(keep_dtype, *args, **kwargs)

    def forward(self, x):
        xf = x.float()
        g = xf.norm(p=2, dim=(1, 2), keepdim=True)
        n = g / (g.mean(dim=-1, keepdim=True) + self.eps)
        return (xf + (self.bias.float() + self.weight.float() * (xf * n))).to(x.dtype)


class _Mlp(nn.Module):
    def __init__(self, dim: int):
        super().__init__()
        self.fc1 = nn.Linear(dim, 4 * dim)
        self.act = nn.GELU()
        self.grn = GRN(4 * dim)
        self.fc2 = nn.Linear(4 * dim, dim)

    def forward(self, x):
        return self.fc2(self.grn(self.act(self.fc1(x))))


class ConvNeXtBlock(nn.Module):
    def __init__(self, dim: int):
        super().__init__()
        self.conv_dw = nn.Conv2d(dim, dim, 7, padding=3, groups=dim)
        self.norm = nn.LayerNorm(dim, eps=1e-6)
        self.mlp = _Mlp(dim)

    def forward(self, x):
        y = self.conv_dw(x).permute(0, 2, 3, 1)
        y = F.layer_norm(y.float(), self.norm.normalized_shape, self.norm.weight, self.norm.bias, self.norm.eps).to(x.dtype)
        return x + self.mlp(y).permute(0, 3, 1, 2)


class ConvNeXtStage(nn.Module):
    def __init__(self, in_dim: int, dim: int, depth: int, first: bool):
        super().__init__()
        self.downsample = nn.Identity() if first else nn.Sequential(LayerNorm2d(in_dim, eps=1e-6),
                                                                   nn.Conv2d(in_dim, dim, 2, stride=2))
        self.blocks = nn.Sequential(*[ConvNeXtBlock(dim) for _ in range(depth)])

    def forward(self, x):
        return self.blocks(self.downsample(x))


class ConvNeXtV2(FusedTrunk, nn.Module):
    _fallback_name = "convnext trunk"

    def __init__(self, depths=(3, 3, 9, 3), dims=(96, 192, 384, 768), num_classes: int = 0, in_chans: int = 3):
        super().__init__()
        self.depths, self.dims = tuple(depths), tuple(dims)
        self.stem = nn.Sequential(nn.Conv2d(in_chans, dims[0], 4, stride=4), LayerNorm2d(dims[0], eps=1e-6))
        self.stages = nn.Sequential(*[ConvNeXtStage(dims[max(i - 1, 0)], dims[i], depths[i], first=i == 0)
                                      for i in range(len(dims))])
        self.num_features = self.embed_dim = dims[-1]
        self.head = nn.Linear(dims[-1], num_classes) if num_classes > 0 else nn.Identity()
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                nn.init.trunc_normal_(m.weight, std=0.02)
                nn.init.zeros_(m.bias)
            elif isinstance(m, GRN):          # timm starts GRN at zero (an identity); a random teacher should exercise it
                nn.init.normal_(m.weight, std=0.1)
                nn.init.normal_(m.bias, std=0.02)

    # ------------------------------------------------------------------------------------------------- plain PyTorch
    def _forward_plain(self, x):
        return self.stages(self.stem(x))

    # ------------------------------------------------------------------------------------------------- fused path
    def fused_refusal(self) -> str | None:
        """Why the kernels do not take this architecture (None: they do)."""
        ops = get_ops()
        for c in self.dims:
            ld = row_width(c)
            if not (ops.dwconv7_ln_supported(c, ld, ld) and ops.grn_supported(4 * c) and ops.gemm_supported(4 * c, ld)
                    and ops.gemm_supported(ld, 4 * c) and ops.layernorm_supported(c)):
                return f"width {c} (rows of {ld}, hidden {4 * c}) is not tiled by the GEMM / trunk kernels"
        return None

    def _build_fused(self):
        """The weight images of ``prepare_fused``: tap-major depthwise weights, zero-padded GEMM images in the patch
        order of ``basd_patchify_bf16`` (K rounded up to a multiple of 64), fp32 norm / GRN parameters."""
        bf, f32 = torch.bfloat16, torch.float32
        lds = [row_width(c) for c in self.dims]

        def conv_image(conv, c_in_ld, n_ld):
            w2d = patch_image(conv.weight, c_in_ld)
            k_pad = (w2d.shape[1] + 63) // 64 * 64
            return padded_image(w2d, conv.bias, n_ld, k_pad) + (k_pad,)

        dev = self.stem[0].weight.device
        fused = {"lds": lds, "stages": []}
        fused["stem"] = conv_image(self.stem[0], self.stem[0].weight.shape[1], lds[0])
        fused["stem_norm"] = norm_params(self.stem[1])
        fused["ident"] = {c: centre_tap_identity(c, dev) for c, ld in zip(self.dims, lds) if ld != c}
        for i, stage in enumerate(self.stages):
            c, ld = self.dims[i], lds[i]
            rec = {"down": None, "blocks": []}
            if i > 0:
                rec["down"] = norm_params(stage.downsample[0]) + conv_image(stage.downsample[1], lds[i - 1], ld)
            for blk in stage.blocks:
                gamma, beta, eps = norm_params(blk.norm)
                w1, b1 = padded_image(blk.mlp.fc1.weight, blk.mlp.fc1.bias, 4 * c, ld)
                w2, b2 = padded_image(blk.mlp.fc2.weight, blk.mlp.fc2.bias, ld, 4 * c)
                rec["blocks"].append({
                    "w49": blk.conv_dw.weight.reshape(c, 49).t().contiguous().to(bf), "dw_bias": blk.conv_dw.bias.to(f32),
                    "gamma": gamma, "beta": beta, "eps": eps, "w1": w1, "b1": b1, "grn_w": blk.mlp.grn.weight.to(f32),
                    "grn_b": blk.mlp.grn.bias.to(f32), "grn_eps": blk.mlp.grn.eps, "w2": w2, "b2": b2})
            fused["stages"].append(rec)
        return fused

    def _forward_fused(self, x):
        """x [B, 3, H, W] bf16 (any strides) -> [B, C_last, H/32, W/32] bf16, a channels-last view of the last rows"""
        ops, fz = get_ops(), self._fused
        lds = fz["lds"]
        b, _, h, w = x.shape
        w_img, b_img, k_pad = fz["stem"]
        h, w = h // 4, w // 4
        t = ops.gemm_bf16(ops.patchify(x, 4, k_pad), w_img, b_img)                       # [B h w, ld0]
        t = self._norm_rows(ops, t, self.dims[0], *fz["stem_norm"])
        for i, rec in enumerate(fz["stages"]):
            c, ld = self.dims[i], lds[i]
            if rec["down"] is not None:
                gamma, beta, eps, w_img, b_img, k_pad = rec["down"]
                t = self._norm_rows(ops, t, self.dims[i - 1], gamma, beta, eps)
                grid = t.view(b, h, w, lds[i - 1]).permute(0, 3, 1, 2)                   # NCHW view of the padded rows
                h, w = h // 2, w // 2
                t = ops.gemm_bf16(ops.patchify(grid, 2, k_pad), w_img, b_img)             # [B h w, ld]
            for blk in rec["blocks"]:
                y = ops.dwconv7_ln(t.view(b, h, w, ld), blk["w49"], blk["dw_bias"], blk["gamma"], blk["beta"], blk["eps"])
                hid = ops.gemm_bf16(y.view(b * h * w, ld), blk["w1"], blk["b1"], gelu=True)
                ops.grn_(hid.view(b, h * w, 4 * c), blk["grn_w"], blk["grn_b"], blk["grn_eps"])
                t.add_(ops.gemm_bf16(hid, blk["w2"], blk["b2"]))                         # residual: one in-place add
        return t.view(b, h, w, lds[-1])[..., :self.dims[-1]].permute(0, 3, 1, 2)

    def _takes_fused(self, x) -> bool:
        return (self._fused is not None and not torch.is_grad_enabled() and x.dtype == torch.bfloat16 and x.dim() == 4
                and x.shape[2] % 32 == 0 and x.shape[3] % 32 == 0 and self.stem[0].weight.dtype == torch.bfloat16)

    def forward(self, x):
        return self.head(self.forward_features(x).mean(dim=(2, 3)))


CONVNEXT_PRESETS = {
    "convnextv2_nano": lambda: ConvNeXtV2((2, 2, 8, 2), (80, 160, 320, 640)),
    "convnextv2_tiny": lambda: ConvNeXtV2((3, 3, 9, 3), (96, 192, 384, 768)),
    "convnextv2_base": lambda: ConvNeXtV2((3, 3, 27, 3), (128, 256, 512, 1024)),
}
