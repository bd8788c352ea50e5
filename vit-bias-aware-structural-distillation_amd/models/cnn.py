"""Convolutional teachers for the cross-architecture configuration: the ResNets defined here (BASELINE configs[2]:
ResNet-50 teacher, single "layer" of 7 x 7 = 49 tokens x 2048 channels, uniform importance) and the ConvNeXt-V2
family of ``models/convnext.py`` (what the reference's cross-arch overlay names,
``configs/experiment/basd_imagenet_cross_arch.yaml:6``), both listed in ``CNN_PRESETS`` -- the table of every teacher
that hands over ONE feature map instead of per-block tokens, which is why the Swin family of ``models/swin.py`` (a
hierarchical ViT with an NHWC map of 7 x 7 x 768 / 1024) is listed there too.

The reference takes CNN teachers from timm (``src/models/teacher.py:118``) and only ever calls ``forward_features``
on them (``teacher.py:184-191``).  timm / torchvision are not available offline, so the trunks are defined in this
package with the torchvision / timm parameter names (``conv1``, ``bn1``, ``layer1..4.N.conv1`` ...) so that a local
state dict of either package loads.

Two forwards of the same ResNet parameters, under the protocol and with the image helpers of
``models/fused_trunk.py``:

* plain PyTorch (``nn.Conv2d``, ``nn.BatchNorm2d``, ``nn.MaxPool2d``): the CPU path, the path of every dtype but bf16
  and of a model with gradients; on the device it runs in library kernels (MIOpen);
* the fused inference path of a frozen bf16 model on the device (``prepare_fused`` once after the weights are
  loaded): BatchNorm is folded into weight and bias, activations are channels-last rows ``[B H W, ld]`` (64 channels
  in rows of 128), the 1 x 1 convolutions are ``basd_gemm_bf16`` (the strided one behind a ``basd_patchify_bf16``
  row gather), the 3 x 3 convolutions, the stem, the pool and the residual add + ReLU are ``csrc/resnet.hip``.  It
  enqueues no convolution, batch-norm, pooling or GEMM of a library.  A bf16 no-grad device forward that cannot
  take it is reported through ``library_fallback``.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from ..losses._ops import get_ops
from .convnext import CONVNEXT_PRESETS
from .fused_trunk import FusedTrunk, padded_image, patch_image, row_width
from .swin import SWIN_PRESETS


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes: int, planes: int, stride: int = 1, downsample: nn.Module | None = None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * self.expansion, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * self.expansion)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample

    def forward(self, x):
        idt = x if self.downsample is None else self.downsample(x)
        y = self.relu(self.bn1(self.conv1(x)))
        y = self.relu(self.bn2(self.conv2(y)))
        y = self.bn3(self.conv3(y))
        return self.relu(y + idt)


class ResNet(FusedTrunk, nn.Module):
    """ResNet-v1.5 trunk (stride on the 3x3 convolution), stages ``layer1..layer4`` as in torchvision / timm."""
    _fallback_name = "resnet trunk"

    def __init__(self, depths=(3, 4, 6, 3), num_classes: int = 0, in_chans: int = 3):
        super().__init__()
        self.inplanes = 64
        self.conv1 = nn.Conv2d(in_chans, 64, 7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, stride=2, padding=1)
        for i, (planes, depth) in enumerate(zip((64, 128, 256, 512), depths)):
            setattr(self, f"layer{i + 1}", self._stage(planes, depth, stride=1 if i == 0 else 2))
        self.num_features = self.embed_dim = 512 * Bottleneck.expansion
        self.fc = nn.Linear(self.num_features, num_classes) if num_classes > 0 else nn.Identity()
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")

    def _stage(self, planes, depth, stride):
        down = None
        if stride != 1 or self.inplanes != planes * Bottleneck.expansion:
            down = nn.Sequential(nn.Conv2d(self.inplanes, planes * Bottleneck.expansion, 1, stride=stride, bias=False),
                                 nn.BatchNorm2d(planes * Bottleneck.expansion))
        blocks = [Bottleneck(self.inplanes, planes, stride, down)]
        self.inplanes = planes * Bottleneck.expansion
        blocks += [Bottleneck(self.inplanes, planes) for _ in range(depth - 1)]
        return nn.Sequential(*blocks)

    # ------------------------------------------------------------------------------------------------- plain PyTorch
    def _forward_plain(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        return self.layer4(self.layer3(self.layer2(self.layer1(x))))        # [B, 2048, H/32, W/32]

    # ------------------------------------------------------------------------------------------------- fused path
    def _stages(self):
        return [getattr(self, f"layer{i}") for i in range(1, 5)]

    def fused_refusal(self) -> str | None:
        """Why the kernels do not take this architecture (None: they do)."""
        ops = get_ops()
        if not hasattr(ops, "conv3x3"):
            return "the kernel provider has no ResNet trunk entries"
        if self.conv1.weight.shape[1] != 3:
            return f"the stem kernel takes 3 input channels (got {self.conv1.weight.shape[1]})"
        ld = row_width(64)
        if not (ops.conv7x7s2_relu_supported(ld) and ops.maxpool3x3s2_supported(64, ld, ld)):
            return f"stem rows of {ld} are not tiled by the stem / pool kernels"
        c_in = 64
        for stage in self._stages():
            for blk in stage:
                if not isinstance(blk, Bottleneck):
                    return f"{type(blk).__name__} blocks (bottleneck blocks only)"
                p, c_out, s = blk.conv2.weight.shape[0], blk.conv3.weight.shape[0], blk.conv2.stride[0]
                ld_in, ld_p, ld_o = row_width(c_in), row_width(p), row_width(c_out)
                if not (ops.gemm_supported(ld_p, ld_in) and ops.conv3x3_supported(p, ld_p, ld_p, s)
                        and ops.gemm_supported(ld_o, ld_p) and ops.gemm_supported(ld_o, ld_in)
                        and ld_o == c_out and ops.add_relu_supported(c_out, ld_o, ld_o)):
                    return f"bottleneck {c_in} -> {p} -> {c_out} (stride {s}) is not tiled by the GEMM / trunk kernels"
                c_in = c_out
        return None

    def _build_fused(self):
        """The weight images of ``prepare_fused``.  BatchNorm is folded in fp32 from the stored parameters, s = gamma /
        sqrt(var + eps): w' = bf16(w s), b' = bf16(beta - mean s), one rounding.  The 3 x 3 images are tap-major
        [C, 9 C], the 1 x 1 images zero-padded [N_ld, K_ld], the stem image [64, K_pad] in the kernel's patch order."""
        ops = get_ops()

        def folded(conv, bn, n_ld, k_ld):
            s = bn.weight.float() / torch.sqrt(bn.running_var.float() + bn.eps)
            w = patch_image(conv.weight.float() * s.view(-1, 1, 1, 1))
            return padded_image(w, bn.bias.float() - bn.running_mean.float() * s, n_ld, k_ld)

        def pointwise(conv, bn, ld_in):
            return folded(conv, bn, row_width(conv.weight.shape[0]), ld_in)

        fused = {"ld0": row_width(64), "blocks": [], "stem": folded(self.conv1, self.bn1, 64, ops.STEM_K_PAD)}
        c_in = 64
        for stage in self._stages():
            for blk in stage:
                p = blk.conv2.weight.shape[0]
                ld_in = row_width(c_in)
                rec = {"c1": pointwise(blk.conv1, blk.bn1, ld_in), "planes": p, "stride": blk.conv2.stride[0],
                       "c2": folded(blk.conv2, blk.bn2, p, 9 * p),
                       "c3": pointwise(blk.conv3, blk.bn3, row_width(p)), "down": None}
                if blk.downsample is not None:
                    rec["down"] = pointwise(blk.downsample[0], blk.downsample[1], ld_in)
                fused["blocks"].append(rec)
                c_in = blk.conv3.weight.shape[0]
        fused["c_last"] = c_in
        return fused

    def _forward_fused(self, x):
        """x [B, 3, H, W] bf16 (any strides) -> [B, 2048, H/32, W/32] bf16, a channels-last view of the last rows"""
        ops, fz = get_ops(), self._fused
        ld = fz["ld0"]
        t = ops.maxpool3x3s2(ops.conv7x7s2_relu(x, *fz["stem"], ld_out=ld), 64, ld)
        b, h, w, _ = t.shape
        rows = t.view(b * h * w, ld)
        for rec in fz["blocks"]:
            ld_in, s = rows.shape[1], rec["stride"]
            y = ops.gemm_bf16(rows, *rec["c1"])                                          # conv1 + bn1; its ReLU ...
            y = ops.conv3x3(y.view(b, h, w, y.shape[1]), *rec["c2"], stride=s, relu_in=True, relu_out=True)   # ... here
            ho, wo = y.shape[1], y.shape[2]
            y = ops.gemm_bf16(y.view(b * ho * wo, y.shape[3]), *rec["c3"])
            idt = rows
            if rec["down"] is not None:
                if s != 1:                                                               # rows of the [::s, ::s] pixels
                    grid = rows.view(b, h, w, ld_in).permute(0, 3, 1, 2)[:, :, ::s, ::s]
                    idt = ops.patchify(grid, 1, ld_in)
                idt = ops.gemm_bf16(idt, *rec["down"])
            rows = ops.add_relu_(y, idt)
            h, w = ho, wo
        return rows.view(b, h, w, rows.shape[1])[..., :fz["c_last"]].permute(0, 3, 1, 2)

    def _takes_fused(self, x) -> bool:
        return (self._fused is not None and not torch.is_grad_enabled() and x.dtype == torch.bfloat16 and x.dim() == 4
                and x.shape[1] == 3 and self.conv1.weight.dtype == torch.bfloat16)

    def _reports(self, x) -> bool:
        # only a bf16 no-grad forward is reported: every other dtype and a model with gradients take the plain path
        return x.dtype == torch.bfloat16 and not torch.is_grad_enabled() and get_ops().handles(x)

    def _fallback_detail(self, x) -> str:
        return f"shape={tuple(x.shape)} weights={self.conv1.weight.dtype} prepared={self._fused is not None}"

    def forward(self, x):
        return self.fc(self.forward_features(x).mean(dim=(2, 3)))


CNN_PRESETS = {
    "resnet50": lambda: ResNet((3, 4, 6, 3)),
    "resnet101": lambda: ResNet((3, 4, 23, 3)),
    **CONVNEXT_PRESETS,
    **SWIN_PRESETS,
}


def create_cnn(name: str) -> nn.Module:
    if name not in CNN_PRESETS:
        raise ValueError(f"unknown CNN preset {name!r}; known: {sorted(CNN_PRESETS)}")
    return CNN_PRESETS[name]()
