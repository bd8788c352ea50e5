"""Functional restatement of ConvNeXt-V2's ``forward_features`` on a state dict (timm parameter names), written from
the published architecture with ``F.conv2d`` / ``F.layer_norm`` / ``F.linear`` / ``F.gelu``.  It shares no code with
``basd_amd.models.convnext``; the tests run it in fp64 as the reference and in fp32 to measure its own rounding."""
from __future__ import annotations

import torch
import torch.nn.functional as F


def expected_state(depths, dims, in_chans=3):
    """{parameter name: shape} of ConvNeXtV2(depths, dims) without a head, generated from the architecture."""
    out = {"stem.0.weight": (dims[0], in_chans, 4, 4), "stem.0.bias": (dims[0],),
           "stem.1.weight": (dims[0],), "stem.1.bias": (dims[0],)}
    for i, (depth, c) in enumerate(zip(depths, dims)):
        if i > 0:
            out[f"stages.{i}.downsample.0.weight"] = (dims[i - 1],)
            out[f"stages.{i}.downsample.0.bias"] = (dims[i - 1],)
            out[f"stages.{i}.downsample.1.weight"] = (c, dims[i - 1], 2, 2)
            out[f"stages.{i}.downsample.1.bias"] = (c,)
        for j in range(depth):
            pre = f"stages.{i}.blocks.{j}."
            out.update({pre + "conv_dw.weight": (c, 1, 7, 7), pre + "conv_dw.bias": (c,),
                        pre + "norm.weight": (c,), pre + "norm.bias": (c,),
                        pre + "mlp.fc1.weight": (4 * c, c), pre + "mlp.fc1.bias": (4 * c,),
                        pre + "mlp.grn.weight": (4 * c,), pre + "mlp.grn.bias": (4 * c,),
                        pre + "mlp.fc2.weight": (c, 4 * c), pre + "mlp.fc2.bias": (c,)})
    return out


def _ln_channels(x, w, b, eps=1e-6):
    """LayerNorm over the channel axis of an NCHW map"""
    return F.layer_norm(x.permute(0, 2, 3, 1), (x.shape[1],), w, b, eps).permute(0, 3, 1, 2)


def grn(x, weight, bias, eps=1e-6):
    """x [B, H, W, C]: g = L2 norm over (H, W), n = g / (mean_C g + eps), x + bias + weight x n"""
    g = (x * x).sum(dim=(1, 2), keepdim=True).sqrt()
    n = g / (g.mean(dim=-1, keepdim=True) + eps)
    return x + bias + weight * x * n


def forward_features(state, x, depths, dtype=torch.float64):
    sd = {k: v.detach().to("cpu", dtype) for k, v in state.items()}
    x = x.detach().to("cpu", dtype)
    x = F.conv2d(x, sd["stem.0.weight"], sd["stem.0.bias"], stride=4)
    x = _ln_channels(x, sd["stem.1.weight"], sd["stem.1.bias"])
    for i, depth in enumerate(depths):
        if i > 0:
            x = _ln_channels(x, sd[f"stages.{i}.downsample.0.weight"], sd[f"stages.{i}.downsample.0.bias"])
            x = F.conv2d(x, sd[f"stages.{i}.downsample.1.weight"], sd[f"stages.{i}.downsample.1.bias"], stride=2)
        for j in range(depth):
            p = f"stages.{i}.blocks.{j}."
            c = x.shape[1]
            y = F.conv2d(x, sd[p + "conv_dw.weight"], sd[p + "conv_dw.bias"], padding=3, groups=c)
            y = F.layer_norm(y.permute(0, 2, 3, 1), (c,), sd[p + "norm.weight"], sd[p + "norm.bias"], 1e-6)
            y = F.gelu(F.linear(y, sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"]))
            y = grn(y, sd[p + "mlp.grn.weight"], sd[p + "mlp.grn.bias"])
            y = F.linear(y, sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"])
            x = x + y.permute(0, 3, 1, 2)
    return x


def randomise_affine(model, seed=0):
    """A seeded random model has every conv / linear bias at 0 and every LayerNorm at (1, 0), which is blind to a
    dropped or mis-padded bias image and to gamma / beta changing places; pretrained weights have neither.  Biases
    ~ N(0, 0.3), gamma ~ 1 + 0.3 N, beta ~ 0.3 N, in place, whatever the parameters' dtype and device."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.LayerNorm):
                m.weight.copy_(1.0 + 0.3 * torch.randn(m.weight.shape, generator=g))
                m.bias.copy_(0.3 * torch.randn(m.bias.shape, generator=g))
            elif isinstance(m, (torch.nn.Conv2d, torch.nn.Linear)) and m.bias is not None:
                m.bias.copy_(0.3 * torch.randn(m.bias.shape, generator=g))
    return model


def tokens(feat):
    """[B, C, H, W] -> [B, H W, C]"""
    return feat.flatten(2).transpose(1, 2)


def rel_l2_per_sample(got, want):
    got, want = got.double().flatten(1), want.double().flatten(1)
    return (got - want).norm(dim=1) / want.norm(dim=1)
