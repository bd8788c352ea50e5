"""fp64 restatement of the ResNet-v1.5 bottleneck trunk (``models/cnn.py::ResNet.forward_features``) from a state dict
with the torchvision / timm parameter names, independent of the module: plain conv2d / batch-norm formulas."""
from __future__ import annotations

import torch
import torch.nn.functional as F

EPS = 1e-5


def _bn(state, name, x, dtype):
    g, b = state[f"{name}.weight"].to(dtype), state[f"{name}.bias"].to(dtype)
    m, v = state[f"{name}.running_mean"].to(dtype), state[f"{name}.running_var"].to(dtype)
    s = g / torch.sqrt(v + EPS)
    return x * s.view(1, -1, 1, 1) + (b - m * s).view(1, -1, 1, 1)


def _conv(state, name, x, dtype, stride=1, padding=0):
    return F.conv2d(x, state[f"{name}.weight"].to(dtype), stride=stride, padding=padding)


def forward_features(state, x, depths, dtype=torch.float64):
    """x [B, 3, H, W] -> [B, 2048, H/32, W/32]; the stride of a stage's first block sits on its 3 x 3 convolution"""
    x = x.to(dtype)
    x = F.relu(_bn(state, "bn1", _conv(state, "conv1", x, dtype, stride=2, padding=3), dtype))
    x = F.max_pool2d(x, 3, stride=2, padding=1)
    for i, depth in enumerate(depths):
        for j in range(depth):
            p = f"layer{i + 1}.{j}"
            stride = 2 if (i > 0 and j == 0) else 1
            idt = x
            if f"{p}.downsample.0.weight" in state:
                idt = _bn(state, f"{p}.downsample.1", _conv(state, f"{p}.downsample.0", x, dtype, stride=stride), dtype)
            y = F.relu(_bn(state, f"{p}.bn1", _conv(state, f"{p}.conv1", x, dtype), dtype))
            y = F.relu(_bn(state, f"{p}.bn2", _conv(state, f"{p}.conv2", y, dtype, stride=stride, padding=1), dtype))
            y = _bn(state, f"{p}.bn3", _conv(state, f"{p}.conv3", y, dtype), dtype)
            x = F.relu(y + idt)
    return x


def randomise_bn(model, seed=0):
    """A fresh BatchNorm is (gamma, beta, mean, var) = (1, 0, 0, 1): folding it is an identity and would prove nothing
    about the fold, the bias images or mean and beta changing places.  gamma = 1 + 0.2 N, beta = 0.1 N, mean = 0.2 N,
    var = 0.5 + U, in place, whatever the parameters' dtype and device."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                n = m.weight.shape
                m.weight.copy_(1.0 + 0.2 * torch.randn(n, generator=g))
                m.bias.copy_(0.1 * torch.randn(n, generator=g))
                m.running_mean.copy_(0.2 * torch.randn(n, generator=g))
                m.running_var.copy_(0.5 + torch.rand(n, generator=g))
    return model


def tokens(feat):
    """[B, C, H, W] -> [B, H W, C]"""
    return feat.flatten(2).transpose(1, 2)


def rel_l2_per_sample(got, want):
    got, want = got.double().flatten(1), want.double().flatten(1)
    return (got - want).norm(dim=1) / want.norm(dim=1)
