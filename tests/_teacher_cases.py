"""Shared by the tests of the one-feature-map teachers (ResNet, ConvNeXt-V2, Swin): the test images, the frozen bf16
preamble and the strict-mode fused forward next to the module's own plain forward.  A plain helper module."""
import contextlib

import torch
from torch.utils._python_dispatch import TorchDispatchMode


def images(batch, size, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(batch, 3, size, size, generator=g)
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, size), torch.linspace(-1, 1, size), indexing="ij")
    return x + 2.0 * torch.sin(3.0 * xx) * torch.cos(2.0 * yy)


def bf16_frozen(model, memory_format=None):
    """a frozen teacher as ``load_teacher`` leaves it: no gradients, bf16 parameters, LayerNorm kept fp32, eval mode"""
    for p in model.parameters():
        p.requires_grad = False
    model = model.to(torch.bfloat16)
    if memory_format is not None:
        model = model.to(memory_format=memory_format)
    for m in model.modules():
        if isinstance(m, torch.nn.LayerNorm):
            m.float()
    return model.eval()


class _OpNames(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.names = set()

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.names.add(func._schema.name)
        return func(*args, **(kwargs or {}))


def fused_and_library(model, x, forbidden_ops=()):
    """-> (fused, library) forwards of x on the device in bf16 channels-last.  The fused one runs under strict mode and
    must report no fallback and reach no library GEMM; with ``forbidden_ops`` it must also run no aten operator whose
    name contains one of them."""
    import basd_amd.losses._ops as O
    xd = x.cuda().to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    O.FALLBACKS.clear()
    O.set_strict(True)
    ops = _OpNames()
    try:
        with torch.no_grad(), O.record_library_gemms() as seen, (ops if forbidden_ops else contextlib.nullcontext()):
            fused = model.forward_features(xd)
    finally:
        O.set_strict(False)
    assert not O.FALLBACKS and not seen, (dict(O.FALLBACKS), seen)
    library = sorted(n for n in ops.names if any(k in n for k in forbidden_ops))
    assert not library, library
    with torch.no_grad():
        lib = model._forward_plain(xd)
    torch.cuda.synchronize()
    return fused, lib
