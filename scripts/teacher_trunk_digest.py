"""sha256 digests of the fused teacher trunks (ResNet, ConvNeXt-V2, Swin): per case one line for the output of
``forward_features`` and one for every tensor of the prepared weight images, in the order of a walk through ``_fused``
(dicts by insertion order, lists and tuples by index).  The trunk kernels carry no atomics, so two commits that build
the same images and pass the same arguments print the same lines: run this file at both and ``diff`` the outputs.  It
uses only names both sides of a host-side refactor of the trunks have.

    python scripts/teacher_trunk_digest.py [--emulated] > digests.txt

Per case: the model from a fixed seed, its affine parameters / statistics randomised (``tests/_*_ref.randomise_*``),
frozen, cast to bf16 (LayerNorm kept fp32), ``prepare_fused()``, then ``forward_features`` under ``no_grad`` and
strict mode; ``FALLBACKS`` must stay empty.  On the GPU: the small cases and resnet50, convnextv2_tiny and swin_tiny
at 224 px, batch 2.  ``--emulated`` installs the CPU providers of ``tests/_*_emul.py`` and runs the small cases only."""
import argparse
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TINY, BASE = (96, 192, 384, 768), (128, 256, 512, 1024)


def images(batch, size, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(batch, 3, size, size, generator=g)
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, size), torch.linspace(-1, 1, size), indexing="ij")
    return x + 2.0 * torch.sin(3.0 * xx) * torch.cos(2.0 * yy)


def line(label, t):
    t = t.detach().cpu().contiguous()
    data = t.view(torch.uint8).numpy().tobytes() if t.numel() else b""
    print(f"{label} {hashlib.sha256(data).hexdigest()} {str(t.dtype)[6:]} {tuple(t.shape)}", flush=True)


def walk(label, node):
    if isinstance(node, torch.Tensor):
        line(label, node)
    elif isinstance(node, dict):
        for key, value in node.items():
            walk(f"{label}[{key!r}]", value)
    elif isinstance(node, (list, tuple)):
        for i, value in enumerate(node):
            walk(f"{label}[{i}]", value)


def small_cases():
    from basd_amd.models.cnn import ResNet
    from basd_amd.models.convnext import ConvNeXtV2
    from basd_amd.models.swin import SwinTransformer
    from tests import _convnext_ref, _resnet_ref, _swin_ref
    heads = {TINY: (3, 6, 12, 24), BASE: (4, 8, 16, 32)}
    for depths, size in (((1, 1, 1, 1), 64), ((2, 1, 1, 1), 72)):
        yield (f"resnet{depths}@{size}", "resnet", lambda d=depths: _resnet_ref.randomise_bn(ResNet(d), seed=7), size)
    for depths, dims in (((1, 1, 2, 1), TINY), ((1, 1, 1, 1), BASE)):
        yield (f"convnext{depths}x{dims[0]}@128", "convnext",
               lambda d=depths, c=dims: _convnext_ref.randomise_affine(ConvNeXtV2(d, c), seed=7), 128)
    for dims in (TINY, BASE):
        yield (f"swin(2, 2, 2, 2)w4x{dims[0]}@128", "swin",
               lambda c=dims: _swin_ref.randomise_affine(SwinTransformer((2, 2, 2, 2), c, heads[c], window_size=4), seed=7), 128)


def frozen_bf16(model, device):
    model = model.to(device).eval()
    for p in model.parameters():
        p.requires_grad = False
    model = model.to(torch.bfloat16)
    for m in model.modules():
        if isinstance(m, torch.nn.LayerNorm):
            m.float()
    return model


def digest(label, model, x):
    import basd_amd.losses._ops as O
    assert model.prepare_fused(), model.fused_refusal()
    O.FALLBACKS.clear()
    O.set_strict(True)
    try:
        with torch.no_grad():
            out = model.forward_features(x)
    finally:
        O.set_strict(False)
    assert not O.FALLBACKS, dict(O.FALLBACKS)
    line(f"{label} out", out)
    walk(f"{label} _fused", model._fused)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--emulated", action="store_true", help="the CPU providers of tests/_*_emul.py, small cases only")
    args = ap.parse_args()
    import basd_amd.losses._ops as O
    if args.emulated:
        from tests import _convnext_emul, _resnet_emul, _swin_emul
        providers = {"resnet": _resnet_emul, "convnext": _convnext_emul, "swin": _swin_emul}
        device = "cpu"
    elif not torch.cuda.is_available():
        raise SystemExit("teacher_trunk_digest.py needs the GPU, or --emulated")
    else:
        providers, device = {}, "cuda"
    for label, family, make, size in small_cases():
        O.set_ops(providers.get(family))
        torch.manual_seed(0)
        model = frozen_bf16(make(), device)
        x = images(2, size, seed=1).to(device).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        digest(label, model, x)
    if args.emulated:
        return
    from basd_amd.models import load_teacher
    from tests import _convnext_ref, _resnet_ref, _swin_ref
    for name, randomise in (("resnet50", _resnet_ref.randomise_bn), ("convnextv2_tiny", _convnext_ref.randomise_affine),
                            ("swin_tiny_patch4_window7_224", _swin_ref.randomise_affine)):
        model = load_teacher(name, 224, device="cuda").model
        randomise(model, seed=9)           # in place on the device parameters: prepare_fused rebuilds the images
        x = images(2, 224, seed=2).cuda().to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        digest(f"{name}@224", model, x)


if __name__ == "__main__":
    main()
