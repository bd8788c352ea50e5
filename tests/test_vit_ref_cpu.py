"""The fp64 ViT reference of tests/_vit_ref.py against the model's own stock CPU path in fp64.

The GPU gradient tests (test_student_grads_gpu.py) measure the HIP training path against ``_vit_ref``; this guard pins
the reference itself: same weights, same injected stochastic-depth scales, logits / taps / every parameter gradient
equal to rounding."""
import types

import pytest
import torch

from tests._vit_ref import drop_path_scales, leaf_params, vit_forward


@pytest.fixture
def host_only():
    """a kernel provider that takes no tensor: every module runs its stock torch path"""
    from basd_amd.losses import _ops
    _ops.set_ops(types.SimpleNamespace(handles=lambda t: False))
    yield
    _ops.set_ops(None)


@pytest.mark.parametrize("depth,mlp_ratio,drop", [(2, 4.0, True), (3, 3.0, True), (3, 4.0, False)])
def test_fp64_reference_matches_the_model_cpu_path(host_only, depth, mlp_ratio, drop):
    from basd_amd.models.vit import create_vit
    torch.manual_seed(depth)
    b, taps = 5, (0, depth - 1)
    model = create_vit("deit_tiny_patch16_224", num_classes=7, img_size=32, patch_size=8, embed_dim=48, num_heads=3,
                       depth=depth, mlp_ratio=mlp_ratio, drop_path_rate=0.2).double().train()
    with torch.no_grad():                     # non-trivial LayerNorm affine parameters and CLS token
        for name, p in model.named_parameters():
            if "norm" in name or name == "cls_token":
                p.add_(0.1 * torch.randn_like(p))
    for blk in model.blocks:                  # every branch of every block may drop (the stock schedule spares block 0)
        blk.drop_path1.p = blk.drop_path2.p = 0.2
    g = torch.Generator().manual_seed(17)
    scales = drop_path_scales(depth, b, 0.8, g) if drop else torch.ones(2 * depth, b)
    model._draw_drop_path_masks = lambda x: (scales.to(x.dtype).view(2 * depth, b, 1, 1), scales)
    x = torch.randn(b, 3, 32, 32, generator=g, dtype=torch.float64)
    g_logits = torch.randn(b, 7, generator=g, dtype=torch.float64)
    g_taps = {i: torch.randn(b, 16, 48, generator=g, dtype=torch.float64) for i in taps}

    captured = {}
    hooks = [model.blocks[i].register_forward_hook(lambda m, inp, out, i=i: captured.__setitem__(i, out[:, 1:]))
             for i in taps]
    logits = model(x)
    for h in hooks:
        h.remove()
    (logits * g_logits).sum().add(sum((captured[i] * g_taps[i]).sum() for i in taps)).backward()

    params = leaf_params(model.state_dict())
    ref_logits, ref_taps = vit_forward(params, x, heads=3, scales=scales, taps=taps)
    (ref_logits * g_logits).sum().add(sum((ref_taps[i] * g_taps[i]).sum() for i in taps)).backward()

    torch.testing.assert_close(logits, ref_logits, rtol=1e-10, atol=1e-12)
    for i in taps:
        torch.testing.assert_close(captured[i], ref_taps[i], rtol=1e-10, atol=1e-12)
    for name, p in model.named_parameters():
        want = params[name].grad
        err = float((p.grad - want).norm() / want.norm())
        assert err < 1e-10, (name, err)
