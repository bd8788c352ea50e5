"""Student ViT training path on the HIP kernels against the fp64 reference of tests/_vit_ref.py, one tensor at a time.

Run as the trainer runs it: fp32 master weights on the device, ``train()``, forward under bf16 autocast, forward hooks
at the four extraction blocks.  The upstream signal is fixed: sum <logits, G> + sum_l <tap_l, G_l> with random fp32
G's, so gradient enters mid-network the way the BASD loss's does.  The fp64 reference runs on the same fp32 master
weights, images and stochastic-depth scales (injected in place of ``_draw_drop_path_masks``).

Every named parameter's gradient gets its own rel-L2 bound: a flat cosine over the whole gradient stays above 0.998
with the gradient of a LayerNorm, a bias, cls_token or pos_embed missing entirely.  Head dim 64 and T <= 224
throughout: the student attention stays on the own backward kernel.
"""
import pytest
import torch

from tests._vit_ref import drop_path_scales, leaf_params, vit_forward

pytestmark = pytest.mark.gpu

# key -> (preset, image size, patch, batch, create_vit overrides); batches leave ragged row tails (B * T % 64)
MODELS = {
    "c1": ("deit_tiny_patch16_224", 32, 4, 23, {}),                          # T = 65, 48-value patches padded to 64
    "tiny224": ("deit_tiny_patch16_224", 224, 16, 6, {}),                    # T = 197, B T % 64 = 30
    "small224": ("deit_small_patch16_224", 224, 16, 3, {}),                  # D = 384, B T % 64 = 15
    "base224_d4": ("vit_base_patch16_224", 224, 16, 3, {"depth": 4}),        # D = 768
    "tiny_mlp3": ("deit_tiny_patch16_224", 32, 4, 19, {"mlp_ratio": 3.0}),   # hidden 576: two-stage fused MLP
}
KEEP = 0.8              # per-branch keep probability of the drop-path modes: scales 0 or 1.25 (exact in bf16)

# rel-L2 bounds per parameter class: about 3x the worst value measured on the MI355X over seeds 0-2 of every case below
# (all near 1e-2: bf16 activations).  A missing or misrouted gradient shows up as 0.1 - 1.
BOUNDS = {
    "weight": 3.6e-2,   # qkv / proj / fc1 / fc2 / head weights; measured 1.21e-2 (head.weight, c1 fused)
    "bias": 3.3e-2,     # their biases; measured 1.08e-2 (blocks.0.attn.qkv.bias, tiny224 fused)
    "ln": 4.0e-2,       # LayerNorm gamma / beta (norm1, norm2, final norm); measured 1.32e-2 (norm.weight, c1 fused)
    "cls_pos": 4.0e-2,  # cls_token, pos_embed; measured 1.34e-2 (cls_token, tiny224 fused)
    "patch": 2.9e-2,    # patch_embed.proj weight / bias; measured 9.6e-3 (bias, tiny224 fused)
    "logits": 4.5e-2,   # worst per-sample relative error of the logits; measured 1.47e-2 (tiny_mlp3 fused_dp)
    "taps": 3.0e-2,     # worst per-sample relative error of the tapped block outputs; measured 1.00e-2 (c1 fused)
}


def param_class(name: str) -> str:
    if name.startswith("patch_embed."):
        return "patch"
    if name in ("cls_token", "pos_embed"):
        return "cls_pos"
    if "norm" in name:
        return "ln"
    return "bias" if name.endswith(".bias") else "weight"


def _per_sample(got, want):
    got, want = got.double().flatten(1), want.double().flatten(1)
    return float(((got - want).norm(dim=1) / want.norm(dim=1)).max())


def run_case(key, mode, seed=0, device="cuda"):
    """-> ({parameter name: rel-L2 error of its gradient}, {"logits" | "taps": worst per-sample error}, {name: grad}).
    ``mode``: "fused" / "fused_dp" (the default trained-block path), "ckpt" / "ckpt_dp" (activation checkpointing),
    "unfused_dp" (``fuse_training`` cleared, no checkpointing)"""
    import basd_amd.losses._ops as O
    from basd_amd.models.vit import create_vit
    preset, img, patch, b, over = MODELS[key]
    dp = mode.endswith("_dp")
    torch.manual_seed(seed)
    model = create_vit(preset, num_classes=100, img_size=img, patch_size=patch, drop_path_rate=0.1 if dp else 0.0,
                       **over).to(device).train()
    with torch.no_grad():          # non-trivial LayerNorm affine parameters and CLS token
        for name, p in model.named_parameters():
            if "norm" in name or name == "cls_token":
                p.add_(0.1 * torch.randn_like(p))
    depth, heads = len(model.blocks), model.blocks[0].attn.num_heads
    assert model.blocks[0].attn.head_dim == 64
    if mode.startswith("ckpt"):
        model.set_grad_checkpointing(True)
    elif mode.startswith("unfused"):
        for blk in model.blocks:
            blk.fuse_training = False
    g = torch.Generator().manual_seed(1000 + seed)
    scales = None
    if dp:
        for blk in model.blocks:   # every branch may drop (the stock schedule spares block 0)
            blk.drop_path1.p = blk.drop_path2.p = 1.0 - KEEP
        scales = drop_path_scales(depth, b, KEEP, g).to(device)
        model._draw_drop_path_masks = lambda x: (scales.to(x.dtype).view(2 * depth, b, 1, 1), scales)
    taps = [round(i * (depth - 1) / 3) for i in range(4)]
    x = torch.randn(b, 3, img, img, generator=g).to(device)
    t = model.pos_embed.shape[1]
    g_logits = torch.randn(b, 100, generator=g).to(device)
    g_taps = {i: torch.randn(b, t - 1, model.embed_dim, generator=g).to(device) for i in taps}

    captured = {}
    hooks = [model.blocks[i].register_forward_hook(lambda m, inp, out, i=i: captured.__setitem__(i, out[:, 1:]))
             for i in taps]
    O.FALLBACKS.clear()
    try:
        with torch.autocast(device, dtype=torch.bfloat16):
            logits = model(x)
        out = {i: captured[i] for i in taps}
        signal = (logits.float() * g_logits).sum() + sum((out[i].float() * g_taps[i]).sum() for i in taps)
        signal.backward()
    finally:
        for h in hooks:
            h.remove()
    if device == "cuda":
        torch.cuda.synchronize()
    assert not O.FALLBACKS, dict(O.FALLBACKS)

    params = leaf_params(model.state_dict(), device)
    ref_logits, ref_taps = vit_forward(params, x, heads=heads, scales=scales, taps=taps)
    ref_signal = (ref_logits * g_logits.double()).sum() + sum((ref_taps[i] * g_taps[i].double()).sum() for i in taps)
    ref_signal.backward()
    outs = {"logits": _per_sample(logits.detach(), ref_logits.detach()),
            "taps": max(_per_sample(out[i].detach(), ref_taps[i].detach()) for i in taps)}
    errs, grads = {}, {}
    for name, p in model.named_parameters():
        want = params[name].grad
        assert p.grad is not None and p.grad.shape == want.shape, name
        errs[name] = float((p.grad.double() - want).norm() / want.norm())
        grads[name] = p.grad.detach().clone()
    return errs, outs, grads


CASES = [("c1", "fused"), ("c1", "fused_dp"), ("c1", "ckpt"), ("c1", "ckpt_dp"),
         ("tiny224", "fused"), ("tiny224", "fused_dp"), ("tiny224", "ckpt_dp"),
         ("small224", "fused_dp"), ("base224_d4", "fused_dp"), ("base224_d4", "ckpt"), ("tiny_mlp3", "fused_dp")]


@pytest.mark.parametrize("key,mode", CASES)
def test_student_gradients_match_fp64_per_tensor(key, mode):
    errs, outs, _ = run_case(key, mode)
    worst = {}
    for name, e in errs.items():
        c = param_class(name)
        if e > worst.get(c, (0.0, ""))[0]:
            worst[c] = (e, name)
    print(f"{key}/{mode}: outputs {outs}; worst per class {worst}")
    for k, e in outs.items():
        assert e < BOUNDS[k], (k, e)
    bad = {name: e for name, e in errs.items() if not e < BOUNDS[param_class(name)]}
    assert not bad, bad


@pytest.mark.parametrize("key", ["c1", "tiny224"])
def test_checkpointing_does_not_change_the_arithmetic(key):
    """activation checkpointing recomputes each block's forward inside the backward; with ``fuse_training`` cleared the
    plain step runs the same kernels on the same values, so every gradient agrees up to the accumulation order of the
    weight-gradient kernels' fp32 atomics (not bitwise: measured <= 2e-7 per tensor)"""
    _, _, plain = run_case(key, "unfused_dp")
    _, _, ckpt = run_case(key, "ckpt_dp")
    assert sorted(plain) == sorted(ckpt)
    diff = {name: float((plain[name] - ckpt[name]).norm() / plain[name].norm()) for name in plain}
    worst = max(diff, key=diff.get)
    print(f"{key}: checkpointed vs plain, worst per-tensor rel-L2 {diff[worst]:.2e} ({worst})")
    assert diff[worst] < 1e-5, (worst, diff[worst])
