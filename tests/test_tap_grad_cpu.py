"""Token taps of the student without a GPU: the hooked ``_extract_student`` keeps the plain slice (and its gradients)
where the fused tap does not apply, the tap function's own backward equals autograd's around the slice, the fused
pre-norm attribute survives the hook, and the ``*_supported`` predicates draw the dispatch lines."""
import pytest
import torch

from basd_amd.models.vit import VisionTransformer
from basd_amd.training.trainer import _TokenTapFn, _extract_student, _fused_tap_ok


def _tiny_vit():
    torch.manual_seed(0)
    # depth 2, width 64, 2 x 2 patches + CLS: T = 5
    return VisionTransformer(img_size=8, patch_size=4, in_chans=3, num_classes=7, embed_dim=64, depth=2, num_heads=2)


def _paths(model):
    return [f"blocks.{i}" for i in range(len(model.blocks))]


def _loss(logits, toks):
    w = torch.linspace(-1.0, 1.0, toks[0].shape[-1])
    return logits.square().sum() + sum(((i + 2) * t * w).sum() + t.square().sum() for i, t in enumerate(toks))


def test_hooked_extract_equals_the_plain_slice_in_fp32():
    model = _tiny_vit().train()
    x = torch.randn(3, 3, 8, 8, requires_grad=True)
    logits, taps = _extract_student(model, x, [0, 1], layer_paths=_paths(model), has_cls_token=True)
    assert sorted(taps) == [0, 1] and all(t.shape == (3, 4, 64) for t in taps.values())
    _loss(logits, [taps[0], taps[1]]).backward()
    got = [x.grad.clone()] + [p.grad.clone() for p in model.parameters()]

    x.grad = None
    model.zero_grad(set_to_none=True)
    outs = {}
    # the slice is taken inside the hook, as the plain tap takes it: autograd sums an output's gradients in the order
    # its consumers were recorded
    hooks = [model.blocks[i].register_forward_hook(lambda m, inp, out, i=i: outs.__setitem__(i, out[:, 1:, :]))
             for i in (0, 1)]
    try:
        logits2 = model(x)
    finally:
        for h in hooks:
            h.remove()
    _loss(logits2, [outs[0], outs[1]]).backward()
    want = [x.grad] + [p.grad for p in model.parameters()]
    assert torch.equal(logits, logits2)
    for g, w in zip(got, want):
        assert torch.equal(g, w)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("use", ["both", "tokens", "output"])
def test_tap_function_backward_equals_autograd_around_the_slice(offset, use):
    torch.manual_seed(1)
    a = torch.randn(2, 5, 64, requires_grad=True)
    b = a.detach().clone().requires_grad_(True)
    wo, wt = torch.randn(2, 5, 64), torch.randn(2, 5 - offset, 64)

    def total(out, tok):
        return (out * wo).sum() * (use != "tokens") + (tok * wt).sum() * (use != "output")

    out, tok = _TokenTapFn.apply(a * 1.0, offset)
    assert out.shape == a.shape and tok.shape == (2, 5 - offset, 64)
    total(out, tok).backward()
    plain = b * 1.0
    total(plain, plain[:, offset:, :]).backward()
    assert torch.equal(a.grad, b.grad)


def test_prenorm_attribute_survives_the_hook(monkeypatch):
    """the replaced block output carries the (norm, tensor) pair the next block's norm1 looks up by identity"""
    import basd_amd.training.trainer as T
    model = _tiny_vit().train()
    marker = (torch.nn.LayerNorm(64), torch.zeros(1))      # not block 1's own norm: carried along, never consumed
    seen = {}

    def tag(mod, inp, out):            # registered first: runs before the tap hook, as Block.forward's attribute would
        out._basd_prenorm = marker
        return out
    h0 = model.blocks[0].register_forward_hook(tag)
    h1 = model.blocks[1].register_forward_pre_hook(lambda m, inp: seen.__setitem__("x", inp[0]))
    monkeypatch.setattr(T, "_fused_tap_ok", lambda model_, block, out: True)
    try:
        x = torch.randn(2, 3, 8, 8, requires_grad=True)
        logits, taps = _extract_student(model, x, [0], layer_paths=_paths(model), has_cls_token=True)
    finally:
        h0.remove()
        h1.remove()
    assert taps[0].shape == (2, 4, 64) and taps[0].grad_fn is not None
    assert type(taps[0].grad_fn.next_functions[0][0]).__name__.startswith("_TokenTapFn")      # behind its own view node
    assert getattr(seen["x"], "_basd_prenorm", None) is marker      # block 1 received the replaced tensor, tagged
    (logits.sum() + taps[0].sum()).backward()
    assert x.grad is not None and torch.isfinite(x.grad).all()


def test_two_stage_backward_through_the_tap_function(monkeypatch):
    """the backward cut of the data-parallel path: stage 1 differentiates down to the output of the block in front of
    the cut and to the taps below it, stage 2 continues from those; the blocks between a tap and the cut must run in
    stage 2 only, and the sum must equal the one-pass backward"""
    import basd_amd.training.trainer as T
    torch.manual_seed(0)
    model = VisionTransformer(img_size=8, patch_size=4, in_chans=3, num_classes=7, embed_dim=64, depth=4,
                              num_heads=2).train()
    x = torch.randn(2, 3, 8, 8)
    params = list(model.parameters())

    def forward():
        holder = {}
        h = model.blocks[1].register_forward_hook(lambda m, i, o: holder.__setitem__("out", o))     # cut = 2
        try:
            logits, taps = _extract_student(model, x, [0, 2], layer_paths=_paths(model), has_cls_token=True)
        finally:
            h.remove()
        return _loss(logits, [taps[0], taps[2]]), [holder["out"], taps[0]]

    monkeypatch.setattr(T, "_fused_tap_ok", lambda model_, block, out: True)
    loss, _ = forward()
    want = torch.autograd.grad(loss, params, allow_unused=True)
    loss, iface = forward()
    late = [q for n, q in model.named_parameters() if n.startswith(("blocks.2.", "blocks.3.", "norm.", "head."))]
    early = [q for q in params if all(q is not l for l in late)]
    g1 = torch.autograd.grad(loss, late + iface, allow_unused=True)
    for q in params:
        q.grad = None
    torch.autograd.backward(iface, list(g1[len(late):]))        # raises if stage 1 already ran (and freed) these blocks
    got = dict(zip(map(id, late), g1[:len(late)]))
    got.update({id(q): q.grad for q in early})
    for q, w in zip(params, want):
        g = got[id(q)]
        assert (g is None) == (w is None)
        if w is not None:
            torch.testing.assert_close(g, w, rtol=1e-5, atol=1e-6)


def test_plain_slice_stays_on_the_cpu_and_under_checkpointing():
    model = _tiny_vit().train()
    out = torch.randn(2, 5, 64, requires_grad=True)
    assert not _fused_tap_ok(model, model.blocks[0], out)                          # fp32 on the CPU
    assert not _fused_tap_ok(model, model.blocks[0], out.bfloat16())               # bf16, but not on the device
    with torch.no_grad():
        assert not _fused_tap_ok(model, model.blocks[0], out.bfloat16())


def test_supported_predicates():
    import basd_amd._native as native
    for d in (192, 384, 768):
        assert native.selector_token_grad_supported(d) and native.tap_grad_scatter_supported(d)
    for d in (200, 64 * 13, 0):
        assert not native.selector_token_grad_supported(d)
    for d in (200, 0, -64):
        assert not native.tap_grad_scatter_supported(d)
    assert native.tap_grad_scatter_supported(64 * 13)        # the scatter takes every multiple of 64
