"""Rotary teachers on the device past and below the short attention kernel's 272 tokens (GPU box only): the tiny frozen
bf16 DINOv3 teacher at 64 px (21 tokens: basd_attention_fwd_rope_bf16) and at 272 px (17 x 17 + 5 = 294 tokens:
basd_attention_fwd_long_rope_bf16), and the tiny EVA-02 teacher at 238 px (17 x 17 + 1 = 290 tokens), under strict mode,
through the tap machinery and a graph capture.

The reference is the fp64 forward of tests/_dinov3_ref.py in DINOv3's own form (tests/_eva_ref.py for EVA-02); the
yardstick is the library path of the same model (``_FUSED_EVA_DISPATCH`` off: torch rotation + SDPA + separate tap),
measured in the same test: the own path may reach 1.5 times its error per layer, the margin of
tests/test_eva_teacher_gpu.py.
"""
import pytest
import torch

from tests._dinov3_ref import (BATCH, DEPTH, DIM, HD, HEADS, PATCH, REG, bf16_exact, dinov3_forward, fp64_params,
                               hub_state_dict, tiny_dinov3)
from tests._teacher_cases import bf16_frozen, images as _images

pytestmark = pytest.mark.gpu

FACTOR = 1.5


def _teacher(model, dim, heads):
    from basd_amd.models.teacher import TeacherModel
    return TeacherModel(model=model, embed_dim=dim, heads_per_layer=[heads] * DEPTH, depth=DEPTH, mlp_ratio=0.0,
                        layer_paths=[f"blocks.{i}" for i in range(DEPTH)], attn_subpath="attn", has_cls_token=True,
                        feature_format="token", mean=(0.5,) * 3, std=(0.5,) * 3)


def _frozen_dinov3(img):
    """what load_teacher does to a Dinov3: checkpoint loaded and permuted, LayerScale folded, bf16 with fp32 norms and
    table -> (model, the checkpoint in hub names)"""
    from basd_amd.models.teacher import fold_layerscale
    state = bf16_exact(hub_state_dict())
    model = tiny_dinov3(img, state)
    for p in model.parameters():
        p.requires_grad = False
    assert fold_layerscale(model) == 2 * DEPTH
    return bf16_frozen(model.cuda()), state


def _strict_intermediates(teacher, x):
    import basd_amd.losses._ops as O
    from basd_amd.models.teacher import extract_intermediates
    O.FALLBACKS.clear()
    O.set_strict(True)
    try:
        with torch.no_grad(), O.record_library_gemms() as seen:
            toks, imps = extract_intermediates(teacher, x)
        torch.cuda.synchronize()
    finally:
        O.set_strict(False)
    assert not O.FALLBACKS and not seen, (dict(O.FALLBACKS), seen)
    return toks, imps


def _rel_l2(toks, want):
    return [float((toks[j].double().cpu() - want[j][:, 1:]).norm() / want[j][:, 1:].norm()) for j in range(DEPTH)]


def _spies(monkeypatch):
    """-> the list both rotary entries append (name, qkv shape, table shape, heads, want_importance) to"""
    import basd_amd._native as native
    calls = []
    for name in ("attention_fwd_rope", "attention_fwd_long_rope"):
        real = getattr(native, name)

        def spy(qkv, rope, heads, head_dim, scale, want_importance=False, _real=real, _name=name):
            calls.append((_name, tuple(qkv.shape), tuple(rope.shape), rope.dtype, heads, want_importance))
            return _real(qkv, rope, heads, head_dim, scale, want_importance)

        monkeypatch.setattr(native, name, spy)
    return calls


def _own_against_library(monkeypatch, model, dim, heads, x, want_t, want_i, entry, t, label):
    """strict own path through ``entry``, then the library path of the same model; both against the fp64 reference"""
    import basd_amd.losses._ops as O
    import basd_amd.models.eva as E
    from basd_amd.models.teacher import extract_intermediates
    calls = _spies(monkeypatch)
    toks, imps = _strict_intermediates(_teacher(model, dim, heads), x)
    assert calls == [(entry, (x.shape[0], t, 3 * dim), (t, HD // 2, 2), torch.float32, heads, True)] * DEPTH, calls
    assert len(toks) == DEPTH and toks[0].shape == (x.shape[0], t - 1, dim) and imps[DEPTH - 1].shape == (x.shape[0], t - 1)
    own = _rel_l2(toks, want_t)
    for j in range(DEPTH):              # bf16 activations in front of the softmax: the bound of the EVA / BEiT tests
        assert torch.allclose(imps[j].double().cpu(), want_i[j], rtol=0.1, atol=1e-3), j
    monkeypatch.setattr(E, "_FUSED_EVA_DISPATCH", False)
    O.FALLBACKS.clear()
    try:
        lib_toks, lib_imps = extract_intermediates(_teacher(model, dim, heads), x)
        torch.cuda.synchronize()
        assert O.FALLBACKS["attention (rope)"] == DEPTH, dict(O.FALLBACKS)
        O.set_strict(True)
        with pytest.raises(O.StrictModeError):
            extract_intermediates(_teacher(model, dim, heads), x)
    finally:
        O.set_strict(False)
        O.FALLBACKS.clear()
    assert len(calls) == DEPTH                       # the library path did not reach the kernels
    lib = _rel_l2(lib_toks, want_t)
    print(f"{label}: rel-L2 vs fp64 per layer: own {[f'{v:.3e}' for v in own]}, library {[f'{v:.3e}' for v in lib]}")
    for j in range(DEPTH):
        assert own[j] <= FACTOR * lib[j], (j, own, lib)
        assert torch.allclose(lib_imps[j].double().cpu(), want_i[j], rtol=0.1, atol=1e-3), j


@pytest.mark.parametrize("img,entry", [(64, "attention_fwd_rope"), (272, "attention_fwd_long_rope")])
def test_tiny_dinov3_runs_strict_on_both_entries_and_matches_fp64_like_the_library_path(monkeypatch, img, entry):
    """Measured on an MI355X (rel-L2 per layer, own path / library path): DESIGN.md section 24."""
    model, state = _frozen_dinov3(img)
    assert model.blocks[0].attn.rope.dtype == torch.float32 and model.blocks[0].attn.qkv.weight.dtype == torch.bfloat16
    x = _images(BATCH, img, seed=3).cuda()
    want_t, want_i = dinov3_forward(fp64_params(state), x.to(torch.bfloat16))
    t = (img // PATCH) ** 2 + 1 + REG
    _own_against_library(monkeypatch, model, DIM, HEADS, x, want_t, want_i, entry, t, f"dinov3-teacher {img} px")


def _tiny_eva(img):
    """tests/_eva_ref.tiny_eva (sub-LN variant) at another input size"""
    from basd_amd.models.eva import Eva
    from tests._eva_ref import DIM as D, HEADS as H, HIDDEN, PATCH as P, REF_GRID
    torch.manual_seed(7)
    model = Eva(img_size=img, patch_size=P, num_classes=0, embed_dim=D, depth=DEPTH, num_heads=H, mlp_hidden=HIDDEN,
                scale_mlp=True, ref_grid=REF_GRID)
    g = torch.Generator().manual_seed(8)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if "norm" in name or name == "cls_token":
                p.add_(0.2 * torch.randn(p.shape, generator=g))
            elif name.endswith("q_bias") or name.endswith("v_bias"):
                p.copy_(0.3 * torch.randn(p.shape, generator=g))
    model.materialize_qkv_bias()
    return bf16_frozen(model.eval().cuda())


def test_tiny_eva_at_290_tokens_runs_strict_on_the_long_entry(monkeypatch):
    """EVA-02 /14 past 272 tokens: today every block counts an "attention (rope)" fallback"""
    from tests._eva_ref import DIM as D, HEADS as H, eva_forward, fp64_params as eva_params
    img = 238
    model = _tiny_eva(img)
    x = _images(BATCH, img, seed=5).cuda()
    want_t, want_i = eva_forward(eva_params(model.state_dict()), x.to(torch.bfloat16), heads=H)
    _own_against_library_eva(monkeypatch, model, D, H, x, want_t, want_i)


def _own_against_library_eva(monkeypatch, model, dim, heads, x, want_t, want_i):
    """as ``_own_against_library``; the library path of an Eva also counts its unfused MLP"""
    import basd_amd.losses._ops as O
    import basd_amd.models.eva as E
    from basd_amd.models.teacher import extract_intermediates
    t = 17 * 17 + 1
    calls = _spies(monkeypatch)
    toks, imps = _strict_intermediates(_teacher(model, dim, heads), x)
    assert calls == [("attention_fwd_long_rope", (x.shape[0], t, 3 * dim), (t, HD // 2, 2), torch.float32, heads,
                      True)] * DEPTH, calls
    own = _rel_l2(toks, want_t)
    for j in range(DEPTH):
        assert torch.allclose(imps[j].double().cpu(), want_i[j], rtol=0.1, atol=1e-3), j
    monkeypatch.setattr(E, "_FUSED_EVA_DISPATCH", False)
    O.FALLBACKS.clear()
    try:
        lib_toks, _ = extract_intermediates(_teacher(model, dim, heads), x)
        torch.cuda.synchronize()
        assert O.FALLBACKS["attention (rope)"] == DEPTH, dict(O.FALLBACKS)
    finally:
        O.FALLBACKS.clear()
    lib = _rel_l2(lib_toks, want_t)
    print(f"eva-teacher 238 px: rel-L2 vs fp64 per layer: own {[f'{v:.3e}' for v in own]}, "
          f"library {[f'{v:.3e}' for v in lib]}")
    for j in range(DEPTH):
        assert own[j] <= FACTOR * lib[j], (j, own, lib)


def test_one_forward_under_graph_capture_replays_to_the_eager_result():
    model, _ = _frozen_dinov3(272)
    x = _images(BATCH, 272, seed=4).cuda().to(torch.bfloat16)
    with torch.no_grad():
        eager = model.forward_features(x).clone()   # also loads the code objects
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            model.forward_features(x)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = model.forward_features(x)
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(captured.view(torch.int16), eager.view(torch.int16))
