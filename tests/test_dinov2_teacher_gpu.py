"""DINOv2 teachers with register tokens and / or a SwiGLU MLP on the device (GPU box only): frozen bf16 models whose gate
rides in the w12 GEMM's epilogue (basd_gemm_bf16_swiglu) and whose token assembly with registers is one kernel
(basd_vit_embed_reg_bf16).

Three tiny teachers built directly with VisionTransformer (56 px, patch 14, D = 128, 2 heads of 64, depth 2, batch 8):
R = 4 with a GELU MLP; R = 0 with SwiGLU (H = 128); R = 4 with SwiGLU and LayerScale, folded.  They run under strict mode;
their tokens (R + N rows: the reference strips only the CLS row) are compared, layer by layer, with the fp64 forward of
tests/_dinov2_ref.py on the same bf16 weights.  The yardstick is the relative L2 error the PLAIN twin (R = 0, GELU MLP:
code the library had before) reaches against its own fp64 forward in the same test: the new models change where roundings
fall, nothing else, so they may reach at most 1.5 times that (the margin of tests/test_clip_teacher_gpu.py).
"""
import types

import pytest
import torch

from tests._dinov2_ref import dinov2_forward, fp64_params
from tests._teacher_cases import bf16_frozen, images as _images

pytestmark = pytest.mark.gpu

# name -> (register tokens, mlp, LayerScale init)
TEACHERS = {"reg4_gelu": (4, "mlp", None), "swiglu": (0, "swiglu", None), "reg4_swiglu_ls": (4, "swiglu", 0.5)}
IMG, PATCH, DIM, HEADS, DEPTH, BATCH, HIDDEN, N = 56, 14, 128, 2, 2, 8, 128, 16


def _build(reg, mlp, ls, seed=7):
    from basd_amd.models.vit import VisionTransformer
    torch.manual_seed(seed)
    model = VisionTransformer(img_size=IMG, patch_size=PATCH, num_classes=0, embed_dim=DIM, depth=DEPTH, num_heads=HEADS,
                              init_values=ls, reg_tokens=reg, mlp=mlp, mlp_hidden=HIDDEN if mlp == "swiglu" else None)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():                        # norms and scales off their init, visible CLS and register rows
        for name, p in model.named_parameters():
            if "norm" in name or "gamma" in name or name in ("cls_token", "reg_token"):
                p.add_(0.2 * torch.randn(p.shape, generator=g))
    return model


def _teacher(model, reg):
    from basd_amd.models.teacher import TeacherModel, fold_layerscale
    model = model.cuda()
    for p in model.parameters():
        p.requires_grad = False
    fold_layerscale(model)                       # as load_teacher does, before the bf16 cast
    model = bf16_frozen(model)
    return TeacherModel(model=model, embed_dim=DIM, heads_per_layer=[HEADS] * DEPTH, depth=DEPTH, mlp_ratio=0.0,
                        layer_paths=[f"blocks.{i}" for i in range(DEPTH)], attn_subpath="attn", has_cls_token=True,
                        feature_format="token", mean=(0.5,) * 3, std=(0.5,) * 3)


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


_TWIN = {}


def _twin_errors(x):
    """the plain twin (R = 0, GELU MLP) against its own fp64 forward: computed once, shared by the three cases"""
    if "errs" not in _TWIN:
        teacher = _teacher(_build(0, "mlp", None, seed=8), 0)
        toks, _ = _strict_intermediates(teacher, x)
        want_t, _, _ = dinov2_forward(fp64_params(teacher.model.state_dict()), x.to(torch.bfloat16), heads=HEADS)
        _TWIN["errs"] = _rel_l2(toks, want_t)
    return _TWIN["errs"]


@pytest.mark.parametrize("name", sorted(TEACHERS))
def test_tiny_teacher_runs_strict_and_matches_fp64_like_the_plain_twin(name):
    """Measured on an MI355X (rel-L2 per layer, new model / plain twin): DESIGN.md section 22."""
    from basd_amd.models.vit import SwiGLU
    reg, mlp, ls = TEACHERS[name]
    x = _images(BATCH, IMG, seed=3).cuda()
    teacher = _teacher(_build(reg, mlp, ls), reg)
    m = teacher.model
    assert all(isinstance(b.ls2, torch.nn.Identity) for b in m.blocks)
    assert (type(m.blocks[0].mlp) is SwiGLU) == (mlp == "swiglu")
    toks, imps = _strict_intermediates(teacher, x)
    assert len(toks) == DEPTH and len(imps) == DEPTH
    want_t, want_i, want_c = dinov2_forward(fp64_params(m.state_dict()), x.to(torch.bfloat16), heads=HEADS)
    errs, twin = _rel_l2(toks, want_t), _twin_errors(x)
    print(f"dinov2-teacher {name}: rel-L2 vs fp64 per layer: new {[f'{v:.3e}' for v in errs]}, plain twin "
          f"{[f'{v:.3e}' for v in twin]}, ratios {[f'{a / b:.3f}' for a, b in zip(errs, twin)]}")
    for j in range(DEPTH):
        assert toks[j].shape == (BATCH, reg + N, DIM) and imps[j].shape == (BATCH, reg + N)
        assert errs[j] <= 1.5 * twin[j], (j, errs, twin)
        # R + N importances, positive; with the CLS column of the fp64 forward they are one softmax row.  The device
        # row sums to 1 - p_cls of ITS softmax, and p_cls moves by at most p (1 - p) <= 1/4 times the largest logit
        # error: q and k are bf16 (2^-9 relative each) and the CLS row's logits stay below 4 in magnitude here, so
        # 2 * 2^-9 * 4 = 0.016 per logit and 4e-3 on p_cls; 5e-3 with the rounding of the activations in front
        imp = imps[j].double().cpu()
        assert bool((imp > 0).all())
        assert torch.allclose(imp.sum(-1) + want_c[j], torch.ones(BATCH, dtype=torch.float64), rtol=0, atol=5e-3)
        assert torch.allclose(imp, want_i[j], rtol=0.1, atol=1e-3), j
    if mlp == "swiglu":                          # the packed operands were built once, after the bf16 cast
        for blk in m.blocks:
            assert blk.mlp._packed is not None and blk.mlp._packed[1].dtype == torch.bfloat16


def test_fused_gate_and_register_assembly_are_what_ran():
    """the R = 4 SwiGLU model against itself with the dispatch switched off (torch assembly, bias-only w12 GEMM + torch
    gate): the token assembly is bitwise the same, so block 0's input is, and the outputs differ only by the extra bf16
    rounding of w12's output"""
    import basd_amd.models.vit as V
    reg, mlp, ls = TEACHERS["reg4_swiglu_ls"]
    teacher = _teacher(_build(reg, mlp, ls), reg)
    x = _images(BATCH, IMG, seed=3).cuda().to(torch.bfloat16)
    seen = []
    hook = teacher.model.blocks[0].register_forward_pre_hook(lambda mod, inp: seen.append(inp[0]))
    try:
        with torch.no_grad():
            fused = teacher.model.forward_features(x)
            V._FUSED_DINOV2_DISPATCH = False
            try:
                plain = teacher.model.forward_features(x)
            finally:
                V._FUSED_DINOV2_DISPATCH = True
    finally:
        hook.remove()
    assert seen[0].shape == (BATCH, 1 + reg + N, DIM)
    assert torch.equal(seen[0].view(torch.int16), seen[1].view(torch.int16))
    rel = float((fused.float() - plain.float()).norm() / plain.float().norm())
    assert 0.0 < rel < 2e-2, rel


def test_unsupported_hidden_width_is_a_counted_fallback():
    """H = 192 is no multiple of 128: the unfused composition runs and is counted (an error in strict mode)"""
    import basd_amd.losses._ops as O
    from basd_amd.models.vit import SwiGLU
    torch.manual_seed(0)
    mlp = bf16_frozen(SwiGLU(128, 192).cuda())
    x = torch.randn(2, 64, 128, device="cuda", dtype=torch.bfloat16)
    O.FALLBACKS.clear()
    with torch.no_grad():
        y = mlp(x)
        x1, x2 = mlp.w12(x).chunk(2, dim=-1)
        want = mlp.w3(torch.nn.functional.silu(x1) * x2)
    assert O.FALLBACKS["SwiGLU MLP"] == 1 and torch.equal(y, want)
    O.FALLBACKS.clear()
    O.set_strict(True)
    try:
        with pytest.raises(O.StrictModeError), torch.no_grad():
            mlp(x)
    finally:
        O.set_strict(False)
        O.FALLBACKS.clear()


def test_basd_loss_on_the_register_swiglu_teacher_equals_the_oracle():
    """BASDLoss of a tiny DeiT-like student (16 tokens, D_s = 64) against the R = 4 SwiGLU teacher: N_t = 20 != N_s = 16,
    the resample path.  The oracle (fp64) runs on the same extracted tokens and importances; tolerances of
    tests/test_oracle_golden.py for ``tiny_interp``."""
    import basd_amd.losses._ops as O
    from basd_amd.losses import BASDLoss
    from basd_amd.models.vit import VisionTransformer
    from oracle import basd_oracle as OR
    from oracle.synth import token_layers
    reg, mlp, ls = TEACHERS["reg4_swiglu_ls"]
    teacher = _teacher(_build(reg, mlp, ls), reg)
    x = _images(BATCH, IMG, seed=3).cuda()
    t_tok, t_imp = _strict_intermediates(teacher, x)
    d_s, l_s, e, classes = 64, 4, 2, 10
    torch.manual_seed(21)
    student = VisionTransformer(img_size=IMG, patch_size=PATCH, num_classes=classes, embed_dim=d_s, depth=l_s,
                                num_heads=1).cuda().eval()
    layers = token_layers(l_s, e)
    taps = {}
    hooks = [student.blocks[l].register_forward_hook(lambda mod, inp, out, l=l: taps.__setitem__(l, out[:, 1:]))
             for l in layers]
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        logits = student(x).float()
    for h in hooks:
        h.remove()
    assert taps[layers[0]].shape == (BATCH, N, d_s) and t_tok[0].shape == (BATCH, reg + N, DIM)
    targets = torch.arange(BATCH, device="cuda") % classes
    torch.manual_seed(0)
    mod = BASDLoss(torch.nn.CrossEntropyLoss(label_smoothing=1.0 / classes), d_s, DIM, l_s, N,
                   config=types.SimpleNamespace(num_extraction_points=e), teacher_has_cls_token=True).cuda()
    s_tok = {l: taps[l].float().contiguous().requires_grad_(True) for l in layers}
    logits = logits.requires_grad_(True)
    O.FALLBACKS.clear()
    O.set_strict(True)
    try:
        O.get_ops().status_word("cuda").zero_()
        loss = mod(logits, targets, s_tok, t_tok, t_imp)
        loss.backward()
        O.get_ops().check_status()
        torch.cuda.synchronize()
    finally:
        O.set_strict(False)
    assert not O.FALLBACKS, dict(O.FALLBACKS)
    # the oracle takes [B, H, T, T] maps and reads row 0 without column 0: one head whose CLS row is the importance
    attns = {}
    for j, imp in t_imp.items():
        a = torch.zeros(BATCH, 1, 1 + reg + N, 1 + reg + N)
        a[:, 0, 0, 1:] = imp.float().cpu()
        attns[j] = a
    sel = mod.layer_selector
    want = OR.basd_loss(logits.detach().cpu(), targets.cpu(), {l: t.detach().cpu() for l, t in s_tok.items()},
                        {j: t.float().cpu() for j, t in t_tok.items()}, attns, layers=layers, proj_s=sel.proj_s.cpu(),
                        proj_t=sel.proj_t.cpu(), log_temperatures=sel.log_temperatures.detach().cpu(), has_cls=True,
                        smoothing=1.0 / classes, dtype=torch.float64)
    got_geo = mod.last_terms["geo"].cpu().double()
    print(f"dinov2-step: loss {float(loss):.7f} oracle {float(want['loss']):.7f} rel "
          f"{abs(float(loss) - float(want['loss'])) / float(want['loss']):.2e}; geo rel "
          f"{((got_geo - want['geo']).abs() / want['geo'].abs()).tolist()}; weights max abs "
          f"{float((sel.last_weights.cpu().double() - want['weights']).abs().max()):.2e}")
    assert [sel.subspace_ranks[j] for j in range(DEPTH)] == want["ranks"].tolist()
    torch.testing.assert_close(sel.last_weights.cpu().double(), want["weights"].detach(), atol=2e-6, rtol=0)
    torch.testing.assert_close(got_geo, want["geo"].detach(), atol=0, rtol=1e-5)
    torch.testing.assert_close(mod.last_terms["ce"].cpu().double(), want["ce"].detach(), atol=0, rtol=1e-5)
    torch.testing.assert_close(loss.detach().cpu().double(), want["loss"].detach(), atol=0, rtol=1e-5)
    for l in layers:
        assert bool(torch.isfinite(s_tok[l].grad).all())
