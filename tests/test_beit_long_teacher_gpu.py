"""A BEiT teacher past 272 tokens on the device (GPU box only): the tiny frozen bf16 model at 68 px with patch 4 (a
17 x 17 grid, 290 tokens -- the first square grid the short kernel refuses) under strict mode, through the tap
machinery and one trainer step, on basd_attention_fwd_long_relbias_bf16.

The yardstick is measured in the same test, as in tests/test_beit_teacher_gpu.py: the plain-ViT twin of the model (same
folded weights, zero position embedding, no table, the existing tiled kernel) against its own fp64 forward.  The new
code adds one fp32 add per logit, so it may reach at most 1.5 times that error.
"""
import os

import pytest
import torch

from tests._beit_long_cases import DEPTH, DIM, HEADS, tiny_beit_at
from tests._beit_ref import beit_forward, fp64_params
from tests._teacher_cases import bf16_frozen, images as _images

pytestmark = pytest.mark.gpu

CFG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                   "vit-bias-aware-structural-distillation_amd", "configs", "config.yaml")
IMG, PATCH = 68, 4
GRID = (IMG // PATCH, IMG // PATCH)
TOKENS = GRID[0] * GRID[1] + 1
FACTOR = 1.5


def _frozen(model):
    """what load_teacher does to a Beit: qkv bias materialised, LayerScale folded, bf16 with fp32 norms and table"""
    from basd_amd.models.teacher import fold_layerscale
    model.materialize_qkv_bias()
    for p in model.parameters():
        p.requires_grad = False
    assert fold_layerscale(model) == 2 * DEPTH
    return bf16_frozen(model.cuda())


def _twin_of(model):
    """the plain ViT with the same (folded, bf16) weights, a zero position embedding and no bias table"""
    from basd_amd.models.vit import VisionTransformer
    twin = VisionTransformer(img_size=IMG, patch_size=PATCH, num_classes=0, embed_dim=DIM, depth=DEPTH, num_heads=HEADS)
    missing, unexpected = twin.load_state_dict(model.state_dict(), strict=False)
    assert missing == ["pos_embed"], missing
    assert all(k.endswith(("q_bias", "v_bias", "relative_position_bias_table")) for k in unexpected), unexpected
    with torch.no_grad():
        twin.pos_embed.zero_()
    for p in twin.parameters():
        p.requires_grad = False
    return bf16_frozen(twin.cuda())


def _teacher(model):
    from basd_amd.models.teacher import TeacherModel
    return TeacherModel(model=model, embed_dim=DIM, heads_per_layer=[HEADS] * DEPTH, depth=DEPTH, mlp_ratio=4.0,
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


def test_tiny_teacher_runs_strict_on_the_long_kernel_and_matches_fp64_like_the_plain_twin(monkeypatch):
    """Measured on an MI355X (rel-L2 per layer, BEiT / plain twin): DESIGN.md section 25."""
    import basd_amd._native as native
    calls = []
    real = native.attention_fwd_long_relbias

    def spy(qkv, table, gh, gw, heads, head_dim, scale, want_importance=False):
        calls.append(("long", tuple(qkv.shape), (gh, gw), table.dtype, want_importance))
        return real(qkv, table, gh, gw, heads, head_dim, scale, want_importance)

    def short_spy(*args, **kwargs):
        calls.append(("short",))
        raise AssertionError("the short entry refuses 290 tokens")

    monkeypatch.setattr(native, "attention_fwd_long_relbias", spy)
    monkeypatch.setattr(native, "attention_fwd_relbias", short_spy)
    batch = 3
    model = _frozen(tiny_beit_at(IMG, PATCH))
    assert model.blocks[0].attn.relative_position_bias_table.dtype == torch.float32
    assert model.blocks[0].attn.qkv.weight.dtype == torch.bfloat16
    twin = _twin_of(model)
    x = _images(batch, IMG, seed=3).cuda()
    errs = {}
    for label, m in (("beit", model), ("twin", twin)):
        toks, imps = _strict_intermediates(_teacher(m), x)
        assert len(toks) == DEPTH and toks[0].shape == (batch, TOKENS - 1, DIM)
        assert imps[DEPTH - 1].shape == (batch, TOKENS - 1)
        want_t, want_i = beit_forward(fp64_params(m.state_dict()), x.to(torch.bfloat16), heads=HEADS)
        errs[label] = _rel_l2(toks, want_t)
        if label == "beit":
            assert calls == [("long", (batch, TOKENS, 3 * DIM), GRID, torch.float32, True)] * DEPTH, calls
            for j in range(DEPTH):      # bf16 activations in front of the softmax: a loose, sound bound
                assert torch.allclose(imps[j].double().cpu(), want_i[j], rtol=0.1, atol=1e-3), j
    assert len(calls) == DEPTH                       # the twin ran the existing kernel
    print(f"beit-long-teacher: rel-L2 vs fp64 per layer: beit {[f'{v:.3e}' for v in errs['beit']]}, "
          f"plain twin {[f'{v:.3e}' for v in errs['twin']]}")
    for j in range(DEPTH):
        assert errs["beit"][j] <= FACTOR * errs["twin"][j], (j, errs)


def test_library_path_is_a_counted_fallback_and_agrees():
    """the switch of scripts/time_beit_teacher.py: dense bias + SDPA + separate tap, counted, refused in strict mode"""
    import basd_amd.losses._ops as O
    import basd_amd.models.beit as B
    from basd_amd.models.teacher import extract_intermediates
    teacher = _teacher(_frozen(tiny_beit_at(IMG, PATCH)))
    x = _images(3, IMG, seed=3).cuda()
    toks, imps = _strict_intermediates(teacher, x)
    B._FUSED_RELBIAS_ATTENTION = False
    try:
        O.FALLBACKS.clear()
        lib_toks, lib_imps = extract_intermediates(teacher, x)
        assert O.FALLBACKS["attention (relative bias)"] == DEPTH
        O.set_strict(True)
        with pytest.raises(O.StrictModeError):
            extract_intermediates(teacher, x)
    finally:
        O.set_strict(False)
        B._FUSED_RELBIAS_ATTENTION = True
        O.FALLBACKS.clear()
    for j in range(DEPTH):
        rel = float((toks[j].float() - lib_toks[j].float()).norm() / lib_toks[j].float().norm())
        assert rel < 2e-2, (j, rel)                  # two bf16 pipelines (tests/test_beit_teacher_gpu.py's bound)


def test_one_eager_trainer_step_against_the_tiny_long_beit_teacher():
    import basd_amd.losses._ops as O
    from basd_amd.config import load_config
    from basd_amd.models.teacher import probe_model
    from basd_amd.train import SyntheticLoader, _create_student
    from basd_amd.training.trainer import Trainer
    batch = 8
    teacher = _teacher(_frozen(tiny_beit_at(IMG, PATCH)))
    torch.manual_seed(0)
    cfg = load_config(CFG, None, [f"data.batch_size={batch}", "data.dataset=synthetic", f"model.vit.img_size={IMG}",
                                  f"model.vit.patch_size={PATCH}", "model.drop_path_rate=0.0",
                                  "model.student_preset=deit_tiny_patch16_224"])
    student = _create_student("deit_tiny_patch16_224", num_classes=cfg.model.num_classes, drop_path_rate=0.0,
                              img_size=IMG, arch_overrides={"depth": 4}, patch_size=PATCH, device="cuda")
    trainer = Trainer(student, cfg, accelerator=None, teacher=teacher, student_info=probe_model(student, IMG))
    trainer.use_mixup = False
    trainer.optimizer.train()
    trainer.model.train()
    b = next(iter(SyntheticLoader(batch, IMG, cfg.model.num_classes, 1, "cuda", seed=5)))
    O.FALLBACKS.clear()
    loss, _ = trainer.train_step(b)
    trainer.check_health()
    torch.cuda.synchronize()
    assert torch.isfinite(loss.detach()).all()
    # the gradients live in the optimizer's flat buffer (every p.grad is a view of it); the step has consumed them, so a
    # non-finite gradient would also show in the updated weights
    grads = [p.grad for p in student.parameters() if p.grad is not None]
    assert grads and all(bool(torch.isfinite(g).all()) for g in grads)
    assert all(bool(torch.isfinite(p.detach()).all()) for p in student.parameters())
    assert not O.FALLBACKS, dict(O.FALLBACKS)
