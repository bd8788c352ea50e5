"""BEiT teachers on the device (GPU box only): basd_attention_fwd_relbias_bf16 against fp64, its refusals, and the tiny
frozen bf16 teacher under strict mode, through the tap machinery and one trainer step.

The yardstick of every accuracy check is measured in the same test: the existing kernel (basd_attention_fwd_bf16) on
the same qkv against its own fp64 reference without a bias, or the plain-ViT twin of the model against its own fp64
forward.  The new code adds one fp32 add per logit, so it may reach at most 1.5 times that error.
"""
import ctypes
import functools
import os

import pytest
import torch

from tests._beit_cases import DEPTH, DIM, GRID, HEADS, IMG, PATCH, tiny_beit
from tests._beit_ref import beit_forward, biased_attention, fp64_params, seeded_table, table_rows
from tests._teacher_cases import bf16_frozen, images as _images

pytestmark = pytest.mark.gpu

CFG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                   "vit-bias-aware-structural-distillation_amd", "configs", "config.yaml")
HD = 64
SCALE = HD ** -0.5
# (gh, gw, heads, batch): T = 2, 7, 7, 17, 197, 257 -- all three instantiations (T <= 64, <= 208, <= 272), a ragged last
# key tile everywhere, non-square grids both ways, H = 3 against a wrong head stride of the [R, H] table
CASES = [(1, 1, 2, 3), (2, 3, 2, 3), (2, 3, 3, 3), (3, 2, 2, 3), (4, 4, 2, 3), (14, 14, 2, 2), (14, 14, 3, 2),
         (16, 16, 2, 2)]
FACTOR = 1.5


@functools.lru_cache(maxsize=None)
def _case(gh, gw, heads, batch):
    """qkv (bf16, CPU), the seeded table and the two fp64 references, computed once per case"""
    t = gh * gw + 1
    g = torch.Generator().manual_seed(1000 * gh + 10 * gw + heads)
    qkv = torch.randn(batch, t, 3 * heads * HD, generator=g).to(torch.bfloat16)
    table = seeded_table(gh, gw, heads, seed=gh + 31 * gw)
    return {"qkv": qkv, "table": table, "biased": biased_attention(qkv, table, gh, gw, heads, SCALE),
            "plain": biased_attention(qkv, None, gh, gw, heads, SCALE)}


def _errors(out, imp, want):
    """(relative L2 error of out, worst relative error of the importance) against an fp64 (out, importance) pair"""
    want_out, want_imp = want
    e_out = float((out.double().cpu() - want_out).norm() / want_out.norm())
    e_imp = float(((imp.double().cpu() - want_imp).abs() / want_imp).max()) if imp is not None else None
    return e_out, e_imp


def _yardstick(case, heads):
    """the existing kernel on the same qkv against the unbiased fp64 reference"""
    import basd_amd._native as native
    out, imp = native.attention_fwd(case["qkv"].cuda(), heads, HD, SCALE, want_importance=True)
    return _errors(out, imp, case["plain"])


def _run(case, table, gh, gw, heads, want_importance=True):
    import basd_amd._native as native
    out, imp = native.attention_fwd_relbias(case["qkv"].cuda(), table.cuda(), gh, gw, heads, HD, SCALE, want_importance)
    torch.cuda.synchronize()
    return out, imp


@pytest.mark.parametrize("gh,gw,heads,batch", CASES)
def test_kernel_matches_fp64_like_the_unbiased_kernel(gh, gw, heads, batch):
    """Measured on an MI355X (new / existing kernel): DESIGN.md section 21."""
    case = _case(gh, gw, heads, batch)
    t = gh * gw + 1
    out, imp = _run(case, case["table"], gh, gw, heads)
    assert out.shape == (batch, t, heads * HD) and imp.shape == (batch, t - 1) and imp.dtype == torch.float32
    new_out, new_imp = _errors(out, imp, case["biased"])
    old_out, old_imp = _yardstick(case, heads)
    print(f"relbias {gh}x{gw} H={heads} T={t}: out rel-L2 new {new_out:.3e} / existing {old_out:.3e} = "
          f"{new_out / old_out:.3f}; importance worst rel new {new_imp:.3e} / existing {old_imp:.3e} = "
          f"{new_imp / old_imp:.3f}")
    assert new_out <= FACTOR * old_out, (new_out, old_out)
    assert new_imp <= FACTOR * old_imp, (new_imp, old_imp)
    # without the importance pointer: the same output, bit for bit, and nothing else written
    out2, none = _run(case, case["table"], gh, gw, heads, want_importance=False)
    assert none is None and torch.equal(out2.view(torch.int16), out.view(torch.int16))


@pytest.mark.parametrize("gh,gw,heads,batch", [(2, 3, 3, 3), (14, 14, 2, 2), (16, 16, 2, 2)])
def test_zero_table_reproduces_the_unbiased_kernel(gh, gw, heads, batch):
    case = _case(gh, gw, heads, batch)
    out, imp = _run(case, torch.zeros_like(case["table"]), gh, gw, heads)
    new_out, new_imp = _errors(out, imp, case["plain"])
    old_out, old_imp = _yardstick(case, heads)
    print(f"relbias zero table {gh}x{gw} H={heads}: out {new_out:.3e} / {old_out:.3e}, importance {new_imp:.3e} / "
          f"{old_imp:.3e}")
    assert new_out <= FACTOR * old_out and new_imp <= FACTOR * old_imp


@pytest.mark.parametrize("gh,gw,heads,batch", [(2, 3, 3, 3), (14, 14, 2, 2)])
def test_cls_rows_change_exactly_what_they_touch(gh, gw, heads, batch):
    """table rows R-3 (CLS query, patch key) and R-1 (CLS, CLS) bias only query row 0: output row 0 and the tap move,
    every other output row keeps its bits; row R-2 (patch query, CLS key) biases only column 0 of the patch queries:
    output row 0 and the tap keep their bits, the other rows move.  Each against fp64 as well."""
    case = _case(gh, gw, heads, batch)
    rows = table_rows(gh, gw)
    zero = torch.zeros(rows, heads)
    base_out, base_imp = _run(case, zero, gh, gw, heads)
    old_out, old_imp = _yardstick(case, heads)

    def check(table):
        out, imp = _run(case, table, gh, gw, heads)
        e_out, e_imp = _errors(out, imp, biased_attention(case["qkv"], table, gh, gw, heads, SCALE))
        assert e_out <= FACTOR * old_out and e_imp <= FACTOR * old_imp, (e_out, old_out, e_imp, old_imp)
        return out, imp

    query0 = zero.clone()
    query0[rows - 3] = -3.0 + 0.5 * torch.arange(heads)
    query0[rows - 1] = 5.0
    out, imp = check(query0)
    assert torch.equal(out[:, 1:].view(torch.int16), base_out[:, 1:].view(torch.int16))
    assert not torch.equal(out[:, 0], base_out[:, 0]) and not torch.equal(imp, base_imp)

    column0 = zero.clone()
    column0[rows - 2] = 2.0 + 0.5 * torch.arange(heads)
    out, imp = check(column0)
    assert torch.equal(out[:, 0].view(torch.int16), base_out[:, 0].view(torch.int16)) and torch.equal(imp, base_imp)
    assert not torch.equal(out[:, 1:], base_out[:, 1:])

    patches = case["table"].clone()                 # ... and the patch rows alone leave the CLS query's logits alone
    patches[rows - 3:] = 0.0
    out, imp = check(patches)
    assert torch.equal(out[:, 0].view(torch.int16), base_out[:, 0].view(torch.int16)) and torch.equal(imp, base_imp)


@pytest.mark.parametrize("gh,gw,hd", [(16, 17, 64), (14, 14, 80), (0, 5, 64)])
def test_refused_shapes_return_err_shape_and_write_nothing(gh, gw, hd):
    import basd_amd._native as native
    b, heads, t = 2, 2, max(gh * gw + 1, 2)
    qkv = torch.zeros(b, t, 3 * heads * hd, dtype=torch.bfloat16, device="cuda")
    table = torch.zeros(max(table_rows(gh, gw), 4), heads, device="cuda")
    out = torch.full((b, t, heads * hd), 7.0, dtype=torch.bfloat16, device="cuda")
    imp = torch.full((b, heads, t - 1), 7.0, device="cuda")
    assert not native.attention_fwd_relbias_supported(gh, gw, hd)
    rc = native.lib().basd_attention_fwd_relbias_bf16(
        ctypes.c_void_p(qkv.data_ptr()), ctypes.c_void_p(table.data_ptr()), b, gh, gw, heads, hd, ctypes.c_float(0.125),
        ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(imp.data_ptr()),
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 1                                   # BASD_ERR_SHAPE
    assert bool((out == 7.0).all()) and bool((imp == 7.0).all())
    assert native.attention_fwd_relbias_supported(16, 16, 64) and native.attention_fwd_relbias_supported(1, 271, 64)


# ---------------------------------------------------------------------------------------------------------------------
# the tiny frozen teacher

def _frozen(model):
    """what load_teacher does to a Beit: qkv bias materialised, LayerScale folded, bf16 with fp32 norms and table"""
    from basd_amd.models.teacher import fold_layerscale
    model.materialize_qkv_bias()
    for p in model.parameters():
        p.requires_grad = False
    assert fold_layerscale(model) == 2 * DEPTH
    return bf16_frozen(model.cuda())


def _twin_of(model):
    """the plain ViT with the same (folded, bf16) weights, a zero position embedding and no bias table: the code the
    library had before this teacher"""
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


def test_tiny_teacher_runs_strict_on_the_new_kernel_and_matches_fp64_like_the_plain_twin(monkeypatch):
    """Measured on an MI355X (rel-L2 per layer, BEiT / plain twin): DESIGN.md section 21."""
    import basd_amd._native as native
    calls = []
    real = native.attention_fwd_relbias

    def spy(qkv, table, gh, gw, heads, head_dim, scale, want_importance=False):
        calls.append((tuple(qkv.shape), (gh, gw), table.dtype, want_importance))
        return real(qkv, table, gh, gw, heads, head_dim, scale, want_importance)

    monkeypatch.setattr(native, "attention_fwd_relbias", spy)
    batch = 3
    model = _frozen(tiny_beit())
    assert model.blocks[0].attn.relative_position_bias_table.dtype == torch.float32
    assert model.blocks[0].attn.qkv.weight.dtype == torch.bfloat16
    twin = _twin_of(model)
    x = _images(batch, IMG, seed=3).cuda()
    errs = {}
    for label, m in (("beit", model), ("twin", twin)):
        toks, imps = _strict_intermediates(_teacher(m), x)
        assert len(toks) == DEPTH and toks[0].shape == (batch, 16, DIM) and imps[DEPTH - 1].shape == (batch, 16)
        want_t, want_i = beit_forward(fp64_params(m.state_dict()), x.to(torch.bfloat16), heads=HEADS)
        errs[label] = _rel_l2(toks, want_t)
        if label == "beit":
            assert calls == [((batch, 17, 3 * DIM), GRID, torch.float32, True)] * DEPTH, calls
            for j in range(DEPTH):      # bf16 activations in front of the softmax: a loose, sound bound
                assert torch.allclose(imps[j].double().cpu(), want_i[j], rtol=0.1, atol=1e-3), j
    assert len(calls) == DEPTH                       # the twin ran the existing kernel
    print(f"beit-teacher: rel-L2 vs fp64 per layer: beit {[f'{v:.3e}' for v in errs['beit']]}, "
          f"plain twin {[f'{v:.3e}' for v in errs['twin']]}")
    for j in range(DEPTH):
        assert errs["beit"][j] <= FACTOR * errs["twin"][j], (j, errs)


def test_library_path_is_a_counted_fallback_and_agrees():
    """the switch of scripts/time_beit_teacher.py: dense bias + SDPA + separate tap, counted, refused in strict mode"""
    import basd_amd.losses._ops as O
    import basd_amd.models.beit as B
    from basd_amd.models.teacher import extract_intermediates
    teacher = _teacher(_frozen(tiny_beit()))
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
        assert rel < 2e-2, (j, rel)                  # two bf16 pipelines (test_clip_teacher_gpu.py uses the same bound)
        assert torch.allclose(imps[j], lib_imps[j], rtol=0.1, atol=1e-3), j


def test_one_eager_trainer_step_against_the_tiny_beit_teacher():
    import basd_amd.losses._ops as O
    from basd_amd.config import load_config
    from basd_amd.models.teacher import probe_model
    from basd_amd.train import SyntheticLoader, _create_student
    from basd_amd.training.trainer import Trainer
    batch = 8
    teacher = _teacher(_frozen(tiny_beit()))
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
