"""EVA-02 teachers without a GPU: the rotary table rule, the model arithmetic on the CPU path, the timm state-dict
mapping, the presets, the loader and the C entry's declaration and argument checks.

The arithmetic is pinned against ``tests/_eva_ref.py``, an fp64 forward written out with plain torch ops whose rotation
comes from timm's construction (meshgrid, bands, ``repeat_interleave``, ``x * cos + rot(x) * sin``), not from the
per-pair table the kernel and the model use."""
import ctypes
import os
import re
import types

import pytest
import torch

from tests._eva_ref import (BATCH, DEPTH, DIM, GRID, HEADS, HIDDEN, IMG, REF_GRID, eva_forward, fp64_params, timm_apply,
                            timm_rope, timm_state_dict, tiny_eva)

CLIP_MEAN, CLIP_STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
# name -> (embed_dim, depth, heads, hidden, sub-LN)
PRESETS = {
    "eva02_tiny_patch14_224": (192, 12, 3, 512, False),
    "eva02_small_patch14_224": (384, 12, 6, 1024, False),
    "eva02_base_patch14_224": (768, 12, 12, 2048, True),
}
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "basd_hip.h")
ENTRY = "basd_attention_fwd_rope_bf16"
_CTYPE = {"const void*": ctypes.c_void_p, "void*": ctypes.c_void_p, "float*": ctypes.c_void_p,
          "const float*": ctypes.c_void_p, "int": ctypes.c_int, "float": ctypes.c_float}


@pytest.fixture
def host_only():
    """a kernel provider that takes no tensor: every module runs its stock torch path"""
    from basd_amd.losses import _ops
    _ops.set_ops(types.SimpleNamespace(handles=lambda t: False))
    yield
    _ops.set_ops(None)


def _teacher(model):
    from basd_amd.models.teacher import TeacherModel
    return TeacherModel(model=model, embed_dim=DIM, heads_per_layer=[HEADS] * DEPTH, depth=DEPTH, mlp_ratio=0.0,
                        layer_paths=[f"blocks.{i}" for i in range(DEPTH)], attn_subpath="attn", has_cls_token=True,
                        feature_format="token", mean=CLIP_MEAN, std=CLIP_STD)


@pytest.mark.parametrize("gh,gw,ref", [(1, 1, None), (1, 5, None), (2, 3, None), (3, 2, None), (4, 4, None),
                                       (16, 16, None), (16, 16, (16, 16)), (24, 24, (16, 16))])
def test_table_equals_the_timm_construction(gh, gw, ref):
    """the per-pair (cos, sin) table applied the model's way against timm's per-channel sin / cos applied timm's way, on
    random vectors in fp64: the table is fp32 (relative 6e-8 on values <= 1), the vectors N(0, 1) -> 1e-6 absolute"""
    from basd_amd._native import rope_table
    from basd_amd.models.eva import apply_rope
    hd = 64
    table = rope_table(gh, gw, hd, ref_grid=ref)
    assert table.dtype == torch.float32 and tuple(table.shape) == (1 + gh * gw, hd // 2, 2) and table.device.type == "cpu"
    assert torch.equal(table[0], torch.tensor([1.0, 0.0]).expand(hd // 2, 2))              # the CLS row: identity
    x = torch.randn(2, 3, 1 + gh * gw, hd, dtype=torch.float64, generator=torch.Generator().manual_seed(gh * 100 + gw))
    got = apply_rope(x, table)
    assert got.dtype == torch.float64 and torch.equal(got[:, :, 0], x[:, :, 0])
    sin, cos = timm_rope(gh, gw, hd, ref)
    assert float((got[:, :, 1:] - timm_apply(x[:, :, 1:], sin, cos)).abs().max()) < 1e-6
    # more prefix rows, no prefix row
    assert torch.equal(rope_table(gh, gw, hd, ref_grid=ref, prefix_tokens=0), table[1:])
    three = rope_table(gh, gw, hd, ref_grid=ref, prefix_tokens=3)
    assert torch.equal(three[3:], table[1:]) and torch.equal(three[:3], table[:1].expand(3, -1, -1))


def test_scaled_coordinates_differ_from_plain_ones_and_bands_follow_the_temperature():
    from basd_amd._native import rope_table
    plain, scaled = rope_table(24, 24, 64), rope_table(24, 24, 64, ref_grid=(16, 16))
    assert float((plain - scaled).abs().max()) > 0.5
    # patch (1, 0): y = 1, x = 0 -> pair j < 16 has the angle temperature^(-j / 16), pairs 16 .. 31 the angle 0
    t = rope_table(2, 2, 64, temperature=100.0)
    want = 100.0 ** (-torch.arange(16, dtype=torch.float64) / 16)
    assert torch.allclose(t[1 + 2, :16, 0].double(), want.cos(), atol=1e-7)
    assert torch.allclose(t[1 + 2, :16, 1].double(), want.sin(), atol=1e-7)
    assert torch.equal(t[1 + 2, 16:], torch.tensor([1.0, 0.0]).expand(16, 2))


@pytest.mark.parametrize("scale_mlp", [False, True])
def test_tiny_model_in_fp32_equals_the_fp64_forward(host_only, scale_mlp):
    """fp32 model, fp64 reference.  Bound (as tests/test_beit_teacher_cpu.py): every token is the end of a chain of fp32
    dot products of at most 588 terms (the patch embedding) with unit roundoff 6e-8: sqrt(588) * 6e-8 = 1.5e-6 relative
    per product if the roundings were independent, a handful of products per block, two blocks -> 2e-5 in relative L2
    per layer; the taps are fp32 softmax outputs of logits carrying that error times |logit| < 20: rtol 1e-3, atol
    1e-6."""
    from basd_amd.models.teacher import extract_intermediates
    model = tiny_eva(scale_mlp)
    assert (model.blocks[0].mlp.norm is not None) == scale_mlp
    x = torch.randn(BATCH, 3, IMG, IMG, generator=torch.Generator().manual_seed(2))
    want_t, want_i = eva_forward(fp64_params(model.state_dict()), x, heads=HEADS)
    toks, imps = extract_intermediates(_teacher(model), x)
    for j in range(DEPTH):
        err = float((toks[j].double() - want_t[j][:, 1:]).norm() / want_t[j][:, 1:].norm())
        assert err < 2e-5, (j, err)
        assert imps[j].shape == (BATCH, GRID[0] * GRID[1])
        torch.testing.assert_close(imps[j].double(), want_i[j], rtol=1e-3, atol=1e-6)
    model.materialize_qkv_bias()                     # the materialised bias is the same forward
    toks2, _ = extract_intermediates(_teacher(model), x)
    assert all(torch.equal(toks[j], toks2[j]) for j in range(DEPTH))


def test_rotation_and_sub_ln_change_the_result():
    """the reference without the rotation, and without the sub-LN, is far from the full one: the checks above see both"""
    model = tiny_eva(True)
    x = torch.randn(2, 3, IMG, IMG, generator=torch.Generator().manual_seed(2))
    params = fp64_params(model.state_dict())
    a, _ = eva_forward(params, x, heads=HEADS)
    b, _ = eva_forward(params, x, heads=HEADS, ref_grid=GRID)                     # other coordinates
    c, _ = eva_forward({k: v for k, v in params.items() if "mlp.norm" not in k}, x, heads=HEADS)
    assert float((a[0] - b[0]).norm() / a[0].norm()) > 1e-3
    assert float((a[0] - c[0]).norm() / a[0].norm()) > 1e-2


@pytest.mark.parametrize("scale_mlp", [False, True])
def test_separate_and_fused_qkv_checkpoints_load_to_the_same_model(host_only, scale_mlp):
    from basd_amd.models.eva import eva_state_dict, load_eva_state_dict
    src = tiny_eva(scale_mlp, seed=7)
    fused, separate = timm_state_dict(src, False), timm_state_dict(src, True)
    assert "blocks.0.attn.q_proj.weight" in separate and "blocks.0.attn.q_proj.bias" in separate
    assert not any("qkv" in k or "q_bias" in k for k in separate) and "blocks.1.attn.qkv.weight" in fused
    mapped = eva_state_dict(src, separate)
    assert not any(k.startswith(("rope.", "head.", "fc_norm.")) or "k_bias" in k or "_proj." in k for k in mapped)
    models = []
    for state in (fused, separate):
        dst = tiny_eva(scale_mlp, seed=21)
        assert load_eva_state_dict(dst, state) == []
        attn = dst.blocks[0].attn
        assert torch.equal(attn.qkv.bias[:DIM], attn.q_bias) and torch.equal(attn.qkv.bias[2 * DIM:], attn.v_bias)
        assert not bool(attn.qkv.bias[DIM:2 * DIM].any()) and not attn.qkv.bias.requires_grad
        for name, a in src.state_dict().items():
            assert torch.equal(a, dst.state_dict()[name]), name
        models.append(dst)
    x = torch.randn(2, 3, IMG, IMG, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        assert torch.equal(models[0].forward_features(x), models[1].forward_features(x))
    broken = dict(separate)
    del broken["blocks.1.attn.k_proj.weight"]
    with pytest.raises(ValueError, match="go together"):
        eva_state_dict(src, broken)


def test_a_pos_embed_of_another_size_is_refused_with_both_sizes(host_only):
    from basd_amd.models.eva import load_eva_state_dict
    model = tiny_eva(False)
    state = timm_state_dict(model, False)
    state["pos_embed"] = torch.zeros(1, 257, DIM)
    with pytest.raises(ValueError, match=r"257 rows.*has 17.*not resampled"):
        load_eva_state_dict(model, state)
    with pytest.raises(ValueError, match="10 tokens.*17 tokens"):       # the forward refuses another token count too
        model.blocks[0].attn(torch.zeros(1, 10, DIM))


def test_the_table_stays_fp32_under_a_bf16_cast_and_is_no_state_dict_key():
    model = tiny_eva(True)
    before = model.blocks[0].attn.rope.clone()
    assert not any("rope" in k for k in model.state_dict())
    model = model.to(torch.bfloat16)
    attn = model.blocks[0].attn
    assert attn.qkv.weight.dtype == torch.bfloat16 and attn.rope.dtype == torch.float32
    assert torch.equal(attn.rope, before)


def test_other_models_keep_their_keys():
    """Block gained an ``mlp_cls`` argument: the plain ViT and BEiT build the module tree they had"""
    from basd_amd.models.beit import Beit
    from basd_amd.models.vit import VisionTransformer
    vit = VisionTransformer(img_size=32, patch_size=16, num_classes=0, embed_dim=64, depth=1, num_heads=1)
    assert sorted(k for k in vit.state_dict() if k.startswith("blocks.0.mlp")) == [
        "blocks.0.mlp.fc1.bias", "blocks.0.mlp.fc1.weight", "blocks.0.mlp.fc2.bias", "blocks.0.mlp.fc2.weight"]
    beit = Beit(img_size=32, patch_size=16, embed_dim=64, depth=1, num_heads=1)
    assert [n for n, _ in beit.blocks[0].named_children()] == [n for n, _ in vit.blocks[0].named_children()]


@pytest.mark.parametrize("name", sorted(PRESETS))
def test_preset_builds_with_timm_parameter_names(name):
    from basd_amd.models.eva import EVA_PRESETS, create_eva
    dim, depth, heads, hidden, sub_ln = PRESETS[name]
    assert EVA_PRESETS[name] == (dim, depth, heads, 14, hidden, sub_ln, (16, 16), CLIP_MEAN, CLIP_STD)
    with torch.device("meta"):                   # shapes and names only
        model = create_eva(name, img_size=224)
    keys = set(model.state_dict())
    assert {"pos_embed", "cls_token", "norm.weight", "patch_embed.proj.weight"} <= keys
    assert tuple(model.pos_embed.shape) == (1, 257, dim)
    assert not any(k.startswith(("head", "fc_norm")) or "rope" in k or "ls1" in k or "qkv.bias" in k for k in keys)
    assert len(model.blocks) == depth and model.embed_dim == model.num_features == dim
    block_keys = {k[len("blocks.0."):] for k in keys if k.startswith("blocks.0.")}
    want = {"norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.q_bias", "attn.v_bias", "attn.proj.weight",
            "attn.proj.bias", "norm2.weight", "norm2.bias", "mlp.fc1_g.weight", "mlp.fc1_g.bias", "mlp.fc1_x.weight",
            "mlp.fc1_x.bias", "mlp.fc2.weight", "mlp.fc2.bias"}
    assert block_keys == want | ({"mlp.norm.weight", "mlp.norm.bias"} if sub_ln else set())
    for blk in model.blocks:
        assert blk.attn.num_heads == heads and blk.attn.head_dim == 64 and blk.norm1.eps == 1e-6
        assert tuple(blk.attn.rope.shape) == (257, 32, 2)
        assert blk.mlp.fc1_g.out_features == hidden and blk.mlp.fc2.in_features == hidden
        assert isinstance(blk.ls1, torch.nn.Identity) and isinstance(blk.ls2, torch.nn.Identity)


def test_load_teacher_builds_eva02_tiny_and_probes_it():
    """today's ``ValueError: not a known preset``; the tagged name resolves through the base-name rule"""
    from basd_amd.models.eva import Eva
    from basd_amd.models.teacher import load_teacher
    t = load_teacher("eva02_tiny_patch14_224.mim_in22k", 224, device="cpu")
    assert isinstance(t.model, Eva)
    assert t.feature_format == "token" and t.has_cls_token is True and t.depth == 12 and t.heads_per_layer == [3] * 12
    assert t.mean == CLIP_MEAN and t.std == CLIP_STD and t.embed_dim == 192 and t.attn_subpath == "attn"
    assert t.layer_paths == [f"blocks.{i}" for i in range(12)]
    assert t.mlp_ratio == 0.0                        # the probe looks for ``fc1``: this MLP has fc1_g / fc1_x
    assert not any(p.requires_grad for p in t.model.parameters()) and not t.model.training
    blk = t.model.blocks[0]
    assert blk.attn.qkv.bias is not None and blk.attn.qkv.weight.dtype == torch.bfloat16      # materialised, cast
    assert blk.attn.rope.dtype == torch.float32 and blk.norm1.weight.dtype == torch.float32
    with pytest.raises(ValueError, match="not a known preset"):
        load_teacher("eva02_large_patch14_224.mim_in22k", 224, device="cpu")


def test_load_teacher_reads_a_separate_qkv_checkpoint(tmp_path, host_only):
    from basd_amd.models.eva import create_eva
    from basd_amd.models.teacher import load_teacher
    torch.manual_seed(11)
    src = create_eva("eva02_tiny_patch14_224", img_size=56)
    with torch.no_grad():
        for blk in src.blocks:
            blk.attn.q_bias.normal_()
    path = tmp_path / "eva.pt"
    torch.save(timm_state_dict(src, True), path)
    t = load_teacher("eva02_tiny_patch14_224", 56, weights=str(path), device="cpu", dtype=torch.float32)
    assert torch.equal(t.model.blocks[3].attn.qkv.weight, src.blocks[3].attn.qkv.weight)
    assert torch.equal(t.model.blocks[3].attn.qkv.bias[:192], src.blocks[3].attn.q_bias)


# ---------------------------------------------------------------------------------------------------------------------
# the C entry, as far as a machine without a GPU can see it

@pytest.fixture(scope="module")
def lib():
    import basd_amd._native as native
    if not os.path.exists(native.LIB_PATH):
        native.build()
    return native.lib()


def test_entry_is_exported_with_the_header_signature(lib):
    import basd_amd._native as native
    text = open(HEADER).read()
    assert ENTRY in native.EXPORTS and hasattr(lib, ENTRY)
    m = re.search(r"\bint " + ENTRY + r"\(([^)]*)\);", text)
    assert m, "include/basd_hip.h does not declare the entry"
    args = [" ".join(a.split()[:-1]) for a in m.group(1).split(",")]
    assert tuple(_CTYPE[a] for a in args) == native._SIGNATURES[ENTRY]
    assert text.count(ENTRY) >= 2                    # the declaration and the list of entries at the top


@pytest.mark.parametrize("b,t,h,hd,table", [(2, 17, 2, 80, True), (2, 1, 2, 64, True), (2, 273, 2, 64, True),
                                            (2, 17, 2, 64, False), (2, 17, 0, 64, True), (0, 17, 2, 64, True)])
def test_refused_arguments_return_err_shape_before_anything_touches_a_device(lib, b, t, h, hd, table):
    import basd_amd._native as native
    p = lambda on: ctypes.c_void_p(4096 if on else 0)       # never dereferenced on the host
    rc = lib.basd_attention_fwd_rope_bf16(p(True), p(table), b, t, h, hd, ctypes.c_float(0.125), p(True), p(False), p(False))
    assert rc == 1                                   # BASD_ERR_SHAPE
    assert "attention_fwd_rope" in lib.basd_last_error().decode()
    assert not native.attention_fwd_rope_supported(t, hd) or not table or h < 1 or b < 1
    assert native.attention_fwd_rope_supported(2, 64) and native.attention_fwd_rope_supported(272, 64)
