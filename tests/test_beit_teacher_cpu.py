"""BEiT / BEiT-v2 teachers without a GPU: the closed-form bias index, the model arithmetic on the CPU path, the timm
state-dict mapping, the presets and the probe record.

The arithmetic is pinned against ``tests/_beit_ref.py``, an fp64 forward written out with plain torch ops whose bias
index comes from timm's meshgrid construction, not from the closed form the kernel and the model use."""
import types

import pytest
import torch

from tests._beit_cases import DEPTH, DIM, GRID, HEADS, IMG, tiny_beit, timm_state_dict
from tests._beit_ref import beit_forward, fp64_params, meshgrid_index, table_rows

IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
HALF = (0.5, 0.5, 0.5)
# name -> (embed_dim, depth, heads, mean, std)
PRESETS = {
    "beit_base_patch16_224": (768, 12, 12, HALF, HALF),
    "beit_large_patch16_224": (1024, 24, 16, HALF, HALF),
    "beitv2_base_patch16_224": (768, 12, 12, IMAGENET_MEAN, IMAGENET_STD),
    "beitv2_large_patch16_224": (1024, 24, 16, IMAGENET_MEAN, IMAGENET_STD),
}


@pytest.fixture
def host_only():
    """a kernel provider that takes no tensor: every module runs its stock torch path"""
    from basd_amd.losses import _ops
    _ops.set_ops(types.SimpleNamespace(handles=lambda t: False))
    yield
    _ops.set_ops(None)


def _teacher(model):
    from basd_amd.models.teacher import TeacherModel
    return TeacherModel(model=model, embed_dim=DIM, heads_per_layer=[HEADS] * DEPTH, depth=DEPTH, mlp_ratio=4.0,
                        layer_paths=[f"blocks.{i}" for i in range(DEPTH)], attn_subpath="attn", has_cls_token=True,
                        feature_format="token", mean=HALF, std=HALF)


@pytest.mark.parametrize("gh,gw", [(1, 1), (1, 5), (2, 3), (3, 2), (4, 4), (14, 14)])
def test_closed_form_index_equals_the_meshgrid_construction(gh, gw):
    from basd_amd._native import relbias_index
    from basd_amd.models.beit import relative_position_index
    want = meshgrid_index(gh, gw)
    t = gh * gw + 1
    got = torch.tensor([[relbias_index(i, j, gh, gw) for j in range(t)] for i in range(t)])
    assert torch.equal(got, want)
    assert torch.equal(relative_position_index(gh, gw), want)
    assert int(want.max()) == table_rows(gh, gw) - 1 and int(want.min()) == 0


def test_tiny_model_in_fp64_equals_the_written_out_forward(host_only):
    """the model cast to fp64 against the restatement, at the tolerances tests/test_vit_ref_cpu.py uses for the plain
    ViT (tokens rtol 1e-10 / atol 1e-12); the tap's softmax runs in fp32 in the model (rtol 1e-5 / atol 1e-7, as
    tests/test_clip_teacher_cpu.py)"""
    from basd_amd.models.teacher import extract_intermediates
    model = tiny_beit().double()
    assert model.blocks[0].attn.relative_position_bias_table.dtype == torch.float64
    x = torch.randn(3, 3, IMG, IMG, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    toks, imps = extract_intermediates(_teacher(model), x)
    want_t, want_i = beit_forward(fp64_params(model.state_dict()), x, heads=HEADS)
    for j in range(DEPTH):
        torch.testing.assert_close(toks[j], want_t[j][:, 1:], rtol=1e-10, atol=1e-12)
        torch.testing.assert_close(imps[j].double(), want_i[j], rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("materialized", [False, True])
def test_tiny_model_in_fp32_equals_the_fp64_forward(host_only, materialized):
    """fp32 model, fp64 reference.  Bound: every token is the end of a chain of fp32 dot products of at most 768 terms
    (the patch embedding) with unit roundoff 6e-8: an error of sqrt(768) * 6e-8 = 1.7e-6 relative per product if the
    roundings were independent, a handful of products per block, two blocks -> 2e-5 in relative L2 per layer; the taps are
    fp32 softmax outputs of logits carrying that error times |logit| < 20: rtol 1e-3, atol 1e-6."""
    from basd_amd.models.teacher import extract_intermediates
    model = tiny_beit()
    x = torch.randn(3, 3, IMG, IMG, generator=torch.Generator().manual_seed(2))
    want_t, want_i = beit_forward(fp64_params(model.state_dict()), x, heads=HEADS)
    if materialized:
        model.materialize_qkv_bias()
        assert model.blocks[0].attn.qkv.bias is not None
    toks, imps = extract_intermediates(_teacher(model), x)
    for j in range(DEPTH):
        err = float((toks[j].double() - want_t[j][:, 1:]).norm() / want_t[j][:, 1:].norm())
        assert err < 2e-5, (j, err)
        assert imps[j].shape == (3, GRID[0] * GRID[1])
        torch.testing.assert_close(imps[j].double(), want_i[j], rtol=1e-3, atol=1e-6)


def test_bias_changes_the_result():
    """the reference with the table zeroed is far from the biased one: the checks above see the bias"""
    model = tiny_beit()
    x = torch.randn(2, 3, IMG, IMG, generator=torch.Generator().manual_seed(2))
    params = fp64_params(model.state_dict())
    plain = {k: (torch.zeros_like(v) if k.endswith("relative_position_bias_table") else v) for k, v in params.items()}
    a, _ = beit_forward(params, x, heads=HEADS)
    b, _ = beit_forward(plain, x, heads=HEADS)
    assert float((a[0] - b[0]).norm() / b[0].norm()) > 1e-2


def test_fold_layerscale_keeps_the_tokens(host_only):
    """non-trivial gammas folded into attn.proj / mlp.fc2 (what load_teacher does): the blocks lose their LayerScale
    modules and the tokens still equal the UNFOLDED fp64 forward, at the fp32 bound of the test above"""
    from basd_amd.models.teacher import extract_intermediates, fold_layerscale
    from basd_amd.models.vit import LayerScale
    model = tiny_beit()
    assert isinstance(model.blocks[0].ls1, LayerScale)
    assert float((model.blocks[0].ls1.gamma.detach() - 1.0).abs().max()) > 0.1
    x = torch.randn(3, 3, IMG, IMG, generator=torch.Generator().manual_seed(5))
    want_t, _ = beit_forward(fp64_params(model.state_dict()), x, heads=HEADS)
    for p in model.parameters():
        p.requires_grad = False
    assert fold_layerscale(model) == 2 * DEPTH
    assert all(isinstance(m, torch.nn.Identity) for blk in model.blocks for m in (blk.ls1, blk.ls2))
    toks, _ = extract_intermediates(_teacher(model), x)
    for j in range(DEPTH):
        err = float((toks[j].double() - want_t[j][:, 1:]).norm() / want_t[j][:, 1:].norm())
        assert err < 2e-5, (j, err)


def test_timm_state_dict_loads_with_only_the_documented_keys_dropped(host_only):
    from basd_amd.models.beit import load_timm_state_dict
    src, dst = tiny_beit(seed=7), tiny_beit(seed=21)
    state = timm_state_dict(src)
    assert "blocks.0.gamma_1" in state and "blocks.1.gamma_2" in state and "blocks.0.attn.q_bias" in state
    assert not any("ls1" in k or "ls2" in k or "qkv.bias" in k for k in state)
    missing, dropped = load_timm_state_dict(dst, state)
    assert missing == []
    assert sorted(dropped) == sorted([f"blocks.{i}.attn.relative_position_index" for i in range(DEPTH)]
                                     + ["fc_norm.weight", "fc_norm.bias", "head.weight", "head.bias"])
    for (name, a), (_, b) in zip(src.state_dict().items(), dst.state_dict().items()):
        assert torch.equal(a, b), name
    x = torch.randn(2, 3, IMG, IMG, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        assert torch.equal(src.forward_features(x), dst.forward_features(x))


def test_a_table_for_another_grid_is_refused_with_both_sizes(host_only):
    from basd_amd.models.beit import load_timm_state_dict
    model = tiny_beit()
    state = timm_state_dict(model)
    have, need = table_rows(3, 3), table_rows(*GRID)
    state["blocks.1.attn.relative_position_bias_table"] = torch.zeros(have, HEADS)
    with pytest.raises(ValueError, match=rf"{have} rows.*= {need}.*not resampled"):
        load_timm_state_dict(model, state)
    with pytest.raises(ValueError, match="not resampled"):       # the forward refuses another token count too
        model.blocks[0].attn(torch.zeros(1, 10, DIM))


def test_the_table_stays_fp32_under_a_bf16_cast_and_the_qkv_bias_is_materialized():
    model = tiny_beit()
    before = model.blocks[0].attn.relative_position_bias_table.detach().clone()
    model.materialize_qkv_bias()
    attn = model.blocks[0].attn
    assert torch.equal(attn.qkv.bias[:DIM], attn.q_bias) and torch.equal(attn.qkv.bias[2 * DIM:], attn.v_bias)
    assert not bool(attn.qkv.bias[DIM:2 * DIM].any()) and not attn.qkv.bias.requires_grad
    model = model.to(torch.bfloat16)
    attn = model.blocks[0].attn
    assert attn.qkv.weight.dtype == torch.bfloat16 and attn.qkv.bias.dtype == torch.bfloat16
    assert attn.relative_position_bias_table.dtype == torch.float32
    assert torch.equal(attn.relative_position_bias_table, before)


@pytest.mark.parametrize("name", sorted(PRESETS))
def test_preset_builds_with_timm_parameter_names(name):
    from basd_amd.models.beit import BEIT_PRESETS, create_beit
    dim, depth, heads, mean, std = PRESETS[name]
    assert BEIT_PRESETS[name][:4] == (dim, depth, heads, 16) and BEIT_PRESETS[name][5:] == (mean, std)
    with torch.device("meta"):                   # shapes and names only: nothing of a ViT-L is allocated
        model = create_beit(name, img_size=224)
    keys = set(model.state_dict())
    assert "pos_embed" not in keys and "cls_token" in keys and "norm.weight" in keys
    assert not any(k.startswith("head") or k.startswith("fc_norm") or "relative_position_index" in k for k in keys)
    assert len(model.blocks) == depth and model.embed_dim == model.num_features == dim
    for blk in model.blocks:
        assert blk.attn.num_heads == heads and blk.attn.head_dim == 64 and blk.norm1.eps == 1e-6
        assert tuple(blk.attn.relative_position_bias_table.shape) == (732, heads)
        assert blk.attn.qkv.bias is None and tuple(blk.attn.q_bias.shape) == (dim,)
        assert type(blk.mlp.act) is torch.nn.GELU and blk.mlp.act.approximate == "none"
        assert blk.mlp.fc1.out_features == 4 * dim and tuple(blk.ls1.gamma.shape) == (dim,)


def test_load_teacher_builds_beitv2_base_and_probes_it():
    """today's ``ValueError: not a known preset``; tagged and untagged names resolve alike"""
    from basd_amd.models.beit import Beit
    from basd_amd.models.teacher import load_teacher
    t = load_teacher("beitv2_base_patch16_224", 224, device="cpu", dtype=torch.float32)
    assert isinstance(t.model, Beit)
    assert t.depth == 12 and t.heads_per_layer == [12] * 12 and t.embed_dim == 768 and t.mlp_ratio == 4.0
    assert t.has_cls_token is True and t.attn_subpath == "attn" and t.feature_format == "token"
    assert t.layer_paths == [f"blocks.{i}" for i in range(12)]
    assert t.mean == IMAGENET_MEAN and t.std == IMAGENET_STD
    assert not any(p.requires_grad for p in t.model.parameters()) and not t.model.training
    blk = t.model.blocks[0]
    assert isinstance(blk.ls1, torch.nn.Identity) and blk.attn.qkv.bias is not None      # folded, materialised


def test_probe_reports_196_tokens_and_tags_resolve():
    from basd_amd.models.beit import create_beit
    from basd_amd.models.teacher import load_teacher, probe_model
    info = probe_model(create_beit("beitv2_base_patch16_224", img_size=224, depth=2), 224)
    assert info["num_tokens"] == 196 and info["has_cls_token"] is True and info["feature_format"] == "token"
    assert info["heads_per_layer"] == [12, 12] and info["mlp_ratio"] == 4.0 and info["attn_subpath"] == "attn"
    assert info["embed_dim"] == 768 and info["depth"] == 2
    t = load_teacher("beit_base_patch16_224.in22k_ft_in22k_in1k", 32, device="cpu", dtype=torch.float32)
    assert t.mean == HALF and t.std == HALF and t.depth == 12
    with pytest.raises(ValueError, match="not a known preset"):
        load_teacher("beitv3_base_patch16_224", 224, device="cpu")
