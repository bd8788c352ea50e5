"""CLIP / SigLIP ViT teachers: presets, tags, statistics, probe record and the model arithmetic (no GPU).

The arithmetic is pinned against ``tests/_clip_ref.py``, an fp64 forward written out with plain torch ops from the
definition of the towers, not a call into ``models/vit.py``."""
import pytest
import torch

from tests._clip_ref import clip_forward, fp64_params

CLIP_MEAN, CLIP_STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
HALF = (0.5, 0.5, 0.5)

# name -> (embed_dim, depth, heads, patch, pre_norm, act, class_token, norm_eps, mean, std)
NEW_PRESETS = {
    "vit_base_patch32_clip_224": (768, 12, 12, 32, True, "gelu", True, 1e-5, CLIP_MEAN, CLIP_STD),
    "vit_base_patch16_clip_224": (768, 12, 12, 16, True, "gelu", True, 1e-5, CLIP_MEAN, CLIP_STD),
    "vit_large_patch14_clip_224": (1024, 24, 16, 14, True, "gelu", True, 1e-5, CLIP_MEAN, CLIP_STD),
    "vit_base_patch16_clip_quickgelu_224": (768, 12, 12, 16, True, "quick_gelu", True, 1e-5, CLIP_MEAN, CLIP_STD),
    "vit_large_patch14_clip_quickgelu_224": (1024, 24, 16, 14, True, "quick_gelu", True, 1e-5, CLIP_MEAN, CLIP_STD),
    "vit_base_patch16_siglip_224": (768, 12, 12, 16, False, "gelu_tanh", False, 1e-6, HALF, HALF),
}


@pytest.mark.parametrize("name", sorted(NEW_PRESETS))
def test_preset_builds_with_timm_parameter_names(name):
    from basd_amd.models.vit import MLP_ACTS, QuickGELU, create_vit, vit_preset
    dim, depth, heads, patch, pre_norm, act, cls, eps, mean, std = NEW_PRESETS[name]
    ps = vit_preset(name)
    assert (ps.embed_dim, ps.depth, ps.heads, ps.patch, ps.layerscale) == (dim, depth, heads, patch, None)
    assert (ps.pre_norm, ps.act, ps.class_token, ps.norm_eps, ps.mean, ps.std) == (pre_norm, act, cls, eps, mean, std)
    assert act in MLP_ACTS
    with torch.device("meta"):                   # shapes and names only: nothing of a ViT-L is allocated
        model = create_vit(name, num_classes=0, img_size=224)
    keys = set(model.state_dict())
    assert ("norm_pre.weight" in keys) == pre_norm and ("norm_pre.bias" in keys) == pre_norm
    assert ("patch_embed.proj.bias" in keys) == (not pre_norm)
    assert ("cls_token" in keys) == cls
    n_tok = (224 // patch) ** 2 + int(cls)
    assert tuple(model.pos_embed.shape) == (1, n_tok, dim) and len(model.blocks) == depth
    assert tuple(model.patch_embed.proj.weight.shape) == (dim, 3, patch, patch)
    assert not any(k.startswith("attn_pool") or k.startswith("head") for k in keys)
    for blk in model.blocks:
        assert blk.attn.num_heads == heads and blk.norm1.eps == eps and blk.norm2.eps == eps
        assert blk.mlp.fc1.out_features == 4 * dim and blk.mlp.act_name == act
        if act == "quick_gelu":
            assert isinstance(blk.mlp.act, QuickGELU)
        else:
            assert isinstance(blk.mlp.act, torch.nn.GELU)
            assert blk.mlp.act.approximate == ("tanh" if act == "gelu_tanh" else "none")
    assert model.norm.eps == eps and (model.norm_pre is None or model.norm_pre.eps == eps)


def test_existing_presets_keep_their_module_tree():
    """the switches default to the plain ViT: no ``norm_pre`` module or key, erf-GELU, eps 1e-6, a patch bias"""
    from basd_amd.models.vit import VIT_PRESETS, create_vit, vit_preset
    for name in sorted(set(VIT_PRESETS) - set(NEW_PRESETS)):
        ps = vit_preset(name)
        assert (ps.pre_norm, ps.act, ps.class_token, ps.norm_eps) == (False, "gelu", True, 1e-6), name
        assert (ps.mean, ps.std) == (IMAGENET_MEAN, IMAGENET_STD), name
    with torch.device("meta"):
        model = create_vit("vit_base_patch16_224", num_classes=0, img_size=224)
    assert model.norm_pre is None and "norm_pre" not in dict(model.named_modules())
    assert "patch_embed.proj.bias" in model.state_dict()
    assert type(model.blocks[0].mlp.act) is torch.nn.GELU and model.blocks[0].mlp.act.approximate == "none"
    assert model.norm.eps == 1e-6 and model.blocks[0].norm1.eps == 1e-6


@pytest.mark.parametrize("name,tagged", [
    ("vit_base_patch16_clip_quickgelu_224", "vit_base_patch16_clip_quickgelu_224.openai"),
    ("vit_base_patch32_clip_224", "vit_base_patch32_clip_224.laion2b_ft_in12k_in1k"),
    ("vit_base_patch16_siglip_224", "vit_base_patch16_siglip_224.webli"),
])
def test_load_teacher_returns_preset_statistics_and_probe_record(name, tagged):
    from basd_amd.models.teacher import load_teacher
    dim, depth, heads, patch, pre_norm, act, cls, eps, mean, std = NEW_PRESETS[name]
    t = load_teacher(tagged, 224, device="cpu", dtype=torch.float32)
    assert t.mean == mean and t.std == std
    assert t.embed_dim == dim and t.depth == depth and t.heads_per_layer == [heads] * depth
    assert t.mlp_ratio == 4.0 and t.attn_subpath == "attn" and t.feature_format == "token"
    assert t.has_cls_token is cls and t.layer_paths == [f"blocks.{i}" for i in range(depth)]
    assert not any(p.requires_grad for p in t.model.parameters()) and not t.model.training


def test_probe_reports_the_token_count_of_every_new_preset():
    """196 tokens and no CLS token for SigLIP; heads, mlp_ratio and the attention sub-path for all six (built two blocks
    deep: the probe's forward of a ViT-L on the CPU is not what is being tested)"""
    from basd_amd.models.teacher import probe_model
    from basd_amd.models.vit import create_vit
    for name, (dim, depth, heads, patch, pre_norm, act, cls, eps, mean, std) in sorted(NEW_PRESETS.items()):
        info = probe_model(create_vit(name, num_classes=0, img_size=224, depth=2), 224)
        assert info["has_cls_token"] is cls and info["num_tokens"] == (224 // patch) ** 2, name
        assert info["heads_per_layer"] == [heads, heads] and info["mlp_ratio"] == 4.0, name
        assert info["attn_subpath"] == "attn" and info["embed_dim"] == dim and info["feature_format"] == "token", name


def test_existing_presets_still_return_imagenet_statistics():
    from basd_amd.models.teacher import load_teacher
    for name in ("vit_tiny_patch16_224", "dinov2_vits14"):
        t = load_teacher(name, 28, device="cpu", dtype=torch.float32, patch_size=14)
        assert t.mean == IMAGENET_MEAN and t.std == IMAGENET_STD and t.has_cls_token is True
    t = load_teacher("resnet50.a1_in1k", 32, device="cpu", dtype=torch.float32)
    assert t.mean == IMAGENET_MEAN and t.std == IMAGENET_STD


def test_overrides_and_unknown_names():
    from basd_amd.models.teacher import load_teacher
    from basd_amd.models.vit import Mlp
    t = load_teacher("vit_tiny_patch16_224", 32, device="cpu", dtype=torch.float32, act="gelu_tanh", norm_eps=1e-5)
    assert t.model.blocks[0].mlp.act_name == "gelu_tanh" and t.model.blocks[0].norm1.eps == 1e-5
    with pytest.raises(ValueError, match="not a known preset"):
        load_teacher("vit_base_patch16_clap_224.openai", 224, device="cpu")
    with pytest.raises(ValueError, match="unknown activation"):
        Mlp(8, 32, "swish")


@pytest.mark.parametrize("pre_norm,act,cls", [(True, "quick_gelu", True), (True, "gelu", True),
                                               (False, "gelu_tanh", False)])
def test_model_equals_the_written_out_fp64_forward(pre_norm, act, cls):
    """depth-2 model in fp64 on the CPU against tests/_clip_ref.py on the same weights: every block's tokens, and the
    importance the blocks' own tap emits against the full softmax map of the reference's hook"""
    from basd_amd.models.teacher import TeacherModel, extract_intermediates, probe_model
    from basd_amd.models.vit import VisionTransformer
    torch.manual_seed(11)
    eps = 1e-5 if pre_norm else 1e-6
    model = VisionTransformer(img_size=32, patch_size=8, num_classes=0, embed_dim=48, depth=2, num_heads=3,
                              class_token=cls, pre_norm=pre_norm, act=act, norm_eps=eps).double().eval()
    with torch.no_grad():
        for p in model.parameters():             # norms off their identity init, a visible CLS token
            p.add_(0.1 * torch.randn_like(p))
    info = probe_model(model, 32)
    teacher = TeacherModel(model=model, embed_dim=48, heads_per_layer=info["heads_per_layer"], depth=2, mlp_ratio=4.0,
                           layer_paths=info["layer_paths"], attn_subpath="attn", has_cls_token=cls,
                           feature_format="token", mean=HALF, std=HALF)
    x = torch.randn(3, 3, 32, 32, dtype=torch.float64)
    toks, imps = extract_intermediates(teacher, x)
    want_t, want_i = clip_forward(fp64_params(model.state_dict()), x, heads=3, act=act, eps=eps)
    for j in range(2):
        torch.testing.assert_close(toks[j], want_t[j][:, int(cls):], rtol=1e-10, atol=1e-10)
        torch.testing.assert_close(imps[j].double(), want_i[j], rtol=1e-5, atol=1e-7)      # the tap's softmax is fp32
