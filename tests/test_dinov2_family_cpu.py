"""The rest of the DINOv2 family (no GPU): register tokens, the SwiGLU MLP of ViT-g/14, presets, state-dict names,
LayerScale folding and the probe record.

The arithmetic is pinned against ``tests/_dinov2_ref.py`` (plain torch, written from the definition of the DINOv2
forward) and against compositions written out in the tests, not against calls into ``models/vit.py``."""
import pytest
import torch
import torch.nn.functional as F

from tests._dinov2_ref import dinov2_forward, embed_reg_emulation, fp64_params, swiglu_unpack_index

# name -> (embed_dim, depth, heads, register tokens, mlp, hidden width)
NEW_PRESETS = {
    "dinov2_vits14_reg": (384, 12, 6, 4, "mlp", 1536),
    "dinov2_vitb14_reg": (768, 12, 12, 4, "mlp", 3072),
    "dinov2_vitl14_reg": (1024, 24, 16, 4, "mlp", 4096),
    "dinov2_vitg14": (1536, 40, 24, 0, "swiglu", 4096),
    "dinov2_vitg14_reg": (1536, 40, 24, 4, "swiglu", 4096),
    "vit_small_patch14_reg4_dinov2": (384, 12, 6, 4, "mlp", 1536),
    "vit_base_patch14_reg4_dinov2": (768, 12, 12, 4, "mlp", 3072),
    "vit_large_patch14_reg4_dinov2": (1024, 24, 16, 4, "mlp", 4096),
    "vit_giant_patch14_dinov2": (1536, 40, 24, 0, "swiglu", 4096),
    "vit_giant_patch14_reg4_dinov2": (1536, 40, 24, 4, "swiglu", 4096),
}


def _tiny(reg_tokens=4, mlp="swiglu", init_values=None, seed=5, hidden=64):
    from basd_amd.models.vit import VisionTransformer
    torch.manual_seed(seed)
    model = VisionTransformer(img_size=28, patch_size=7, num_classes=0, embed_dim=48, depth=2, num_heads=3,
                              init_values=init_values, reg_tokens=reg_tokens, mlp=mlp, mlp_hidden=hidden).eval()
    with torch.no_grad():
        for p in model.parameters():                 # norms and scales off their init, visible CLS / register rows
            p.add_(0.1 * torch.randn_like(p))
    return model


@pytest.mark.parametrize("h", [128, 384])
def test_swiglu_pack_is_the_documented_permutation(h):
    from basd_amd._native import gemm_swiglu_supported, swiglu_pack, swiglu_pack_index
    g = torch.Generator().manual_seed(h)
    k = 64
    w12, b12 = torch.randn(2 * h, k, generator=g), torch.randn(2 * h, generator=g)
    wp, bp = swiglu_pack(w12, b12)
    assert wp.shape == w12.shape and bp.shape == b12.shape and wp.is_contiguous()
    assert sorted(swiglu_pack_index(h).tolist()) == list(range(2 * h))          # a permutation of the rows
    unpack = swiglu_unpack_index(h)                                             # hub row -> packed row, from the header
    assert torch.equal(wp[unpack], w12) and torch.equal(bp[unpack], b12)
    # the product over the packed rows, regrouped by the map: every wave slice of 64 columns = 32 x1 then 32 x2
    x = torch.randn(5, k, generator=g)
    y = (x @ wp.t() + bp).view(5, h // 32, 2, 32)
    x1, x2 = (x @ w12.t() + b12).chunk(2, dim=-1)
    assert torch.equal(y[:, :, 0].reshape(5, h), x1) and torch.equal(y[:, :, 1].reshape(5, h), x2)
    assert swiglu_pack(w12)[1] is None
    assert gemm_swiglu_supported(h, k) and not gemm_swiglu_supported(192, 64) and not gemm_swiglu_supported(128, 96)
    assert not gemm_swiglu_supported(64, 64) and not gemm_swiglu_supported(128, 0)


def test_swiglu_module_is_the_written_out_composition():
    from basd_amd.models.vit import SwiGLU
    torch.manual_seed(2)
    m = SwiGLU(48, 64)
    assert set(m.state_dict()) == {"w12.weight", "w12.bias", "w3.weight", "w3.bias"}
    assert tuple(m.w12.weight.shape) == (128, 48) and tuple(m.w3.weight.shape) == (48, 64)
    x = 2.0 * torch.randn(3, 7, 48)
    x1, x2 = F.linear(x, m.w12.weight, m.w12.bias).chunk(2, dim=-1)
    want = F.linear(F.silu(x1) * x2, m.w3.weight, m.w3.bias)
    with torch.no_grad():
        torch.testing.assert_close(m(x), want, rtol=0, atol=0)
    torch.testing.assert_close(m(x), want, rtol=0, atol=0)          # with autograd on: the same composition
    with pytest.raises(ValueError, match="unknown MLP"):
        from basd_amd.models.vit import Block
        Block(48, 3, mlp="glu")


def test_register_rows_stand_behind_the_cls_row_without_a_position_row():
    model = _tiny(reg_tokens=4, mlp="mlp")
    assert tuple(model.reg_token.shape) == (1, 4, 48) and tuple(model.pos_embed.shape) == (1, 17, 48)
    seen = []
    hook = model.blocks[0].register_forward_pre_hook(lambda mod, inp: seen.append(inp[0]))
    x = torch.randn(3, 3, 28, 28)
    with torch.no_grad():
        out = model.forward_features(x)
        patches = model.patch_embed(x)
    hook.remove()
    h = seen[0]
    assert h.shape == (3, 1 + 4 + 16, 48) and out.shape == (3, 21, 48)
    assert torch.equal(h[:, 1:5], model.reg_token.expand(3, -1, -1))
    want = torch.cat([model.cls_token.expand(3, -1, -1), patches], dim=1) + model.pos_embed
    assert torch.equal(h[:, :1], want[:, :1]) and torch.equal(h[:, 5:], want[:, 1:])
    with pytest.raises(ValueError, match="CLS token"):
        from basd_amd.models.vit import VisionTransformer
        VisionTransformer(img_size=28, patch_size=7, num_classes=0, embed_dim=48, depth=1, num_heads=3,
                          class_token=False, reg_tokens=4)


@pytest.mark.parametrize("reg_tokens,mlp,ls", [(4, "mlp", None), (0, "swiglu", None), (4, "swiglu", 0.5)])
def test_model_equals_the_written_out_fp64_forward(reg_tokens, mlp, ls):
    from basd_amd.models.teacher import TeacherModel, extract_intermediates, probe_model
    model = _tiny(reg_tokens, mlp, ls).double()
    info = probe_model(model, 28)
    teacher = TeacherModel(model=model, embed_dim=48, heads_per_layer=info["heads_per_layer"], depth=2,
                           mlp_ratio=info["mlp_ratio"], layer_paths=info["layer_paths"], attn_subpath="attn",
                           has_cls_token=True, feature_format="token", mean=(0.5,) * 3, std=(0.5,) * 3)
    x = torch.randn(3, 3, 28, 28, dtype=torch.float64)
    toks, imps = extract_intermediates(teacher, x)
    want_t, want_i, want_c = dinov2_forward(fp64_params(model.state_dict()), x, heads=3)
    for j in range(2):
        assert toks[j].shape == (3, reg_tokens + 16, 48) and imps[j].shape == (3, reg_tokens + 16)
        torch.testing.assert_close(toks[j], want_t[j][:, 1:], rtol=1e-10, atol=1e-10)
        torch.testing.assert_close(imps[j].double(), want_i[j], rtol=1e-5, atol=1e-7)
        torch.testing.assert_close(imps[j].double().sum(-1) + want_c[j], torch.ones(3, dtype=torch.float64),
                                   rtol=0, atol=1e-5)


@pytest.mark.parametrize("name", sorted(NEW_PRESETS))
def test_preset_builds_with_the_stated_shape(name):
    from basd_amd.models.vit import Mlp, SwiGLU, create_vit, vit_preset
    dim, depth, heads, reg, mlp, hidden = NEW_PRESETS[name]
    ps = vit_preset(name)
    assert (ps.embed_dim, ps.depth, ps.heads, ps.patch, ps.layerscale) == (dim, depth, heads, 14, 1.0)
    assert (ps.reg_tokens, ps.mlp) == (reg, mlp) and (ps.mlp_hidden or 4 * dim) == hidden
    with torch.device("meta"):                       # shapes and names only: nothing of a ViT-g is allocated
        model = create_vit(name, num_classes=0, img_size=224)
    keys = set(model.state_dict())
    assert ("reg_token" in keys) == (reg > 0) and tuple(model.pos_embed.shape) == (1, 257, dim)
    assert reg == 0 or tuple(model.reg_token.shape) == (1, reg, dim)
    assert len(model.blocks) == depth and tuple(model.patch_embed.proj.weight.shape) == (dim, 3, 14, 14)
    for blk in model.blocks:
        assert blk.attn.num_heads == heads and blk.attn.head_dim == 64 and tuple(blk.ls2.gamma.shape) == (dim,)
        if mlp == "swiglu":
            assert type(blk.mlp) is SwiGLU and tuple(blk.mlp.w12.weight.shape) == (2 * hidden, dim)
            assert tuple(blk.mlp.w3.weight.shape) == (dim, hidden) and not hasattr(blk.mlp, "fc1")
        else:
            assert type(blk.mlp) is Mlp and blk.mlp.fc1.out_features == hidden


def test_existing_presets_and_models_keep_their_tree():
    from basd_amd.models.vit import VIT_PRESETS, Mlp, create_vit, vit_preset
    for name in sorted(set(VIT_PRESETS) - set(NEW_PRESETS)):
        ps = vit_preset(name)
        assert (ps.reg_tokens, ps.mlp, ps.mlp_hidden) == (0, "mlp", None), name
    with torch.device("meta"):
        model = create_vit("dinov2_vitb14", num_classes=0, img_size=224)
    assert model.reg_token is None and "reg_token" not in model.state_dict()
    assert type(model.blocks[0].mlp) is Mlp and model.blocks[0].mlp.fc1.out_features == 3072


def test_hub_and_timm_state_dicts_load_to_the_same_parameters(tmp_path):
    from basd_amd.models.teacher import load_teacher
    from basd_amd.models.vit import dinov2_state_dict
    src = _tiny(4, "swiglu", 0.5, seed=9)
    own = {k: v.clone() for k, v in src.state_dict().items()}
    hub = {("register_tokens" if k == "reg_token" else k): v for k, v in own.items()}
    hub["mask_token"] = torch.zeros(1, 48)
    timm = {k.replace(".mlp.w12.", ".mlp.fc1.").replace(".mlp.w3.", ".mlp.fc2."): v for k, v in own.items()}
    assert "register_tokens" in hub and "reg_token" in timm and "blocks.1.mlp.fc1.weight" in timm
    for state in (hub, timm):
        dst = _tiny(4, "swiglu", 0.5, seed=10)
        missing, unexpected = dst.load_state_dict(dinov2_state_dict(dst, state), strict=False)
        assert not missing and not unexpected, (missing, unexpected)
        for k, v in dst.state_dict().items():
            assert torch.equal(v, own[k]), k
    # a GELU model keeps its fc1 / fc2 keys
    gelu = _tiny(4, "mlp")
    assert set(dinov2_state_dict(gelu, gelu.state_dict())) == set(gelu.state_dict())
    # through load_teacher: a hub-named file for a register preset (two blocks of it would not load: use the names only)
    path = tmp_path / "hub.pt"
    ref = load_teacher("dinov2_vits14_reg", 28, device="cpu", dtype=torch.float32, seed=3)
    state = {("register_tokens" if k == "reg_token" else k): v for k, v in ref.model.state_dict().items()}
    state["mask_token"] = torch.zeros(1, 384)
    torch.save(state, path)
    got = load_teacher("dinov2_vits14_reg", 28, device="cpu", dtype=torch.float32, seed=4, weights=str(path))
    assert torch.equal(got.model.reg_token, ref.model.reg_token)
    assert torch.equal(got.model.blocks[3].mlp.fc2.weight, ref.model.blocks[3].mlp.fc2.weight)


def test_fold_layerscale_folds_ls2_into_w3():
    from basd_amd.models.teacher import fold_layerscale
    from basd_amd.models.vit import LayerScale
    model = _tiny(4, "swiglu", 0.5)
    for p in model.parameters():
        p.requires_grad = False
    assert all(isinstance(b.ls1, LayerScale) and isinstance(b.ls2, LayerScale) for b in model.blocks)
    x = torch.randn(2, 3, 28, 28)
    with torch.no_grad():
        before = model.forward_features(x)
        w3 = model.blocks[0].mlp.w3.weight.clone()
        gamma2 = model.blocks[0].ls2.gamma.clone()
        assert fold_layerscale(model) == 4
        after = model.forward_features(x)
    assert all(isinstance(b.ls1, torch.nn.Identity) and isinstance(b.ls2, torch.nn.Identity) for b in model.blocks)
    assert torch.equal(model.blocks[0].mlp.w3.weight, w3 * gamma2.unsqueeze(1))
    assert float((after - before).abs().max()) <= 1e-6 * max(1.0, float(before.abs().max()))


def test_probe_reports_what_the_reference_probe_reports():
    from basd_amd.models.teacher import load_teacher, probe_model
    info = probe_model(_tiny(4, "swiglu"), 28)
    assert info["has_cls_token"] is True and info["num_tokens"] == 4 + 16
    assert info["mlp_ratio"] == 0.0                  # no fc1 in a SwiGLU block: reference teacher.py:69-76
    assert info["heads_per_layer"] == [3, 3] and info["attn_subpath"] == "attn" and info["feature_format"] == "token"
    info = probe_model(_tiny(4, "mlp", hidden=192), 28)
    assert info["num_tokens"] == 20 and info["mlp_ratio"] == 4.0
    t = load_teacher("vit_small_patch14_reg4_dinov2.lvd142m", 28, device="cpu", dtype=torch.float32)
    assert t.has_cls_token and t.embed_dim == 384 and t.depth == 12 and t.mlp_ratio == 4.0
    assert tuple(t.model.reg_token.shape) == (1, 4, 384) and not t.model.reg_token.requires_grad


@pytest.mark.parametrize("with_cls", [True, False])
def test_embed_emulation_without_registers_is_the_torch_assembly(with_cls):
    g = torch.Generator().manual_seed(17)
    b, n, d = 3, 5, 24
    patches = torch.randn(b, n, d, generator=g).bfloat16()
    cls = torch.randn(d, generator=g).bfloat16() if with_cls else None
    pos = torch.randn(n + int(with_cls), d, generator=g).bfloat16()
    x = patches if cls is None else torch.cat([cls.view(1, 1, d).expand(b, -1, -1), patches], dim=1)
    want = x + pos
    for reg in (None, torch.empty(0, d, dtype=torch.bfloat16)):
        got = embed_reg_emulation(patches, cls, reg, pos)
        assert got.dtype == torch.bfloat16 and torch.equal(got.view(torch.int16), want.view(torch.int16))
    if with_cls:
        reg = torch.randn(2, d, generator=g).bfloat16()
        reg[0, 0] = -0.0                             # a copied row keeps a negative zero
        got = embed_reg_emulation(patches, cls, reg, pos)
        assert got.shape == (b, 1 + 2 + n, d)
        assert torch.equal(got[:, 1:3].view(torch.int16), reg.expand(b, -1, -1).contiguous().view(torch.int16))
        assert torch.equal(got[:, :1], want[:, :1]) and torch.equal(got[:, 3:], want[:, 1:])
