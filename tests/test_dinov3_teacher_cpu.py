"""DINOv3 teachers without a GPU: the presets and the loader, the rotary table rule, the model arithmetic on the CPU
path after the q / k row permutation, the checkpoint key mapping, and the dispatch between the two rotary attention
entries.

The arithmetic is pinned against ``tests/_dinov3_ref.py``: an fp64 forward in DINOv3's own form (half-split pairs through
``rotate_half``, tiled angles, unpermuted weights, the k bias masked, LayerScale explicit), not the interleaved table
and permuted weights the model and the kernels use."""
import ctypes
import os
import re
import types

import pytest
import torch

from tests._dinov3_ref import (BATCH, DEPTH, DIM, HD, HEADS, PATCH, REG, dinov3_angles, dinov3_forward, fp64_params,
                               hub_state_dict, rope_apply, timm_names, tiny_dinov3)

IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "basd_hip.h")
ENTRY = "basd_attention_fwd_long_rope_bf16"
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
    return TeacherModel(model=model, embed_dim=DIM, heads_per_layer=[HEADS] * DEPTH, depth=DEPTH, mlp_ratio=4.0,
                        layer_paths=[f"blocks.{i}" for i in range(DEPTH)], attn_subpath="attn", has_cls_token=True,
                        feature_format="token", mean=IMAGENET_MEAN, std=IMAGENET_STD)


def test_load_teacher_builds_dinov3_small_and_probes_it(host_only):
    """today's ``ValueError: not a known preset``; the hub alias and a tagged name resolve to the same preset"""
    from basd_amd.models.dinov3 import DINOV3_PRESETS, Dinov3
    from basd_amd.models.teacher import load_teacher
    t = load_teacher("vit_small_patch16_dinov3", 32, device="cpu", dtype=torch.float32)
    assert isinstance(t.model, Dinov3)
    assert t.embed_dim == 384 and t.depth == 12 and t.heads_per_layer == [6] * 12 and t.has_cls_token is True
    assert t.feature_format == "token" and t.attn_subpath == "attn" and t.mlp_ratio == 4.0
    assert t.mean == IMAGENET_MEAN and t.std == IMAGENET_STD
    assert t.layer_paths == [f"blocks.{i}" for i in range(12)]
    assert not any(p.requires_grad for p in t.model.parameters()) and not t.model.training
    blk = t.model.blocks[0]
    assert blk.attn.head_dim == 64 and blk.norm1.eps == 1e-5 and blk.mlp.fc1.out_features == 4 * 384
    assert isinstance(blk.ls1, torch.nn.Identity) and isinstance(blk.ls2, torch.nn.Identity)      # folded
    assert blk.attn.pairs_interleaved and not bool(blk.attn.qkv.bias[384:768].any())            # the k bias is masked
    assert tuple(blk.attn.rope.shape) == (1 + 4 + 4, 32, 2) and blk.attn.rope.dtype == torch.float32
    assert tuple(t.model.reg_token.shape) == (1, 4, 384) and not hasattr(t.model, "pos_embed")
    for alias in ("dinov3_vits16", "vit_small_patch16_dinov3.lvd1689m"):
        a = load_teacher(alias, 32, device="cpu", dtype=torch.float32)
        assert (a.embed_dim, a.depth, a.heads_per_layer) == (384, 12, [6] * 12)
    assert DINOV3_PRESETS["dinov3_vits16"] is DINOV3_PRESETS["vit_small_patch16_dinov3"]
    assert DINOV3_PRESETS["vit_base_patch16_dinov3"][:4] == (768, 12, 12, 16) == DINOV3_PRESETS["dinov3_vitb16"][:4]
    assert DINOV3_PRESETS["vit_large_patch16_dinov3"][:4] == (1024, 24, 16, 16) == DINOV3_PRESETS["dinov3_vitl16"][:4]
    with pytest.raises(ValueError, match="not a known preset.*vit_base_patch16_dinov3"):
        load_teacher("vit_huge_plus_patch16_dinov3", 32, device="cpu")


def test_bf16_cast_keeps_the_table_and_the_norms_in_fp32(host_only):
    from basd_amd.models.teacher import load_teacher
    t = load_teacher("dinov3_vits16", 32, device="cpu")
    blk = t.model.blocks[0]
    assert blk.attn.qkv.weight.dtype == torch.bfloat16 and blk.attn.rope.dtype == torch.float32
    assert blk.norm1.weight.dtype == torch.float32 and t.model.zero_pos.dtype == torch.bfloat16
    assert not bool(t.model.zero_pos.any()) and not any("rope" in k or "zero_pos" in k for k in t.model.state_dict())


@pytest.mark.parametrize("gh,gw", [(2, 3), (14, 14)])
def test_table_equals_the_reference_angles(gh, gw):
    """the per-pair (cos, sin) table applied the model's way to interleaved channels against DINOv3's tiled angles applied
    through rotate_half to the same vectors in half-split order, in fp64: the table is fp32 (relative 6e-8 on values
    <= 1), the vectors N(0, 1) -> 1e-6 absolute"""
    from basd_amd._native import dinov3_rope_table
    from basd_amd.models.eva import apply_rope
    table = dinov3_rope_table(gh, gw, HD)
    n = gh * gw
    assert table.dtype == torch.float32 and tuple(table.shape) == (5 + n, HD // 2, 2) and table.device.type == "cpu"
    assert torch.equal(table[:5], torch.tensor([1.0, 0.0]).expand(5, HD // 2, 2))             # prefix rows: identity
    angles = dinov3_angles(gh, gw, HD)
    assert float((table[5:, :, 0].double() - angles[:, :HD // 2].cos()).abs().max()) < 1e-6
    assert float((table[5:, :, 1].double() - angles[:, :HD // 2].sin()).abs().max()) < 1e-6
    x = torch.randn(2, 3, n, HD, dtype=torch.float64, generator=torch.Generator().manual_seed(gh * 100 + gw))
    want = rope_apply(x, angles)                                                             # half-split order
    inter = torch.stack([x[..., :HD // 2], x[..., HD // 2:]], dim=-1).flatten(-2)            # 2 i <- i, 2 i + 1 <- i + hd / 2
    got = apply_rope(inter, table[5:])
    assert float((got[..., 0::2] - want[..., :HD // 2]).abs().max()) < 1e-6
    assert float((got[..., 1::2] - want[..., HD // 2:]).abs().max()) < 1e-6
    # other prefixes, another base
    assert torch.equal(dinov3_rope_table(gh, gw, HD, prefix_tokens=0), table[5:])
    assert torch.equal(dinov3_rope_table(gh, gw, HD, prefix_tokens=1)[1:], table[5:])
    assert float((dinov3_rope_table(gh, gw, HD, base=10.0) - table).abs().max()) > 0.1


def test_first_patch_angles_by_hand():
    """2 x 2 grid: patch (0, 0) sits at (-0.5, -0.5); pair j < 16 has the angle -pi / 100^(j / 16) from y, pairs 16 .. 31
    the same from x"""
    from basd_amd._native import dinov3_rope_table
    t = dinov3_rope_table(2, 2, 64, prefix_tokens=0)
    want = -torch.pi / 100.0 ** (torch.arange(16, dtype=torch.float64) / 16)
    for half in (slice(0, 16), slice(16, 32)):
        assert torch.allclose(t[0, half, 0].double(), want.cos(), atol=1e-7)
        assert torch.allclose(t[0, half, 1].double(), want.sin(), atol=1e-7)
    # patch (0, 1): y = -0.5, x = +0.5
    assert torch.allclose(t[1, :16, 1].double(), want.sin(), atol=1e-7)
    assert torch.allclose(t[1, 16:, 1].double(), (-want).sin(), atol=1e-7)


@pytest.mark.parametrize("names", ["hub", "timm"])
@pytest.mark.parametrize("gh,gw", [(2, 3), (4, 4)])
def test_tiny_model_in_fp32_equals_the_fp64_reference(host_only, names, gh, gw):
    """fp32 model with permuted weights, fp64 reference in DINOv3's own form.  Bound: that of
    tests/test_eva_teacher_cpu.py for the same comparison (fp32 dot products of at most 768 terms, unit roundoff 6e-8, a
    handful of products per block, two blocks -> 2e-5 in relative L2 per layer; the taps rtol 1e-3, atol 1e-6)."""
    from basd_amd.models.dinov3 import Dinov3, load_dinov3_state_dict
    from basd_amd.models.teacher import extract_intermediates
    hub = hub_state_dict()
    assert bool(hub["blocks.0.attn.qkv.bias"][DIM:2 * DIM].any())          # a non-zero k bias under the mask
    state = hub if names == "hub" else timm_names(hub)
    assert ("reg_token" in state) == (names == "timm") and ("blocks.0.gamma_1" in state) == (names == "timm")
    model = Dinov3(img_size=PATCH, patch_size=PATCH, embed_dim=DIM, depth=DEPTH, num_heads=HEADS, reg_tokens=REG)
    # a non-square grid: the model's own grid is square, the attention takes any table
    model = _with_grid(model, gh, gw)
    assert load_dinov3_state_dict(model, state) == []
    model.eval()
    x = torch.randn(BATCH, 3, gh * PATCH, gw * PATCH, generator=torch.Generator().manual_seed(2))
    want_t, want_i = dinov3_forward(fp64_params(hub), x)
    toks, imps = extract_intermediates(_teacher(model), x)
    for j in range(DEPTH):
        assert toks[j].shape == (BATCH, REG + gh * gw, DIM) and imps[j].shape == (BATCH, REG + gh * gw)
        err = float((toks[j].double() - want_t[j][:, 1:]).norm() / want_t[j][:, 1:].norm())
        assert err < 2e-5, (j, err)
        torch.testing.assert_close(imps[j].double(), want_i[j], rtol=1e-3, atol=1e-6)
    # the rotation and the k-bias mask are seen by the check: the reference without either is far away
    plain, _ = dinov3_forward(fp64_params(hub), x, rotate=False)
    assert float((plain[0] - want_t[0]).norm() / want_t[0].norm()) > 1e-3
    # permuting twice changes nothing
    before = {k: v.clone() for k, v in model.state_dict().items()}
    model.interleave_rope_pairs()
    assert all(torch.equal(v, model.state_dict()[k]) for k, v in before.items())
    # LayerScale folded (what load_teacher does) is the same forward to fp32 rounding
    from basd_amd.models.teacher import fold_layerscale
    for p in model.parameters():
        p.requires_grad = False
    assert fold_layerscale(model) == 2 * DEPTH
    toks2, _ = extract_intermediates(_teacher(model), x)
    for j in range(DEPTH):
        assert float((toks2[j].double() - want_t[j][:, 1:]).norm() / want_t[j][:, 1:].norm()) < 2e-5


def _with_grid(model, gh, gw):
    """the tiny model with the tables and the zero position rows of a gh x gw grid (``Dinov3`` builds square grids)"""
    from basd_amd._native import dinov3_rope_table
    for blk in model.blocks:
        blk.attn.grid = (gh, gw)
        blk.attn.rope = dinov3_rope_table(gh, gw, HD, prefix_tokens=1 + REG)
    model.zero_pos = torch.zeros(1, 1 + gh * gw, DIM)
    return model


def test_permutation_moves_q_and_k_rows_only(host_only):
    hub = hub_state_dict()
    model = tiny_dinov3(32, hub)
    w, b = hub["blocks.1.attn.qkv.weight"], hub["blocks.1.attn.qkv.bias"]
    attn = model.blocks[1].attn
    for part in (0, 1):                                  # q and k
        for head in range(HEADS):
            o = part * DIM + head * HD
            for i in (0, 1, 17, 31):
                assert torch.equal(attn.qkv.weight[o + 2 * i], w[o + i])
                assert torch.equal(attn.qkv.weight[o + 2 * i + 1], w[o + i + HD // 2])
                if part == 0:
                    assert attn.qkv.bias[o + 2 * i] == b[o + i] and attn.qkv.bias[o + 2 * i + 1] == b[o + i + HD // 2]
    assert torch.equal(attn.qkv.weight[2 * DIM:], w[2 * DIM:]) and torch.equal(attn.qkv.bias[2 * DIM:], b[2 * DIM:])
    assert not bool(attn.qkv.bias[DIM:2 * DIM].any())
    assert torch.equal(attn.proj.weight, hub["blocks.1.attn.proj.weight"])
    assert torch.equal(model.reg_token, hub["storage_tokens"])


def test_an_unknown_key_raises_and_ignored_keys_are_dropped(host_only):
    from basd_amd.models.dinov3 import dinov3_state_dict, load_dinov3_state_dict
    hub = hub_state_dict()
    mapped = dinov3_state_dict(hub)
    assert not any("bias_mask" in k or "rope_embed" in k or k in ("mask_token", "storage_tokens") for k in mapped)
    model = tiny_dinov3(32, hub)
    broken = dict(hub)
    broken["blocks.0.attn.rel_pos"] = torch.zeros(3)
    with pytest.raises(ValueError, match="without a counterpart.*blocks.0.attn.rel_pos"):
        load_dinov3_state_dict(model, broken)
    with pytest.raises(ValueError, match="10 tokens.*9 tokens"):       # the forward refuses another token count
        model.blocks[0].attn(torch.zeros(1, 10, DIM))


def test_load_teacher_reads_a_hub_checkpoint(tmp_path, host_only):
    from basd_amd.models.teacher import load_teacher
    torch.manual_seed(11)
    from basd_amd.models.dinov3 import create_dinov3
    src = create_dinov3("dinov3_vits16", img_size=32)
    state = {("storage_tokens" if k == "reg_token" else k): v.clone() for k, v in src.state_dict().items()}
    state["rope_embed.periods"] = torch.zeros(16)
    path = tmp_path / "dinov3.pt"
    torch.save(state, path)
    t = load_teacher("dinov3_vits16", 32, weights=str(path), device="cpu", dtype=torch.float32)
    w = src.blocks[3].attn.qkv.weight
    assert torch.equal(t.model.blocks[3].attn.qkv.weight[0], w[0]) and torch.equal(t.model.blocks[3].attn.qkv.weight[1], w[32])
    assert torch.equal(t.model.blocks[3].attn.qkv.weight[768:], w[768:])


# ---------------------------------------------------------------------------------------------------------------------
# the two rotary attention entries: ranges, declaration, dispatch

def test_predicates_over_their_ranges():
    import basd_amd._native as native
    for t in range(0, 1100):
        assert native.attention_fwd_rope_supported(t, 64) == (2 <= t <= 272), t
        assert native.attention_fwd_long_rope_supported(t, 64) == (2 <= t <= 1024), t
    for hd in (32, 80, 128):
        assert not native.attention_fwd_long_rope_supported(300, hd) and not native.attention_fwd_rope_supported(100, hd)


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


@pytest.mark.parametrize("b,t,h,hd,table", [(2, 300, 2, 80, True), (2, 1, 2, 64, True), (2, 1025, 2, 64, True),
                                            (2, 300, 2, 64, False), (2, 300, 0, 64, True), (0, 300, 2, 64, True)])
def test_refused_arguments_return_err_shape_before_anything_touches_a_device(lib, b, t, h, hd, table):
    p = lambda on: ctypes.c_void_p(4096 if on else 0)       # never dereferenced on the host
    rc = lib.basd_attention_fwd_long_rope_bf16(p(True), p(table), b, t, h, hd, ctypes.c_float(0.125), p(True), p(False),
                                               p(False))
    assert rc == 1                                   # BASD_ERR_SHAPE
    msg = lib.basd_last_error().decode()
    assert "attention_fwd_long_rope" in msg and f"T={t}" in msg and f"hd={hd}" in msg and ("NULL" in msg) == (not table)


class _Recorder:
    """a provider that takes every tensor and records which attention entry the module chose"""

    def __init__(self):
        import basd_amd._native as native
        self.calls = []
        self.attention_fwd_rope_supported = native.attention_fwd_rope_supported
        self.attention_fwd_long_rope_supported = native.attention_fwd_long_rope_supported

    def handles(self, t):
        return True

    def gemm_supported(self, n, k):
        return False

    wgrad_supported = gemm_supported

    def _fwd(self, name, qkv, rope, heads, head_dim, scale, want_importance=False):
        self.calls.append((name, qkv.shape[1], want_importance))
        imp = torch.zeros(qkv.shape[0], qkv.shape[1] - 1) if want_importance else None
        return torch.zeros(qkv.shape[0], qkv.shape[1], heads * head_dim, dtype=qkv.dtype), imp

    def attention_fwd_rope(self, *a, **k):
        return self._fwd("short", *a, **k)

    def attention_fwd_long_rope(self, *a, **k):
        return self._fwd("long", *a, **k)


@pytest.mark.parametrize("t,want", [(2, "short"), (272, "short"), (273, "long"), (581, "long"), (1024, "long"),
                                    (1025, None)])
def test_rope_attention_chooses_the_entry_by_token_count(monkeypatch, t, want):
    """frozen, bf16, fp32 table, CLS tap: the short entry where it applies, the long one up to 1024 tokens, the counted
    library fallback past that and whenever the switch is off"""
    import basd_amd.losses._ops as O
    import basd_amd.models.eva as E
    from basd_amd.models.eva import RopeAttention
    attn = RopeAttention(64, 1, grid=(1, t - 1)).to(torch.bfloat16).eval()
    attn.materialize_qkv_bias()
    for p in attn.parameters():
        p.requires_grad = False
    assert attn.rope.dtype == torch.float32 and attn.rope.shape[0] == t
    rec = _Recorder()
    O.set_ops(rec)
    O.FALLBACKS.clear()
    try:
        x = torch.zeros(1, t, 64, dtype=torch.bfloat16)
        attn.tap = {"has_cls": True, "out": None}
        with torch.no_grad():
            attn(x)
        assert rec.calls == ([(want, t, True)] if want else []), rec.calls
        assert O.FALLBACKS.get("attention (rope)", 0) == (0 if want else 1)
        attn.tap = None
        with torch.no_grad():
            attn(x)
        assert rec.calls[1:] == ([(want, t, False)] if want else [])
        # gradients enabled, or the switch off: the library path, counted
        before = len(rec.calls)
        O.FALLBACKS.clear()
        attn(x)
        monkeypatch.setattr(E, "_FUSED_EVA_DISPATCH", False)
        with torch.no_grad():
            attn(x)
        assert len(rec.calls) == before and O.FALLBACKS["attention (rope)"] == 2
    finally:
        O.set_ops(None)
        O.FALLBACKS.clear()
