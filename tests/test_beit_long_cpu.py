"""BEiT teachers past 272 tokens, host side (no GPU): the 384 px presets, the choice between the short entry, the tiled
one and the torch path in ``RelPosAttention.forward``, the range predicate and the index rule."""
import pytest
import torch

HALF = (0.5, 0.5, 0.5)
PRESETS = {"beit_base_patch16_384": (768, 12, 12), "beit_large_patch16_384": (1024, 24, 16)}


@pytest.mark.parametrize("name", sorted(PRESETS))
def test_384_presets_are_the_224_architectures_with_half_statistics(name):
    from basd_amd.models.beit import BEIT_PRESETS, create_beit
    dim, depth, heads = PRESETS[name]
    assert BEIT_PRESETS[name][:4] == (dim, depth, heads, 16) and BEIT_PRESETS[name][5:] == (HALF, HALF)
    assert BEIT_PRESETS[name] == BEIT_PRESETS[name.replace("_384", "_224")]
    with torch.device("meta"):                   # shapes and names only: nothing of a ViT-L is allocated
        model = create_beit(name, img_size=384)
    assert model.grid == (24, 24) and len(model.blocks) == depth and model.embed_dim == dim
    for blk in model.blocks:
        assert blk.attn.num_heads == heads and blk.attn.head_dim == 64
        assert tuple(blk.attn.relative_position_bias_table.shape) == (47 * 47 + 3, heads)


def test_load_teacher_resolves_the_384_names_and_not_the_512_one():
    """the name table of ``load_teacher`` (a small image keeps the CPU forward of the probe short: the preset, not the
    grid, is what is looked up)"""
    from basd_amd.models.beit import Beit
    from basd_amd.models.teacher import load_teacher
    for name, (dim, depth, heads) in PRESETS.items():
        t = load_teacher(name + ".in22k_ft_in22k_in1k", 32, device="cpu", dtype=torch.float32)
        assert isinstance(t.model, Beit) and t.model.grid == (2, 2)
        assert t.embed_dim == dim and t.depth == depth and t.heads_per_layer == [heads] * depth
        assert t.mean == HALF and t.std == HALF and t.has_cls_token is True
    with pytest.raises(ValueError, match="not a known preset"):
        load_teacher("beit_large_patch16_512", 512, device="cpu")


class _Recorder:
    """a provider that takes every tensor and records which attention entry the module chose"""

    def __init__(self):
        import basd_amd._native as native
        self.calls = []
        self.attention_fwd_relbias_supported = native.attention_fwd_relbias_supported
        self.attention_fwd_long_relbias_supported = native.attention_fwd_long_relbias_supported

    def handles(self, t):
        return True

    def gemm_supported(self, n, k):
        return False

    wgrad_supported = gemm_supported

    def _fwd(self, name, qkv, table, gh, gw, heads, head_dim, scale, want_importance=False):
        assert table.dtype == torch.float32 and tuple(table.shape) == ((2 * gh - 1) * (2 * gw - 1) + 3, heads)
        self.calls.append((name, qkv.shape[1], want_importance))
        imp = torch.zeros(qkv.shape[0], qkv.shape[1] - 1) if want_importance else None
        return torch.zeros(qkv.shape[0], qkv.shape[1], heads * head_dim, dtype=qkv.dtype), imp

    def attention_fwd_relbias(self, *args, **kwargs):
        return self._fwd("short", *args, **kwargs)

    def attention_fwd_long_relbias(self, *args, **kwargs):
        return self._fwd("long", *args, **kwargs)


@pytest.mark.parametrize("grid,head_dim,want", [((16, 16), 64, "short"), ((17, 17), 64, "long"), ((24, 24), 64, "long"),
                                                ((32, 32), 64, None), ((17, 17), 80, None)])
def test_relpos_attention_chooses_the_entry_by_grid_and_head_dim(monkeypatch, grid, head_dim, want):
    """frozen, bf16, fp32 table, CLS tap: the short entry where it applies, the tiled one up to 1024 tokens, the counted
    library fallback past that, for another head dim and whenever the switch is off or gradients are on"""
    import basd_amd.losses._ops as O
    import basd_amd.models.beit as B
    t = grid[0] * grid[1] + 1
    attn = B.RelPosAttention(head_dim, 1, window_size=grid).to(torch.bfloat16).eval()
    attn.materialize_qkv_bias()
    for p in attn.parameters():
        p.requires_grad = False
    assert attn.relative_position_bias_table.dtype == torch.float32
    rec = _Recorder()
    O.set_ops(rec)
    O.FALLBACKS.clear()
    try:
        x = torch.zeros(1, t, head_dim, dtype=torch.bfloat16)
        attn.tap = {"has_cls": True, "out": None}
        with torch.no_grad():
            attn(x)
        assert rec.calls == ([(want, t, True)] if want else []), rec.calls
        assert O.FALLBACKS.get("attention (relative bias)", 0) == (0 if want else 1)
        attn.tap = None
        with torch.no_grad():
            attn(x)
        assert rec.calls[1:] == ([(want, t, False)] if want else [])
        if want:           # gradients enabled, or the switch off: the library path, counted
            before = len(rec.calls)
            O.FALLBACKS.clear()
            attn(x)
            monkeypatch.setattr(B, "_FUSED_RELBIAS_ATTENTION", False)
            with torch.no_grad():
                attn(x)
            assert len(rec.calls) == before and O.FALLBACKS["attention (relative bias)"] == 2
    finally:
        O.set_ops(None)
        O.FALLBACKS.clear()


def test_long_predicate_on_its_boundaries():
    from basd_amd._native import LONG_ATTENTION_MAX_T, attention_fwd_long_relbias_supported as ok
    assert LONG_ATTENTION_MAX_T == 1024
    assert ok(1, 1, 64) and ok(16, 16, 64) and ok(16, 17, 64) and ok(24, 24, 64)
    assert ok(31, 33, 64) and ok(1, 1023, 64) and ok(1023, 1, 64)
    assert not ok(32, 32, 64) and not ok(1, 1024, 64)                 # 1025 tokens
    assert not ok(0, 5, 64) and not ok(5, 0, 64) and not ok(-1, -5, 64)
    assert not ok(14, 14, 80) and not ok(24, 24, 32)


def test_closed_form_index_is_the_index_buffer_on_a_3_by_5_grid():
    """the rule the kernels evaluate per logit and the buffer the torch path gathers with stay one rule"""
    from basd_amd._native import relbias_index
    from basd_amd.models.beit import relative_position_index
    gh, gw = 3, 5
    want = relative_position_index(gh, gw)
    t = gh * gw + 1
    got = torch.tensor([[relbias_index(i, j, gh, gw) for j in range(t)] for i in range(t)])
    assert torch.equal(got, want)
    assert int(want.max()) == (2 * gh - 1) * (2 * gw - 1) + 2 and int(want.min()) == 0


def test_export_is_declared_and_bound():
    import basd_amd._native as native
    assert "basd_attention_fwd_long_relbias_bf16" in native.EXPORTS
    assert len(native._SIGNATURES["basd_attention_fwd_long_relbias_bf16"]) == 11
