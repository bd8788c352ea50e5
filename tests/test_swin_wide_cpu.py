"""Swin teachers with windows 9 .. 16 without a GPU: the window-12 / Swin-L presets, the index arithmetic of the wide
window attention kernel against the module's index buffer, the fused path's choice of attention entry per block with the
kernels emulated in plain torch (tests/_swin_wide_emul.py), and what is refused at load."""
import pytest
import torch

from tests import _swin_emul, _swin_ref as R, _swin_wide_emul

SWIN_B, SWIN_L = ((2, 2, 18, 2), (128, 256, 512, 1024), (4, 8, 16, 32)), ((2, 2, 18, 2), (192, 384, 768, 1536), (6, 12, 24, 48))


@pytest.fixture
def wide_kernels():
    from basd_amd.losses import _ops
    _ops.set_ops(_swin_wide_emul)
    yield _swin_wide_emul
    _ops.set_ops(None)


@pytest.fixture
def narrow_kernels():
    """the provider of the existing Swin tests: it has no wide entry"""
    from basd_amd.losses import _ops
    assert not hasattr(_swin_emul, "window_attention_wide")
    _ops.set_ops(_swin_emul)
    yield _swin_emul
    _ops.set_ops(None)


@pytest.mark.parametrize("name,arch,ws", [("swin_base_patch4_window12_384", SWIN_B, 12),
                                          ("swin_large_patch4_window12_384", SWIN_L, 12),
                                          ("swin_large_patch4_window7_224", SWIN_L, 7)])
def test_presets_have_the_published_shapes(name, arch, ws):
    from basd_amd.models.cnn import CNN_PRESETS
    depths, dims, heads = arch
    model = CNN_PRESETS[name]()
    state = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert state == R.expected_state(depths, dims, heads, ws)
    assert state["layers.0.blocks.0.attn.relative_position_bias_table"] == ((2 * ws - 1) ** 2, heads[0])
    if ws == 12:
        assert (2 * ws - 1) ** 2 == 529
    assert model.window_size == ws and model.embed_dim == model.num_features == dims[-1]
    assert all(c == 32 * h for c, h in zip(dims, heads))
    assert [b.shift for b in model.layers[2].blocks] == [0, ws // 2] * (depths[2] // 2)
    assert [b.window_size for s in model.layers for b in s.blocks] == [ws] * sum(depths)


@pytest.mark.parametrize("name", ["swin_base_patch4_window12_384", "swin_large_patch4_window12_384",
                                  "swin_large_patch4_window7_224"])
def test_every_stage_of_the_new_presets_passes_the_gates(wide_kernels, name):
    """Swin-L: qkv width 576 -> 640, merge 4 C = 3072; nothing of the 192 / 384 / 768 / 1536 stages is refused"""
    from basd_amd.models.cnn import CNN_PRESETS
    model = CNN_PRESETS[name]()
    assert model.fused_refusal() is None
    if model.dims[0] == 192:
        assert model._qkv_width(192, 192) == 640


@pytest.mark.parametrize("ws", range(9, 17))
def test_kernel_index_formula_is_the_modules_index(ws):
    """csrc/swin_wide.hip: a slot carries koff = iy (2 ws - 1) + ix, a query reads row cbase + koff_q - koff_k of the
    table with cbase = (ws - 1)(2 ws - 1) + ws - 1; every row lies inside the table"""
    from basd_amd.models.swin import relative_position_index
    tw = 2 * ws - 1
    slot = torch.arange(ws * ws)
    koff = (slot // ws) * tw + slot % ws
    idx = (ws - 1) * tw + ws - 1 + koff[:, None] - koff[None, :]
    assert torch.equal(idx, relative_position_index(ws)) and torch.equal(idx, R.bias_index(ws))
    assert int(idx.min()) == 0 and int(idx.max()) == tw * tw - 1


def _bf16_teacher(model):
    model = model.to(torch.bfloat16)
    for m in model.modules():
        if isinstance(m, torch.nn.LayerNorm):
            m.float()
    for p in model.parameters():
        p.requires_grad = False
    return model.eval()


def _spy(monkeypatch, provider):
    calls = []
    for name in ("window_attention", "window_attention_wide"):
        fn = getattr(provider, name)

        def spy(*a, _fn=fn, _name=name, **k):
            calls.append((_name, a[0].shape[1], a[2], a[3], tuple(a[1].shape)))
            return _fn(*a, **k)
        monkeypatch.setattr(provider, name, spy)
    return calls


def test_window_12_model_takes_the_wide_entry_in_every_block(wide_kernels, monkeypatch):
    """384 px is the smallest image window 12 fits: grids 96, 48, 24, 12 -- a shifted second block in stages 1-3, one
    unshifted window in stage 4.  Every block calls the wide entry with the fp32 table [529, heads]; the 64-slot entry is
    never called.  Agreement with the plain path as in tests/test_swin_cpu.py: against the fp64 restatement the fused
    path's error is at most twice the plain bf16 path's, and at most the 3.6e-2 derived there for 8 blocks."""
    from basd_amd.models.swin import SwinTransformer
    depths, dims, heads = (2, 2, 2, 2), (64, 128, 256, 512), (2, 4, 8, 16)
    torch.manual_seed(1)
    model = _bf16_teacher(R.randomise_affine(SwinTransformer(depths, dims, heads, window_size=12), seed=11))
    assert model.fused_refusal() is None and model.prepare_fused()
    blk = model._fused["stages"][1]["blocks"][0]
    assert blk["bias"].shape == (529, 4) and blk["bias"].dtype == torch.float32
    assert torch.equal(blk["bias"], model.layers[1].blocks[0].attn.relative_position_bias_table.float())
    calls = _spy(monkeypatch, wide_kernels)
    x = torch.randn(1, 3, 384, 384).to(torch.bfloat16)
    with torch.no_grad():
        got = model.forward_features(x)
        plain = model._forward_plain(x)
    assert got.shape == plain.shape == (1, 12, 12, 512) and got.dtype == torch.bfloat16
    assert {c[0] for c in calls} == {"window_attention_wide"}
    assert [c[1:4] for c in calls] == [(96, 12, 0), (96, 12, 6), (48, 12, 0), (48, 12, 6), (24, 12, 0), (24, 12, 6),
                                       (12, 12, 0), (12, 12, 0)]
    assert [c[4] for c in calls] == [(529, h) for h in heads for _ in range(2)]
    want = R.forward_features(model.state_dict(), x, depths, heads, 12)
    err = float(R.rel_l2_per_sample(got, want).max())
    err_plain = float(R.rel_l2_per_sample(plain, want).max())
    print(f"fused (emulated, window 12) vs fp64 {err:.3e}, plain bf16 vs fp64 {err_plain:.3e}")
    assert err <= 2.0 * err_plain, (err, err_plain)
    assert err <= 3.6e-2, err


def test_window_4_model_still_takes_the_64_slot_entry(wide_kernels, monkeypatch):
    from basd_amd.models.swin import SwinTransformer
    torch.manual_seed(1)
    model = _bf16_teacher(SwinTransformer((2, 2, 2, 2), (64, 128, 256, 512), (2, 4, 8, 16), window_size=4))
    assert model.prepare_fused() and model._fused["stages"][0]["blocks"][0]["bias"].shape == (2, 64, 64)
    calls = _spy(monkeypatch, wide_kernels)
    with torch.no_grad():
        model.forward_features(torch.randn(1, 3, 128, 128).to(torch.bfloat16))
    assert len(calls) == 8 and {c[0] for c in calls} == {"window_attention"}


def test_provider_without_the_wide_entry_names_stage_and_window(narrow_kernels):
    """window 12 on a provider that only has the 64-slot entry: a refusal with the stage and the window, no weight
    images; window 4 on the same provider is accepted as before"""
    from basd_amd.models.swin import SwinTransformer
    model = _bf16_teacher(SwinTransformer((1, 1, 1, 1), (64, 128, 256, 512), (2, 4, 8, 16), window_size=12))
    why = model.fused_refusal()
    assert why is not None and "stage 0" in why and "window 12" in why
    assert not model.prepare_fused() and model._fused is None
    ok = _bf16_teacher(SwinTransformer((1, 1, 1, 1), (64, 128, 256, 512), (2, 4, 8, 16), window_size=4))
    assert ok.fused_refusal() is None and ok.prepare_fused()


def test_window_above_16_is_refused_with_the_stage_named(wide_kernels):
    from basd_amd.models.swin import SwinTransformer
    why = SwinTransformer((1, 1, 1, 1), (64, 128, 256, 512), (2, 4, 8, 16), window_size=17).fused_refusal()
    assert why is not None and "stage 0" in why and "window 17" in why


def test_window_12_preset_at_224px_fails_at_load():
    from basd_amd.models import load_teacher
    with pytest.raises(ValueError, match=r"image size 224.*window 12"):
        load_teacher("swin_base_patch4_window12_384.ms_in22k_ft_in1k", 224, device="cpu", dtype=torch.float32)


def test_checkpoint_of_another_window_fails_at_load():
    """a window-7 checkpoint (169-row tables) into a window-12 model: refused, tables are not resampled"""
    from basd_amd.models.swin import SwinTransformer
    arch = ((1, 1, 1, 1), (64, 128, 256, 512), (2, 4, 8, 16))
    state = SwinTransformer(*arch, window_size=7).state_dict()
    with pytest.raises(ValueError, match=r"169 rows.*window 12.*529"):
        SwinTransformer(*arch, window_size=12).load_state_dict(state, strict=False)
    SwinTransformer(*arch, window_size=7).load_state_dict(state, strict=True)
