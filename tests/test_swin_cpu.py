"""Swin teacher without a GPU: preset / loader / probe, the architecture against the independent fp64 restatement
(tests/_swin_ref.py), properties of the window index and the shift mask that do not share the product's formulation, the
state-dict layouts, and the fused path's host logic (weight images, padded rows, shift bookkeeping) with the trunk
kernels emulated in plain torch (tests/_swin_emul.py)."""
import re

import pytest
import torch
import torch.nn.functional as F

from tests import _swin_emul, _swin_ref as R

SMALL = dict(depths=(2, 2, 2, 2), dims=(32, 64, 128, 256), heads=(1, 2, 4, 8), window_size=4)


@pytest.fixture
def emulated_kernels():
    from basd_amd.losses import _ops
    _ops.set_ops(_swin_emul)
    yield _swin_emul
    _ops.set_ops(None)


def test_preset_with_pretrained_tag_loads_and_probes():
    """timm's name with its tag: the tag is dropped, the probe finds the four stages in the ``layers`` container and an
    NHWC map, the tap is one layer of 7 x 7 tokens x 768 with uniform importance"""
    from basd_amd.models import extract_intermediates, load_teacher
    teacher = load_teacher("swin_tiny_patch4_window7_224.ms_in1k", 224, device="cpu", dtype=torch.float32)
    assert teacher.layer_paths == [f"layers.{i}" for i in range(4)] and teacher.depth == 4
    assert teacher.feature_format == "nhwc" and teacher.heads_per_layer == [1] and teacher.embed_dim == 768
    assert teacher.attn_subpath is None and teacher.has_cls_token is False
    assert not any(p.requires_grad for p in teacher.model.parameters())
    tok, imp = extract_intermediates(teacher, torch.randn(2, 3, 224, 224))
    assert list(tok) == [0] and tok[0].shape == (2, 49, 768) and tok[0].is_contiguous()
    assert torch.equal(imp[0], torch.full((2, 49), 1.0 / 49))
    with pytest.raises(ValueError):
        load_teacher("swin_unknown_patch4_window7_224.ms_in1k", 224, device="cpu")


def test_presets_have_the_published_shapes():
    from basd_amd.models.cnn import CNN_PRESETS
    for name, depths, dims, heads in (("swin_tiny_patch4_window7_224", (2, 2, 6, 2), (96, 192, 384, 768), (3, 6, 12, 24)),
                                      ("swin_small_patch4_window7_224", (2, 2, 18, 2), (96, 192, 384, 768), (3, 6, 12, 24)),
                                      ("swin_base_patch4_window7_224", (2, 2, 18, 2), (128, 256, 512, 1024), (4, 8, 16, 32))):
        model = CNN_PRESETS[name]()
        assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == R.expected_state(depths, dims, heads)
        assert model.embed_dim == model.num_features == dims[-1]
        assert all(c == 32 * h for c, h in zip(dims, heads))
        blocks = [b for s in model.layers for b in s.blocks]
        assert [b.shift for b in model.layers[2].blocks] == [0, 3] * (depths[2] // 2) and len(blocks) == sum(depths)


def test_state_dict_keys_are_the_timm_names():
    """the names of timm >= 0.9, written out: no index / mask buffers, the patch merging at the START of stages 1..3"""
    from basd_amd.models.cnn import create_cnn
    patterns = [r"patch_embed\.proj\.(weight|bias)", r"patch_embed\.norm\.(weight|bias)", r"norm\.(weight|bias)",
                r"layers\.[123]\.downsample\.norm\.(weight|bias)", r"layers\.[123]\.downsample\.reduction\.weight",
                r"layers\.[0-3]\.blocks\.\d+\.norm[12]\.(weight|bias)",
                r"layers\.[0-3]\.blocks\.\d+\.attn\.(qkv|proj)\.(weight|bias)",
                r"layers\.[0-3]\.blocks\.\d+\.attn\.relative_position_bias_table",
                r"layers\.[0-3]\.blocks\.\d+\.mlp\.fc[12]\.(weight|bias)"]
    keys = list(create_cnn("swin_tiny_patch4_window7_224").state_dict())
    hits = {p: 0 for p in patterns}
    for k in keys:
        found = [p for p in patterns if re.fullmatch(p, k)]
        assert len(found) == 1, k
        hits[found[0]] += 1
    assert list(hits.values()) == [2, 2, 2, 6, 3, 48, 48, 12, 48] and len(keys) == 171


def test_old_layout_state_dict_loads_into_identical_parameters():
    """timm < 0.9: ``layers.{i}.downsample`` closes stage i, and the checkpoints carry ``attn_mask`` and
    ``relative_position_index`` buffers"""
    from basd_amd.models.swin import SwinTransformer
    torch.manual_seed(0)
    src = R.randomise_affine(SwinTransformer(**SMALL), seed=1)
    old = {}
    for k, v in src.state_dict().items():
        m = re.fullmatch(r"layers\.(\d)\.downsample\.(.*)", k)
        old[f"layers.{int(m.group(1)) - 1}.downsample.{m.group(2)}" if m else k] = v.clone()
    assert "layers.0.downsample.reduction.weight" in old and "layers.3.downsample.reduction.weight" not in old
    for i, depth in enumerate(SMALL["depths"]):
        for j in range(depth):
            old[f"layers.{i}.blocks.{j}.attn_mask"] = torch.zeros(4, 16, 16)
            old[f"layers.{i}.blocks.{j}.attn.relative_position_index"] = torch.zeros(16, 16, dtype=torch.long)
    torch.manual_seed(5)
    dst = SwinTransformer(**SMALL)
    n_keys = len(old)
    res = dst.load_state_dict(old, strict=True)
    assert not res.missing_keys and not res.unexpected_keys and len(old) == n_keys      # the caller's dict is untouched
    want = src.state_dict()
    got = dst.state_dict()
    assert list(got) == list(want) and all(torch.equal(got[k], want[k]) for k in want)
    dst2 = SwinTransformer(**SMALL)
    dst2.load_state_dict(src.state_dict(), strict=True)                                 # the current layout still loads
    assert all(torch.equal(a, b) for a, b in zip(dst2.state_dict().values(), want.values()))


def test_module_forward_equals_the_fp64_restatement():
    """fp32 CPU forward of the module (index gather, label mask) against the restatement (roll, reshape partition, slice
    mask) in fp64; every stage but the last has a shifted block.  The bound is 10x the restatement's own fp32 error on
    the same weights and images."""
    from basd_amd.models.swin import SwinTransformer
    torch.manual_seed(0)
    model = R.randomise_affine(SwinTransformer(**SMALL), seed=5).eval()
    x = torch.randn(2, 3, 128, 128)
    with torch.no_grad():
        got = model.forward_features(x)
    args = (model.state_dict(), x, SMALL["depths"], SMALL["heads"], SMALL["window_size"])
    want = R.forward_features(*args)
    own = R.forward_features(*args, dtype=torch.float32)
    assert got.shape == want.shape == (2, 4, 4, 256)
    err = float(R.rel_l2_per_sample(got, want).max())
    bound = 10.0 * float(R.rel_l2_per_sample(own, want).max())
    print(f"module fp32 vs fp64 {err:.3e}, restatement fp32 vs fp64 {bound / 10:.3e}")
    assert 0.0 < bound < 1e-4 and err <= bound, (err, bound)


@pytest.mark.parametrize("ws", [4, 5, 7, 8])
def test_relative_position_index_formula(ws):
    from basd_amd.models.swin import relative_position_index
    idx = relative_position_index(ws)
    assert idx.shape == (ws * ws, ws * ws)
    for y1, x1, y2, x2 in [(0, 0, 0, 0), (0, 0, ws - 1, ws - 1), (ws - 1, 0, 0, ws - 1), (2, 1, 0, 3), (ws - 1, ws - 2, 1, 0)]:
        assert int(idx[y1 * ws + x1, y2 * ws + x2]) == (y1 - y2 + ws - 1) * (2 * ws - 1) + (x1 - x2 + ws - 1)
    assert torch.equal(idx, R.bias_index(ws))


def _attention_only_block(dim, heads, ws, shift, seed):
    from basd_amd.models.swin import SwinBlock
    torch.manual_seed(seed)
    blk = SwinBlock(dim, heads, ws, shift).eval()
    with torch.no_grad():
        blk.attn.qkv.bias.normal_(std=0.2)
        blk.attn.qkv.weight.normal_(std=0.2)
    return blk


def test_unshifted_block_with_zero_table_is_per_window_sdpa():
    blk = _attention_only_block(64, 2, 7, 0, seed=3)
    with torch.no_grad():
        blk.attn.relative_position_bias_table.zero_()
        y = torch.randn(2, 14 * 21, 64)
        got = blk.attend(y, 14, 21)
        qkv = blk.attn.qkv(y).reshape(2, 2, 7, 3, 7, 3, 2, 32)            # [B, wy, iy, wx, ix, (q k v), head, d]
        q, k, v = qkv.permute(5, 0, 1, 3, 6, 2, 4, 7).reshape(3, 2, 6, 2, 49, 32)
        out = F.scaled_dot_product_attention(q, k, v)                      # [B, nW, head, N, d]
        out = out.reshape(2, 2, 3, 2, 7, 7, 32).permute(0, 1, 4, 2, 5, 3, 6).reshape(2, 14 * 21, 64)
        want = blk.attn.proj(out)
    assert float((got - want).abs().max()) < 1e-5


def test_shifted_block_gives_no_weight_across_mask_labels():
    """v = one-hot of the token's mask label (identity v and output projections), q and k from other channels: what a
    token receives in the label channels is the attention weight per label.  On a shifted 14 x 14 grid at window 7 no
    token receives more than 1e-30 from a label that is not its own, every token's own label carries weight 1, and the
    last window row / column really mixes labels inside a window."""
    ws, shift, n, c = 7, 3, 14, 32
    blk = _attention_only_block(c, 1, ws, shift, seed=4)
    lab = torch.roll(R.slice_labels(n, n, ws, shift).long(), shifts=(shift, shift), dims=(0, 1))   # label of token (y, x)
    with torch.no_grad():
        w = blk.attn.qkv.weight
        w[:2 * c, 16:] = 0.0                                              # q, k read the random channels only
        w[2 * c:] = torch.eye(c)
        blk.attn.qkv.bias[2 * c:] = 0.0
        blk.attn.proj.weight.copy_(torch.eye(c))
        blk.attn.proj.bias.zero_()
        blk.attn.relative_position_bias_table.normal_(std=0.5)
        y = torch.zeros(2, n * n, c)
        y[:, :, :16] = torch.randn(2, n * n, 16)
        y[:, :, 16:25] = F.one_hot(lab.reshape(-1), 9).float()
        got = blk.attend(y, n, n)[:, :, 16:25]                            # [B, tokens, label]: weight received per label
    own = F.one_hot(lab.reshape(-1), 9).bool()
    assert float(got[:, ~own].abs().max()) <= 1e-30
    assert float((got[:, own] - 1.0).abs().max()) < 1e-5
    assert len(set(lab[7 + 4:, 7 + 4:].reshape(-1).tolist())) == 1 and len(set(lab.reshape(-1).tolist())) == 9
    rolled_window = torch.roll(lab, shifts=(-shift, -shift), dims=(0, 1))[7:, 7:]
    assert len(set(rolled_window.reshape(-1).tolist())) == 4               # the last window holds four labels


def test_window_tokens_is_the_roll_and_partition():
    from basd_amd.models.swin import window_tokens
    for h, w, ws, shift in [(14, 14, 7, 3), (14, 21, 7, 3), (8, 8, 4, 2), (10, 15, 5, 2), (16, 8, 8, 4), (14, 14, 7, 0)]:
        ids = torch.arange(h * w).reshape(1, h, w, 1)
        want = R.partition(torch.roll(ids, shifts=(-shift, -shift), dims=(1, 2)), ws).squeeze(-1)
        token, label = window_tokens(h, w, ws, shift)
        assert torch.equal(token, want)
        if shift:
            assert torch.equal(label, R.partition(R.slice_labels(h, w, ws, shift).reshape(1, h, w, 1), ws).squeeze(-1).long())
        else:
            assert int(label.abs().max()) == 0


def _bf16_teacher(model):
    model = model.to(torch.bfloat16)
    for m in model.modules():
        if isinstance(m, torch.nn.LayerNorm):
            m.float()
    for p in model.parameters():
        p.requires_grad = False
    return model.eval()


@pytest.mark.parametrize("dims,heads", [((96, 192, 384, 768), (3, 6, 12, 24)), ((128, 256, 512, 1024), (4, 8, 16, 32))],
                         ids=["tiny-widths", "base-widths"])
def test_fused_forward_layout_and_padding_with_emulated_kernels(emulated_kernels, monkeypatch, dims, heads):
    """The fused forward (patch gather + GEMM images, qkv padded 288 -> 384, bias images, 96 channels in rows of 128,
    shift bookkeeping per block) through the emulated entries against the module's own plain bf16 forward: both are
    measured against the fp64 restatement on the same bf16 weights and the fused path's error may be at most twice the
    plain path's (two bf16 paths that round at different points; the rule of the device trunk test).  Every bias,
    LayerNorm parameter and bias table is random, so a dropped or mis-padded image gives an error of order 1.  The
    absolute bound is the bf16 rounding the path performs: unit roundoff 2^-9 at about 9 rounding points per block over
    8 blocks and 8 embed / merge / norm layers, summed in quadrature ~ 2^-9 * sqrt(80) = 1.8e-2, doubled for the growth
    through the MLPs.  Every pad column of every stage-0 tensor is exactly zero after every step."""
    from basd_amd.models.swin import SwinTransformer
    E = emulated_kernels
    depths = (2, 2, 2, 2)
    torch.manual_seed(1)
    model = _bf16_teacher(R.randomise_affine(SwinTransformer(depths, dims, heads, window_size=4), seed=11))
    assert model.fused_refusal() is None and model.prepare_fused()
    c0, ld0 = dims[0], model._fused["lds"][0]
    padded, shifts = [], []
    for name in ("gemm_bf16", "dwconv7_ln", "window_attention", "layernorm_fwd", "add_layernorm_fwd"):
        fn = getattr(E, name)

        def spy(*a, _fn=fn, _name=name, **k):
            out = _fn(*a, **k)
            if _name == "window_attention":
                shifts.append((a[0].shape[1], a[2], a[3]))
            for t in (out if isinstance(out, tuple) else (out,)):
                if ld0 != c0 and t.dim() >= 2 and t.shape[-1] == ld0:
                    padded.append((_name, t))
            return out
        monkeypatch.setattr(E, name, spy)
    x = torch.randn(2, 3, 128, 128).to(torch.bfloat16)
    with torch.no_grad():
        got = model.forward_features(x)
        plain = model._forward_plain(x)
    assert got.shape == plain.shape == (2, 4, 4, dims[-1]) and got.dtype == torch.bfloat16
    # (grid, window, shift) per block: a shifted second block in every stage but the last, whose grid is one window
    assert shifts == [(32, 4, 0), (32, 4, 2), (16, 4, 0), (16, 4, 2), (8, 4, 0), (8, 4, 2), (4, 4, 0), (4, 4, 0)]
    if c0 == 96:
        assert ld0 == 128 and model._fused["stages"][0]["blocks"][0]["qkv"][0].shape == (384, 128)
        assert {n for n, _ in padded} == {"gemm_bf16", "dwconv7_ln", "window_attention"} and len(padded) >= 12
    else:
        assert ld0 == c0 and not padded
    for _, t in padded:                  # the residual stream is updated in place: its final state is checked as well
        assert float(t.reshape(-1, ld0)[:, c0:].abs().max()) == 0.0
        assert float(t.reshape(-1, ld0)[:, :c0].abs().max()) > 0.0
    args = (model.state_dict(), x, depths, heads, 4)
    want = R.forward_features(*args)
    err = float(R.rel_l2_per_sample(got, want).max())
    err_plain = float(R.rel_l2_per_sample(plain, want).max())
    print(f"fused (emulated) vs fp64 {err:.3e}, plain bf16 vs fp64 {err_plain:.3e}")
    assert err <= 2.0 * err_plain, (err, err_plain)
    assert err <= 3.6e-2, err


def test_a_dropped_bias_image_is_seen(emulated_kernels):
    """the check above is not blind: zeroing one relative-position bias image, or one padded linear bias, of the prepared
    model moves the result by far more than the two bf16 paths differ"""
    from basd_amd.models.swin import SwinTransformer
    torch.manual_seed(1)
    model = _bf16_teacher(R.randomise_affine(SwinTransformer((2, 2, 2, 2), (96, 192, 384, 768), (3, 6, 12, 24), 4), seed=11))
    assert model.prepare_fused()
    x = torch.randn(2, 3, 128, 128).to(torch.bfloat16)
    with torch.no_grad():
        plain = model._forward_plain(x)
        good = float(R.rel_l2_per_sample(model.forward_features(x), plain).max())
        model._fused["stages"][1]["blocks"][0]["bias"].zero_()
        bad_table = float(R.rel_l2_per_sample(model.forward_features(x), plain).max())
        model.prepare_fused()
        model._fused["stages"][0]["blocks"][1]["qkv"][1].zero_()
        bad_bias = float(R.rel_l2_per_sample(model.forward_features(x), plain).max())
    assert good < 3.6e-2 < min(bad_table, bad_bias), (good, bad_table, bad_bias)


def test_unsupported_architecture_reports_instead_of_hiding(emulated_kernels):
    """head dim 64 is not what the window attention kernel takes: no weight images, and the forward on tensors the
    provider handles goes through library_fallback (strict mode names it); a .to() drops prepared images"""
    import basd_amd.losses._ops as O
    from basd_amd.models.swin import SwinTransformer
    model = _bf16_teacher(SwinTransformer((1, 1, 1, 1), (128, 256, 512, 1024), (2, 4, 8, 16), 4))
    assert "head dim" in model.fused_refusal() and not model.prepare_fused()
    O.FALLBACKS.clear()
    O.set_strict(True)
    try:
        with pytest.raises(O.StrictModeError), torch.no_grad():
            model.forward_features(torch.zeros(1, 3, 128, 128, dtype=torch.bfloat16))
    finally:
        O.set_strict(False)
        O.FALLBACKS.clear()
    ok = _bf16_teacher(SwinTransformer((1, 1, 1, 1), (128, 256, 512, 1024), (4, 8, 16, 32), 4))
    assert ok.prepare_fused() and ok._fused is not None
    ok.float()
    assert ok._fused is None
