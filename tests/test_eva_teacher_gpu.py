"""EVA-02 teachers on the device (GPU box only): basd_attention_fwd_rope_bf16 against fp64, its refusals, and the tiny
frozen bf16 teacher under strict mode, through the tap machinery and a graph capture.

The yardstick of every accuracy check is measured in the same test: the existing kernel (basd_attention_fwd_bf16) on a
qkv whose q and k were rotated in fp64 and rounded to bf16 once on the host, against the same fp64 reference (rotation
without rounding).  Both kernels round the same operands to bf16; the new one rotates in fp32 instead of fp64 in front
of that rounding, so it may reach at most 1.5 times that error (the margin tests/test_beit_teacher_gpu.py uses for the
same comparison).
"""
import ctypes
import functools
import math

import pytest
import torch

from tests._eva_ref import (BATCH, DEPTH, DIM, GRID, HEADS, IMG, eva_forward, fp64_params, rope_attention, rotated_bf16,
                            table_sin_cos, tiny_eva)
from tests._teacher_cases import bf16_frozen, images as _images

pytestmark = pytest.mark.gpu

HD = 64
SCALE = HD ** -0.5
B = 2
# (T, heads): T = 2; 7 with H = 2 and 3 (the head stride); 17 crosses a 16-key tile; 33 crosses a 32-key P V step; 257 is
# EVA's own length (17 tiles, odd); 272 the upper bound -- all three instantiations (T <= 64, <= 208, <= 272)
CASES = [(2, 2), (7, 2), (7, 3), (17, 2), (33, 2), (257, 3), (272, 2)]
# a grid with T - 1 patches
GRIDS = {2: (1, 1), 7: (2, 3), 17: (4, 4), 33: (4, 8), 257: (16, 16), 272: (1, 271)}
FACTOR = 1.5


def _table(kind, t):
    """"grid": the real table of a grid with T - 1 patches; "random": angles uniform in [0, 2 pi) in every row and pair,
    which catches pair and index mix-ups that smooth angles hide; "identity"; "uniform": one random row for all tokens"""
    from basd_amd._native import rope_table
    g = torch.Generator().manual_seed(17 * t + len(kind))
    if kind == "grid":
        return rope_table(*GRIDS[t], HD)
    if kind == "identity":
        return torch.tensor([1.0, 0.0]).expand(t, HD // 2, 2).contiguous()
    ang = 2.0 * math.pi * torch.rand(t if kind == "random" else 1, HD // 2, dtype=torch.float64, generator=g)
    return torch.stack([ang.cos(), ang.sin()], dim=-1).float().expand(t, -1, -1).contiguous()


@functools.lru_cache(maxsize=None)
def _case(t, heads, kind):
    """qkv (bf16, CPU), the table, the fp64 reference and the host-rotated qkv of the yardstick, computed once"""
    g = torch.Generator().manual_seed(1000 * t + heads)
    qkv = torch.randn(B, t, 3 * heads * HD, generator=g).to(torch.bfloat16)
    table = _table(kind, t)
    sin, cos = table_sin_cos(table)
    return {"qkv": qkv, "table": table, "want": rope_attention(qkv, sin, cos, heads, SCALE),
            "rotated": rotated_bf16(qkv, sin, cos, heads)}


def _errors(out, imp, want):
    """(relative L2 error of out, worst relative error of the importance) against an fp64 (out, importance) pair"""
    want_out, want_imp = want
    e_out = float((out.double().cpu() - want_out).norm() / want_out.norm())
    e_imp = float(((imp.double().cpu() - want_imp).abs() / want_imp).max()) if imp is not None else None
    return e_out, e_imp


def _yardstick(case, heads, want=None):
    """the existing kernel on the host-rotated qkv against the fp64 reference"""
    import basd_amd._native as native
    out, imp = native.attention_fwd(case["rotated"].cuda(), heads, HD, SCALE, want_importance=True)
    return _errors(out, imp, case["want"] if want is None else want)


def _run(case, heads, want_importance=True, table=None):
    import basd_amd._native as native
    table = case["table"] if table is None else table
    out, imp = native.attention_fwd_rope(case["qkv"].cuda(), table.cuda(), heads, HD, SCALE, want_importance)
    torch.cuda.synchronize()
    return out, imp


@pytest.mark.parametrize("kind", ["grid", "random"])
@pytest.mark.parametrize("t,heads", CASES)
def test_kernel_matches_fp64_like_the_existing_kernel_on_rotated_inputs(t, heads, kind):
    """Measured on an MI355X (new / existing kernel): DESIGN.md section 23."""
    case = _case(t, heads, kind)
    out, imp = _run(case, heads)
    assert out.shape == (B, t, heads * HD) and imp.shape == (B, t - 1) and imp.dtype == torch.float32
    new_out, new_imp = _errors(out, imp, case["want"])
    old_out, old_imp = _yardstick(case, heads)
    print(f"rope {kind} T={t} H={heads}: out rel-L2 new {new_out:.3e} / existing {old_out:.3e} = "
          f"{new_out / old_out:.3f}; importance worst rel new {new_imp:.3e} / existing {old_imp:.3e} = "
          f"{new_imp / old_imp:.3f}")
    assert new_out <= FACTOR * old_out, (new_out, old_out)
    assert new_imp <= FACTOR * old_imp, (new_imp, old_imp)
    # without the importance pointer: the same output, bit for bit
    out2, none = _run(case, heads, want_importance=False)
    assert none is None and torch.equal(out2.view(torch.int16), out.view(torch.int16))


@pytest.mark.parametrize("t,heads", [(7, 3), (17, 2), (257, 3)])
def test_identity_table_reproduces_the_existing_kernel_bit_for_bit(t, heads):
    import basd_amd._native as native
    case = _case(t, heads, "identity")
    out, imp = _run(case, heads)
    plain, _ = native.attention_fwd(case["qkv"].cuda(), heads, HD, SCALE)
    assert torch.equal(out.view(torch.int16), plain.view(torch.int16))
    assert float(((imp.double().cpu() - case["want"][1]).abs() / case["want"][1]).max()) < 1e-2


@pytest.mark.parametrize("t,heads", [(17, 2), (257, 3)])
def test_one_rotation_for_all_tokens_leaves_the_attention_alone(t, heads):
    """every row carries the same random angles: q . k is unchanged mathematically, so the reference is the existing
    kernel's (no rotation); the yardstick still rounds the rotated operands, as the kernel must"""
    case = _case(t, heads, "uniform")
    plain = rope_attention(case["qkv"], None, None, heads, SCALE)
    # the table is fp32: cos^2 + sin^2 = 1 to 1.2e-7, on logits of a few units -> the two references agree to 1e-6
    assert float((plain[0] - case["want"][0]).abs().max()) < 1e-6
    out, imp = _run(case, heads)
    new_out, new_imp = _errors(out, imp, plain)
    old_out, old_imp = _yardstick(case, heads, want=plain)
    print(f"rope uniform T={t} H={heads}: out {new_out:.3e} / {old_out:.3e}, importance {new_imp:.3e} / {old_imp:.3e}")
    assert new_out <= FACTOR * old_out and new_imp <= FACTOR * old_imp


@pytest.mark.parametrize("t,hd,table", [(17, 80, True), (1, 64, True), (273, 64, True), (17, 64, False)])
def test_refused_shapes_return_err_shape_and_write_nothing(t, hd, table):
    import basd_amd._native as native
    heads = 2
    qkv = torch.zeros(B, t, 3 * heads * hd, dtype=torch.bfloat16, device="cuda")
    rope = torch.zeros(t, hd // 2, 2, device="cuda")
    out = torch.full((B, t, heads * hd), 7.0, dtype=torch.bfloat16, device="cuda")
    imp = torch.full((B, heads, max(t - 1, 1)), 7.0, device="cuda")
    rc = native.lib().basd_attention_fwd_rope_bf16(
        ctypes.c_void_p(qkv.data_ptr()), ctypes.c_void_p(rope.data_ptr() if table else 0), B, t, heads, hd,
        ctypes.c_float(SCALE), ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(imp.data_ptr()),
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 1                                   # BASD_ERR_SHAPE
    msg = native.lib().basd_last_error().decode()
    assert "attention_fwd_rope" in msg and f"T={t}" in msg and f"hd={hd}" in msg and ("NULL" in msg) == (not table), msg
    assert bool((out == 7.0).all()) and bool((imp == 7.0).all())
    assert native.attention_fwd_rope_supported(t, hd) == (table is False)


# ---------------------------------------------------------------------------------------------------------------------
# the tiny frozen teacher

def _frozen(model):
    """what load_teacher does to an Eva: qkv bias materialised, bf16 with fp32 norms and table"""
    model.materialize_qkv_bias()
    return bf16_frozen(model.cuda())


def _teacher(model):
    from basd_amd.models.teacher import TeacherModel
    return TeacherModel(model=model, embed_dim=DIM, heads_per_layer=[HEADS] * DEPTH, depth=DEPTH, mlp_ratio=0.0,
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


@pytest.mark.parametrize("scale_mlp", [False, True])
def test_tiny_teacher_runs_strict_on_the_new_kernel_and_matches_fp64_like_the_library_path(monkeypatch, scale_mlp):
    """Measured on an MI355X (rel-L2 per layer, own path / library path): DESIGN.md section 23."""
    import basd_amd._native as native
    import basd_amd.losses._ops as O
    import basd_amd.models.eva as E
    from basd_amd.models.teacher import extract_intermediates
    calls = []
    real = native.attention_fwd_rope

    def spy(qkv, rope, heads, head_dim, scale, want_importance=False):
        calls.append((tuple(qkv.shape), tuple(rope.shape), rope.dtype, heads, want_importance))
        return real(qkv, rope, heads, head_dim, scale, want_importance)

    monkeypatch.setattr(native, "attention_fwd_rope", spy)
    model = _frozen(tiny_eva(scale_mlp))
    assert model.blocks[0].attn.rope.dtype == torch.float32 and model.blocks[0].attn.qkv.weight.dtype == torch.bfloat16
    x = _images(BATCH, IMG, seed=3).cuda()
    want_t, want_i = eva_forward(fp64_params(model.state_dict()), x.to(torch.bfloat16), heads=HEADS)
    toks, imps = _strict_intermediates(_teacher(model), x)
    t = GRID[0] * GRID[1] + 1
    assert calls == [((BATCH, t, 3 * DIM), (t, HD // 2, 2), torch.float32, HEADS, True)] * DEPTH, calls
    assert len(toks) == DEPTH and toks[0].shape == (BATCH, t - 1, DIM) and imps[DEPTH - 1].shape == (BATCH, t - 1)
    own = _rel_l2(toks, want_t)
    for j in range(DEPTH):              # bf16 activations in front of the softmax: the bound of the BEiT test
        assert torch.allclose(imps[j].double().cpu(), want_i[j], rtol=0.1, atol=1e-3), j
    # the library path of the same model: torch rotation + SDPA + separate tap, unfused MLP, torch token assembly
    monkeypatch.setattr(E, "_FUSED_EVA_DISPATCH", False)
    O.FALLBACKS.clear()
    try:
        lib_toks, lib_imps = extract_intermediates(_teacher(model), x)
        torch.cuda.synchronize()
        assert O.FALLBACKS["attention (rope)"] == DEPTH and O.FALLBACKS["SwiGLU MLP (EVA)"] == DEPTH, dict(O.FALLBACKS)
        O.set_strict(True)
        with pytest.raises(O.StrictModeError):
            extract_intermediates(_teacher(model), x)
    finally:
        O.set_strict(False)
        O.FALLBACKS.clear()
    assert len(calls) == DEPTH                       # the library path did not reach the kernel
    lib = _rel_l2(lib_toks, want_t)
    print(f"eva-teacher scale_mlp={scale_mlp}: rel-L2 vs fp64 per layer: own {[f'{v:.3e}' for v in own]}, "
          f"library {[f'{v:.3e}' for v in lib]}")
    for j in range(DEPTH):
        assert own[j] <= FACTOR * lib[j], (j, own, lib)
        assert torch.allclose(lib_imps[j].double().cpu(), want_i[j], rtol=0.1, atol=1e-3), j


def test_one_forward_under_graph_capture_replays_to_the_eager_result():
    model = _frozen(tiny_eva(True))
    x = _images(BATCH, IMG, seed=4).cuda().to(torch.bfloat16)
    with torch.no_grad():
        eager = model.forward_features(x).clone()   # also loads the code objects and packs the MLP operands
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            model.forward_features(x)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = model.forward_features(x)
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(captured.view(torch.int16), eager.view(torch.int16))
