"""basd_attention_fwd_long_rope_bf16 on the device (GPU box only): the rotary embedding inside the tiled attention
forward and its CLS tap against fp64, on every path of the kernel (one key, inside one key tile, exactly one tile, one
key past a tile, the first token count the dispatch sends here, DINOv3 at 384 px, the bound).

The yardstick of every accuracy check is measured in the same test: the existing tiled kernel
(basd_attention_fwd_long_bf16) on a qkv whose q and k were rotated in fp64 and rounded to bf16 once on the host, against
the same fp64 reference (rotation without rounding).  Both kernels round the same operands to bf16; the new one rotates
in fp32 instead of fp64 in front of that rounding, so it may reach at most 1.5 times that error on the output (relative
L2) and on the importance (worst relative): the project's factor for this comparison (tests/test_eva_teacher_gpu.py).
"""
import ctypes
import functools
import math

import pytest
import torch

from tests._eva_ref import rope_attention, rotated_bf16, table_sin_cos

pytestmark = pytest.mark.gpu

HD = 64
SCALE = HD ** -0.5
B = 2
# (T, heads): the minimum; inside one 64-key tile with an odd head stride; exactly one tile; one key past a tile; the
# first T the dispatch sends here; DINOv3 at 384 px (24 x 24 + 5); the bound
CASES = [(2, 2), (17, 3), (64, 2), (65, 2), (273, 3), (581, 2), (1024, 2)]
FACTOR = 1.5
KINDS = [(t, h, kind) for t, h in CASES for kind in ("dinov3", "eva", "random") if not (kind == "dinov3" and t < 6)]


def _grid(n):
    """the most square gh x gw = n"""
    gh = max(d for d in range(1, int(math.isqrt(n)) + 1) if n % d == 0)
    return gh, n // gh


def _table(kind, t):
    """"dinov3": the real DINOv3 table of a grid with T - 5 patches behind 5 prefix rows; "eva": EVA-02's of a grid with
    T - 1 patches; "random": angles uniform in [0, 2 pi) in every row and pair, which catches pair and index mix-ups that
    smooth angles hide; "identity"; "uniform": one random row for all tokens"""
    from basd_amd._native import dinov3_rope_table, rope_table
    g = torch.Generator().manual_seed(17 * t + len(kind))
    if kind == "dinov3":
        return dinov3_rope_table(*_grid(t - 5), HD, prefix_tokens=5)
    if kind == "eva":
        return rope_table(*_grid(t - 1), HD)
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
    assert tuple(table.shape) == (t, HD // 2, 2)
    sin, cos = table_sin_cos(table)
    return {"qkv": qkv, "table": table, "want": rope_attention(qkv, sin, cos, heads, SCALE),
            "rotated": rotated_bf16(qkv, sin, cos, heads)}


def _errors(out, imp, want):
    """(relative L2 error of out, worst relative error of the importance) against an fp64 (out, importance) pair"""
    want_out, want_imp = want
    e_out = float((out.double().cpu() - want_out).norm() / want_out.norm())
    e_imp = float(((imp.double().cpu() - want_imp).abs() / want_imp).max()) if imp is not None else None
    return e_out, e_imp


def _plain_long(qkv, heads, want_importance=True):
    """basd_attention_fwd_long_bf16 whatever T is (``attention_fwd`` would take the short kernel up to 272 tokens)"""
    import basd_amd._native as native
    qkv = qkv.cuda().contiguous()
    out = torch.empty(qkv.shape[0], qkv.shape[1], heads * HD, dtype=torch.bfloat16, device="cuda")
    out, imp = native._attention_fwd_long(qkv, out, heads, HD, SCALE, want_importance, False, False)
    torch.cuda.synchronize()
    return out, imp


def _run(case, heads, want_importance=True):
    import basd_amd._native as native
    out, imp = native.attention_fwd_long_rope(case["qkv"].cuda(), case["table"].cuda(), heads, HD, SCALE, want_importance)
    torch.cuda.synchronize()
    return out, imp


@pytest.mark.parametrize("t,heads,kind", KINDS)
def test_kernel_matches_fp64_like_the_existing_kernel_on_rotated_inputs(t, heads, kind):
    """Measured on an MI355X (new / existing kernel): DESIGN.md section 24."""
    case = _case(t, heads, kind)
    out, imp = _run(case, heads)
    assert out.shape == (B, t, heads * HD) and imp.shape == (B, t - 1) and imp.dtype == torch.float32
    new_out, new_imp = _errors(out, imp, case["want"])
    old_out, old_imp = _errors(*_plain_long(case["rotated"], heads), case["want"])
    print(f"long rope {kind} T={t} H={heads}: out rel-L2 new {new_out:.3e} / existing {old_out:.3e} = "
          f"{new_out / old_out:.3f}; importance worst rel new {new_imp:.3e} / existing {old_imp:.3e} = "
          f"{new_imp / old_imp:.3f}")
    assert new_out <= FACTOR * old_out, (new_out, old_out)
    assert new_imp <= FACTOR * old_imp, (new_imp, old_imp)
    # without the importance pointer: the same output, bit for bit
    out2, none = _run(case, heads, want_importance=False)
    assert none is None and torch.equal(out2.view(torch.int16), out.view(torch.int16))


@pytest.mark.parametrize("t,heads", CASES)
def test_identity_table_reproduces_the_existing_kernel_bit_for_bit(t, heads):
    case = _case(t, heads, "identity")
    out, imp = _run(case, heads)
    plain, plain_imp = _plain_long(case["qkv"], heads)
    assert torch.equal(out.view(torch.int16), plain.view(torch.int16))
    assert torch.equal(imp.view(torch.int32), plain_imp.view(torch.int32))


@pytest.mark.parametrize("t,heads", [(17, 3), (65, 2), (581, 2)])
def test_one_rotation_for_all_tokens_leaves_the_attention_alone(t, heads):
    """every row carries the same random angles: q . k is unchanged mathematically, so the reference is the unrotated
    attention; the yardstick still rounds the rotated operands, as the kernel must"""
    case = _case(t, heads, "uniform")
    plain = rope_attention(case["qkv"], None, None, heads, SCALE)
    # the table is fp32: cos^2 + sin^2 = 1 to 1.2e-7, on logits of a few units -> the two references agree to 1e-6
    assert float((plain[0] - case["want"][0]).abs().max()) < 1e-6
    out, imp = _run(case, heads)
    new_out, new_imp = _errors(out, imp, plain)
    old_out, old_imp = _errors(*_plain_long(case["rotated"], heads), plain)
    print(f"long rope uniform T={t} H={heads}: out {new_out:.3e} / {old_out:.3e}, importance {new_imp:.3e} / {old_imp:.3e}")
    assert new_out <= FACTOR * old_out and new_imp <= FACTOR * old_imp


def _call(qkv, rope_ptr, t, heads, hd, out_ptr, imp_ptr):
    import basd_amd._native as native
    rc = native.lib().basd_attention_fwd_long_rope_bf16(
        ctypes.c_void_p(qkv.data_ptr()), ctypes.c_void_p(rope_ptr), B, t, heads, hd, ctypes.c_float(SCALE),
        ctypes.c_void_p(out_ptr), ctypes.c_void_p(imp_ptr), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("t,heads", [(2, 2), (65, 2), (273, 3)])
def test_sentinels_around_both_outputs_survive(t, heads):
    guard = 1024
    case = _case(t, heads, "random")
    n_out, n_imp = B * t * heads * HD, B * heads * (t - 1)
    big_out = torch.full((guard + n_out + guard,), 7.0, dtype=torch.bfloat16, device="cuda")
    big_imp = torch.full((guard + n_imp + guard,), 7.0, device="cuda")
    rc = _call(case["qkv"].cuda(), case["table"].cuda().data_ptr(), t, heads, HD, big_out.data_ptr() + 2 * guard,
               big_imp.data_ptr() + 4 * guard)
    assert rc == 0
    for big, n in ((big_out, n_out), (big_imp, n_imp)):
        assert bool((big[:guard] == 7.0).all()) and bool((big[guard + n:] == 7.0).all())
    out, imp = _run(case, heads)
    assert torch.equal(big_out[guard:guard + n_out].view(torch.int16), out.reshape(-1).view(torch.int16))
    assert torch.equal(big_imp[guard:guard + n_imp].view(B, heads, t - 1).sum(dim=1), imp)


@pytest.mark.parametrize("t,hd,table", [(300, 80, True), (1, 64, True), (1025, 64, True), (300, 64, False)])
def test_refused_shapes_return_err_shape_and_write_nothing(t, hd, table):
    import basd_amd._native as native
    heads = 2
    qkv = torch.zeros(B, t, 3 * heads * hd, dtype=torch.bfloat16, device="cuda")
    rope = torch.zeros(t, hd // 2, 2, device="cuda")
    out = torch.full((B, t, heads * hd), 7.0, dtype=torch.bfloat16, device="cuda")
    imp = torch.full((B, heads, max(t - 1, 1)), 7.0, device="cuda")
    rc = _call(qkv, rope.data_ptr() if table else 0, t, heads, hd, out.data_ptr(), imp.data_ptr())
    assert rc == 1                                   # BASD_ERR_SHAPE
    msg = native.lib().basd_last_error().decode()
    assert "attention_fwd_long_rope" in msg and f"T={t}" in msg and f"hd={hd}" in msg and ("NULL" in msg) == (not table), msg
    assert bool((out == 7.0).all()) and bool((imp == 7.0).all())
    assert native.attention_fwd_long_rope_supported(t, hd) == (table is False)
