"""basd_attention_fwd_long_relbias_bf16 on the device (GPU box only): BEiT's relative-position bias inside the tiled
attention forward and its CLS tap against fp64, on every path of the kernel (the minimum, inside one key tile, exactly
one tile, one key and one query past a tile, the first token count the dispatch sends here, BEiT at 384 px, a one-row
grid at the bound, the largest table).

The yardstick is ``tests/_beit_long_cases.py::emulated_attention``: the kernel's rounding points restated in fp64,
against the same exact fp64 reference (``tests/_beit_ref.py::biased_attention``).  The kernel has the same rounding
points and another order of fp32 operations (online softmax, the bias added as table / scale to the raw dot), so it may
reach at most 1.5 times the emulation's error on the output (relative L2) and on the importance (worst relative): the
project's factor for this comparison (tests/test_attention_long_rope_gpu.py).

The emulation's own errors, computed on the CPU (out rel-L2, importance worst rel), with ``seeded_table``'s N(0, 1.5^2)
patch rows -- all below the 1e-2 the amplitude was to keep, so the amplitude is ``seeded_table``'s:
    1x1, H 2 (T 2): 1.306e-03, 2.914e-03        16x17, H 3 (T 273):   1.921e-03, 1.050e-02
    3x5, H 3 (T 16): 1.775e-03, 4.905e-03       24x24, H 2 (T 577):   1.989e-03, 1.108e-02
    7x9, H 2 (T 64): 1.875e-03, 6.171e-03       1x1023, H 2 (T 1024): 2.010e-03, 8.762e-03
    8x8, H 2 (T 65): 1.906e-03, 7.872e-03       31x33, H 2 (T 1024):  2.028e-03, 8.388e-03
"""
import ctypes
import functools

import pytest
import torch

from tests._beit_long_cases import emulated_attention
from tests._beit_ref import biased_attention, seeded_table, table_rows

pytestmark = pytest.mark.gpu

HD = 64
SCALE = HD ** -0.5
B = 2
# (gh, gw, heads): T = 2, 16, 64, 65, 273, 577, 1024, 1024
CASES = [(1, 1, 2), (3, 5, 3), (7, 9, 2), (8, 8, 2), (16, 17, 3), (24, 24, 2), (1, 1023, 2), (31, 33, 2)]
SHORT = [c for c in CASES if c[0] * c[1] + 1 <= 272]
FACTOR = 1.5
ERR_SHAPE = 1


def _errors(out, imp, want):
    """(relative L2 error of out, worst relative error of the importance) against an fp64 (out, importance) pair"""
    want_out, want_imp = want
    e_out = float((out.double().cpu() - want_out).norm() / want_out.norm())
    e_imp = float(((imp.double().cpu() - want_imp).abs() / want_imp).max()) if imp is not None else None
    return e_out, e_imp


@functools.lru_cache(maxsize=None)
def _case(gh, gw, heads):
    """qkv (bf16, CPU), the seeded table, the fp64 reference and the emulation's errors against it, computed once"""
    t = gh * gw + 1
    g = torch.Generator().manual_seed(1000 * gh + 10 * gw + heads)
    qkv = torch.randn(B, t, 3 * heads * HD, generator=g).to(torch.bfloat16)
    table = seeded_table(gh, gw, heads, seed=gh + 31 * gw)
    want = biased_attention(qkv, table, gh, gw, heads, SCALE)
    return {"qkv": qkv, "table": table, "want": want,
            "emulation": _errors(*emulated_attention(qkv, table, gh, gw, heads, SCALE), want)}


def _run(case, table, gh, gw, heads, want_importance=True):
    import basd_amd._native as native
    out, imp = native.attention_fwd_long_relbias(case["qkv"].cuda(), table.cuda(), gh, gw, heads, HD, SCALE,
                                                 want_importance)
    torch.cuda.synchronize()
    return out, imp


@functools.lru_cache(maxsize=None)
def _zero_run(gh, gw, heads):
    """the new entry with an all-zero table, shared by the tests that compare against it"""
    case = _case(gh, gw, heads)
    return _run(case, torch.zeros_like(case["table"]), gh, gw, heads)


def _plain_long(qkv, heads):
    """basd_attention_fwd_long_bf16 whatever T is (``attention_fwd`` would take the short kernel up to 272 tokens)"""
    import basd_amd._native as native
    qkv = qkv.cuda().contiguous()
    out = torch.empty(qkv.shape[0], qkv.shape[1], heads * HD, dtype=torch.bfloat16, device="cuda")
    out, imp = native._attention_fwd_long(qkv, out, heads, HD, SCALE, True, False, False)
    torch.cuda.synchronize()
    return out, imp


def _same_bits(a, b):
    view = torch.int16 if a.dtype == torch.bfloat16 else torch.int32
    return a.shape == b.shape and torch.equal(a.contiguous().view(view), b.contiguous().view(view))


@pytest.mark.parametrize("gh,gw,heads", CASES)
def test_kernel_matches_fp64_like_the_emulation_of_its_rounding_points(gh, gw, heads):
    """Measured on an MI355X (kernel / emulation): DESIGN.md section 25.  The output rows of the three heads of the
    H = 3 cases read three different columns of the table (``seeded_table`` shifts the CLS rows by 0.25 h and draws
    the patch rows per head): a wrong head stride fails here."""
    case = _case(gh, gw, heads)
    t = gh * gw + 1
    out, imp = _run(case, case["table"], gh, gw, heads)
    assert out.shape == (B, t, heads * HD) and out.dtype == torch.bfloat16
    assert imp.shape == (B, t - 1) and imp.dtype == torch.float32
    new_out, new_imp = _errors(out, imp, case["want"])
    emu_out, emu_imp = case["emulation"]
    print(f"long relbias {gh}x{gw} H={heads} T={t}: out rel-L2 kernel {new_out:.3e} / emulation {emu_out:.3e} = "
          f"{new_out / emu_out:.3f}; importance worst rel kernel {new_imp:.3e} / emulation {emu_imp:.3e} = "
          f"{new_imp / emu_imp:.3f}")
    assert emu_out < 1e-2, emu_out                   # the table's amplitude leaves the yardstick meaningful
    assert new_out <= FACTOR * emu_out, (new_out, emu_out)
    assert new_imp <= FACTOR * emu_imp, (new_imp, emu_imp)
    # null cls_importance: the same output, bit for bit
    out2, none = _run(case, case["table"], gh, gw, heads, want_importance=False)
    assert none is None and _same_bits(out2, out)


@pytest.mark.parametrize("gh,gw,heads", SHORT)
def test_agrees_with_the_short_kernel_where_both_apply(gh, gw, heads):
    """output: the errors against fp64 side by side; taps: the short kernel taps fp32 logits, the long one bf16-rounded
    ones, both within bf16 rounding of the exact row -- the bound of the existing BEiT tests between them"""
    import basd_amd._native as native
    case = _case(gh, gw, heads)
    out, imp = _run(case, case["table"], gh, gw, heads)
    s_out, s_imp = native.attention_fwd_relbias(case["qkv"].cuda(), case["table"].cuda(), gh, gw, heads, HD, SCALE, True)
    torch.cuda.synchronize()
    new_out, _ = _errors(out, imp, case["want"])
    old_out, _ = _errors(s_out, s_imp, case["want"])
    print(f"long / short relbias {gh}x{gw} H={heads}: out rel-L2 {new_out:.3e} / {old_out:.3e} = {new_out / old_out:.3f}")
    assert new_out <= FACTOR * old_out, (new_out, old_out)
    assert torch.allclose(imp, s_imp, rtol=0.1, atol=1e-3)


@pytest.mark.parametrize("gh,gw,heads", CASES)
def test_zero_table_reproduces_the_plain_tiled_kernel_bit_for_bit(gh, gw, heads):
    out, imp = _zero_run(gh, gw, heads)
    plain, plain_imp = _plain_long(_case(gh, gw, heads)["qkv"], heads)
    assert _same_bits(out, plain)
    assert _same_bits(imp, plain_imp)


@pytest.mark.parametrize("gh,gw,heads", CASES)
def test_patch_rows_alone_leave_the_cls_query_and_the_tap_alone(gh, gw, heads):
    case = _case(gh, gw, heads)
    base_out, base_imp = _zero_run(gh, gw, heads)
    patches = case["table"].clone()
    patches[table_rows(gh, gw) - 3:] = 0.0
    out, imp = _run(case, patches, gh, gw, heads)
    assert _same_bits(out[:, 0], base_out[:, 0]) and _same_bits(imp, base_imp)
    if gh * gw > 1:            # one patch: its only patch key is itself, one logit against the unbiased CLS key
        assert bool((out[:, 1:] != base_out[:, 1:]).any(dim=-1).all())
    else:
        assert not torch.equal(out[:, 1:], base_out[:, 1:])


@pytest.mark.parametrize("gh,gw,heads", CASES)
def test_cls_rows_alone_move_every_query_and_the_tap(gh, gw, heads):
    """rows R - 3 (CLS query, patch key), R - 2 (patch query, CLS key) and R - 1 (CLS, CLS): dropping any of the three
    special cases leaves part of this unchanged"""
    case = _case(gh, gw, heads)
    rows = table_rows(gh, gw)
    base_out, base_imp = _zero_run(gh, gw, heads)
    cls_only = torch.zeros_like(case["table"])
    cls_only[rows - 3:] = case["table"][rows - 3:]
    out, imp = _run(case, cls_only, gh, gw, heads)
    assert bool((out != base_out).any(dim=-1).all())
    assert bool((imp != base_imp).all())
    want = biased_attention(case["qkv"], cls_only, gh, gw, heads, SCALE)
    e_out, e_imp = _errors(out, imp, want)
    emu_out, emu_imp = _errors(*emulated_attention(case["qkv"], cls_only, gh, gw, heads, SCALE), want)
    assert e_out <= FACTOR * emu_out and e_imp <= FACTOR * emu_imp, (e_out, emu_out, e_imp, emu_imp)


@pytest.mark.parametrize("gh,gw,heads", [(3, 5, 3), (16, 17, 3)])
def test_every_head_reads_its_own_column_of_the_table(gh, gw, heads):
    """a head's output depends on nothing but its own q, k, v and its own column: the H = 3 run equals, bit for bit, the
    three H = 1 runs on the head's slice of qkv and column of the table; the H = 3 tap is their mean"""
    case = _case(gh, gw, heads)
    t = gh * gw + 1
    out, imp = _run(case, case["table"], gh, gw, heads)
    qkv = case["qkv"].reshape(B, t, 3, heads, HD)
    taps = []
    for h in range(heads):
        one = {"qkv": qkv[:, :, :, h].reshape(B, t, 3 * HD).contiguous()}
        o, i = _run(one, case["table"][:, h:h + 1].contiguous(), gh, gw, 1)
        assert _same_bits(out[:, :, h * HD:(h + 1) * HD], o), h
        taps.append(i)
    torch.testing.assert_close(imp, torch.stack(taps).sum(dim=0) / heads, rtol=1e-5, atol=1e-8)


def _call(qkv, table_ptr, gh, gw, heads, hd, scale, out_ptr, imp_ptr):
    import basd_amd._native as native
    rc = native.lib().basd_attention_fwd_long_relbias_bf16(
        ctypes.c_void_p(qkv.data_ptr()), ctypes.c_void_p(table_ptr), B, gh, gw, heads, hd, ctypes.c_float(scale),
        ctypes.c_void_p(out_ptr), ctypes.c_void_p(imp_ptr), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("gh,gw,heads", [(1, 1, 2), (8, 8, 2), (16, 17, 3)])
def test_sentinels_around_both_outputs_survive(gh, gw, heads):
    guard = 1024
    case = _case(gh, gw, heads)
    t = gh * gw + 1
    n_out, n_imp = B * t * heads * HD, B * heads * (t - 1)
    big_out = torch.full((guard + n_out + guard,), 7.0, dtype=torch.bfloat16, device="cuda")
    big_imp = torch.full((guard + n_imp + guard,), 7.0, device="cuda")
    rc = _call(case["qkv"].cuda(), case["table"].cuda().data_ptr(), gh, gw, heads, HD, SCALE,
               big_out.data_ptr() + 2 * guard, big_imp.data_ptr() + 4 * guard)
    assert rc == 0
    for big, n in ((big_out, n_out), (big_imp, n_imp)):
        assert bool((big[:guard] == 7.0).all()) and bool((big[guard + n:] == 7.0).all())
    out, imp = _run(case, case["table"], gh, gw, heads)
    assert _same_bits(big_out[guard:guard + n_out], out.reshape(-1))
    assert torch.equal(big_imp[guard:guard + n_imp].view(B, heads, t - 1).sum(dim=1), imp)


@pytest.mark.parametrize("gh,gw,hd,table,scale", [(32, 32, 64, True, SCALE), (14, 14, 80, True, SCALE),
                                                  (0, 5, 64, True, SCALE), (14, 14, 64, False, SCALE),
                                                  (14, 14, 64, True, 0.0)])
def test_refused_shapes_return_err_shape_and_write_nothing(gh, gw, hd, table, scale):
    import basd_amd._native as native
    heads, t = 2, max(gh * gw + 1, 2)
    qkv = torch.zeros(B, t, 3 * heads * hd, dtype=torch.bfloat16, device="cuda")
    tab = torch.zeros(max(table_rows(gh, gw), 4), heads, device="cuda")
    out = torch.full((B, t, heads * hd), 7.0, dtype=torch.bfloat16, device="cuda")
    imp = torch.full((B, heads, t - 1), 7.0, device="cuda")
    rc = _call(qkv, tab.data_ptr() if table else 0, gh, gw, heads, hd, scale, out.data_ptr(), imp.data_ptr())
    assert rc == ERR_SHAPE
    assert "attention_fwd_long_relbias" in native.lib().basd_last_error().decode()
    assert bool((out == 7.0).all()) and bool((imp == 7.0).all())
    # the predicates speak about the shape: they agree with the entry wherever the shape is what it refuses
    shape_ok = table and scale > 0
    assert native.attention_fwd_long_relbias_supported(gh, gw, hd) == (not shape_ok)
    if not shape_ok:
        assert native.attention_fwd_relbias_supported(gh, gw, hd)         # 14 x 14, hd 64: both entries' range
    else:
        assert not native.attention_fwd_relbias_supported(gh, gw, hd)
    assert native.attention_fwd_long_relbias_supported(31, 33, 64) and native.attention_fwd_long_relbias_supported(1, 1, 64)
    assert native.attention_fwd_long_relbias_supported(16, 17, 64) and not native.attention_fwd_relbias_supported(16, 17, 64)
