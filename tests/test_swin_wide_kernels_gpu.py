"""basd_window_attention_fwd_wide_bf16 (csrc/swin_wide.hip, windows 9 .. 16) against fp64 on the same bf16 inputs.

As tests/test_swin_kernels_gpu.py: the reference is tests/_swin_ref.py (explicit roll, reshape partition, mask tensor,
dense softmax, the bias expanded entry by entry from the table) in fp64 on the CPU.  The yardstick is the same arithmetic
in torch fp32 on the device, rounded to bf16 at the kernel's rounding points (the probabilities before the second
product, and the output): the kernel and the yardstick may differ in fp32 summation order and in the exp implementation
and in nothing else, so the kernel's error against fp64 (rel-L2 and max-abs) may be at most twice the yardstick's (the
rule of DESIGN section 8).  The inputs are those of that file (outlier channels, 7.0 behind 3 C)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests import _swin_ref as R
from tests.test_swin_kernels_gpu import _errors, _qkv

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nat():
    import basd_amd._native as native
    native.lib()
    return native


WIDE_CASES = [  # B, H, W, ws, shift, heads, ld_qkv, ld_out, logit gain
    (2, 24, 24, 12, 6, 3, 288, 96, 1.0),       # all four window kinds of the mask; nine tiles
    (2, 24, 24, 12, 0, 3, 288, 96, 1.0),       # shift 0
    (1, 12, 12, 12, 0, 24, 2304, 768, 1.0),    # one window, many heads
    (2, 24, 36, 12, 6, 6, 576, 192, 30.0),     # non-square grid: the wrap differs per axis; logits of order +-30
    (2, 18, 27, 9, 4, 2, 192, 64, 1.0),        # 81 slots, 15 dead in the last tile
    (1, 20, 30, 10, 5, 4, 384, 128, 1.0),      # 100 slots, seven tiles: the half-empty 32-key step
    (1, 32, 16, 16, 8, 2, 192, 64, 1.0),       # all 256 slots
    (1, 48, 48, 12, 6, 3, 384, 128, 1.0),      # padded rows: input pad 7.0 never read, output pad exactly zero
]


@pytest.mark.parametrize("B,H,W,ws,shift,heads,ld_qkv,ld_out,gain", WIDE_CASES)
def test_wide_window_attention_against_fp64(nat, B, H, W, ws, shift, heads, ld_qkv, ld_out, gain):
    c, scale = 32 * heads, 32 ** -0.5
    g = torch.Generator().manual_seed(H * W + heads)
    qkv = _qkv(B, H, W, heads, ld_qkv, gain, seed=H + W + ws)
    table = 0.5 * torch.randn((2 * ws - 1) ** 2, heads, generator=g)
    bias = R.expand_bias(table, ws)                                       # [heads, N, N] fp32: the reference's only
    got = nat.window_attention_wide(qkv.cuda(), table.cuda(), ws, shift, heads, scale, ld_out=ld_out)
    torch.cuda.synchronize()
    assert got.shape == (B, H, W, ld_out) and got.dtype == torch.bfloat16
    assert bool(torch.isfinite(got.float()).all())
    if ld_out > c:
        assert float(got[..., c:].float().abs().max()) == 0.0
    want = R.window_attention(qkv[..., :3 * c].double(), bias.double(), ws, shift, heads, scale)
    yard = R.window_attention(qkv[..., :3 * c].cuda().float(), bias.cuda(), ws, shift, heads, scale,
                              round_p=True).to(torch.bfloat16)
    logits = float((scale * (qkv[..., :c].float().reshape(-1, heads, 32) * qkv[..., c:2 * c].float().reshape(-1, heads, 32)).sum(-1)).std())
    r_k, r_y, m_k, m_y = _errors(got[..., :c], yard, want)
    print(f"wide window attention {B}x{H}x{W} ws {ws} shift {shift} heads {heads} (logit std {logits:.1f}): rel-L2 kernel "
          f"{r_k:.3e} yardstick {r_y:.3e} ratio {r_k / r_y:.3f}; max-abs kernel {m_k:.3e} yardstick {m_y:.3e} "
          f"ratio {m_k / m_y:.3f}")
    assert gain / 1.5 < logits < gain * 1.5
    assert r_k <= 2.0 * r_y and m_k <= 2.0 * m_y
    again = nat.window_attention_wide(qkv.cuda(), table.cuda(), ws, shift, heads, scale, ld_out=ld_out)
    assert torch.equal(again, got)                                        # no atomics, no schedule dependence


def test_shifted_wide_windows_do_not_leak_across_mask_labels(nat):
    """v = one-hot of the token's mask label at window 12, shift 6 on a 24 x 24 grid: no token receives weight from
    another label"""
    ws, shift, n, heads = 12, 6, 24, 1
    lab = torch.roll(R.slice_labels(n, n, ws, shift).long(), shifts=(shift, shift), dims=(0, 1))
    assert len(set(lab.reshape(-1).tolist())) == 9
    qkv = torch.zeros(2, n, n, 96)
    qkv[..., :64] = torch.randn(2, n, n, 64, generator=torch.Generator().manual_seed(0))
    qkv[..., 64:73] = F.one_hot(lab, 9).float()
    table = torch.zeros((2 * ws - 1) ** 2, heads, device="cuda")
    got = nat.window_attention_wide(qkv.to(torch.bfloat16).cuda(), table, ws, shift, heads, 32 ** -0.5).float().cpu()[..., :9]
    own = F.one_hot(lab, 9).bool().expand(2, n, n, 9)
    assert float(got[~own].abs().max()) <= 1e-30                          # exp(-100 + a logit difference of order 10)
    assert float((got[own] - 1.0).abs().max()) <= 2 ** -7                 # the bf16 probabilities of a row sum to 1


def test_wide_window_attention_refuses_what_it_does_not_tile(nat):
    """window 8 (the 64-slot entry's) and 17, head dim 64 (C != 32 heads), a grid that is no multiple of the window, a
    shift outside the window, bad strides, a misaligned pointer, out aliasing qkv: an error status that names the entry
    and no launch; the Python gate agrees with every shape refusal"""
    x = torch.zeros(1, 24, 24, 768, dtype=torch.bfloat16, device="cuda")
    out = torch.full((1, 24, 24, 256), 3.0, dtype=torch.bfloat16, device="cuda")
    table = torch.zeros(33 * 33, 8, device="cuda")
    call = nat.lib().basd_window_attention_fwd_wide_bf16
    good = dict(B=1, H=24, W=24, heads=4, C=128, ws=12, shift=6, ld_qkv=768, ld_out=256)
    assert nat.window_attention_wide_supported(*(good[k] for k in ("H", "W", "ws", "shift", "heads", "C", "ld_qkv", "ld_out")))
    bad = [dict(ws=8), dict(ws=17), dict(C=256), dict(H=20), dict(W=22), dict(shift=12), dict(shift=-1), dict(ld_qkv=380),
           dict(ld_qkv=376), dict(ld_out=120), dict(ld_out=252), dict(qkv_offset=2), dict(alias=True)]
    for change in bad:
        a = dict(good, qkv_offset=0, alias=False)
        a.update(change)
        qkv_ptr = ctypes.c_void_p(x.data_ptr() + a["qkv_offset"])
        out_ptr = qkv_ptr if a["alias"] else nat._ptr(out)
        rc = call(qkv_ptr, nat._ptr(table), a["B"], a["H"], a["W"], a["heads"], a["C"], a["ws"], a["shift"], a["ld_qkv"],
                  a["ld_out"], 0.17, out_ptr, nat._stream())
        assert rc != 0, change
        assert b"window_attention_fwd_wide" in nat.lib().basd_last_error(), change
        if "qkv_offset" not in change and "alias" not in change:
            assert not nat.window_attention_wide_supported(a["H"], a["W"], a["ws"], a["shift"], a["heads"], a["C"],
                                                           a["ld_qkv"], a["ld_out"]), change
    torch.cuda.synchronize()
    assert float((out.float() - 3.0).abs().max()) == 0.0 and float(x.float().abs().max()) == 0.0     # nothing ran
    with pytest.raises(nat.BasdNativeError):
        nat.window_attention_wide(x, table[:529, :4].contiguous(), 8, 4, 4, 0.17)
    with pytest.raises(nat.BasdNativeError):                              # an expanded image is not a table
        nat.window_attention_wide(x, torch.zeros(4, 144, 144, device="cuda"), 12, 6, 4, 0.17)
    assert not nat.window_attention_supported(24, 24, 12, 6, 4, 128, 384, 128)      # the 64-slot entry is unchanged
