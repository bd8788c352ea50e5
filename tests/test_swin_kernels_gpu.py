"""The two entries of csrc/swin.hip against fp64 on the same bf16 inputs.

The reference is tests/_swin_ref.py (explicit roll, reshape partition, mask tensor, dense softmax) in fp64 on the CPU.  The
yardstick is the same arithmetic in torch fp32 on the device, rounded to bf16 at the kernel's rounding points (window
attention: the probabilities before the second product, and the output; patch merge: the output): the kernel and the
yardstick may differ in fp32 summation order and in the exp / rsqrt implementation and in nothing else, so the kernel's
error against fp64 (rel-L2 and max-abs) may be at most twice the yardstick's (the rule of DESIGN section 8)."""
import pytest
import torch
import torch.nn.functional as F

from tests import _swin_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nat():
    import basd_amd._native as native
    native.lib()
    return native


def _features(shape, seed, outliers=True):
    """feature statistics of a trained network: unit-scale channels plus a few whose magnitude is 50 - 100 times larger"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    c = shape[-1]
    if outliers and c >= 8:
        idx = torch.randperm(c, generator=g)[:max(2, c // 48)]
        x[..., idx] *= 50.0 + 50.0 * torch.rand(len(idx), generator=g)
    return x.to(torch.bfloat16)


def _errors(got, yard, want):
    got, yard, want = got.double().cpu(), yard.double().cpu(), want.double()
    scale = float(want.norm())
    return (float((got - want).norm()) / scale, float((yard - want).norm()) / scale,
            float((got - want).abs().max()), float((yard - want).abs().max()))


WA_CASES = [  # B, H, W, ws, shift, heads, ld_qkv, ld_out, logit gain
    (2, 14, 14, 7, 3, 3, 288, 96, 1.0),        # all four window kinds of the mask
    (2, 14, 14, 7, 0, 3, 288, 96, 1.0),        # shift 0
    (1, 7, 7, 7, 0, 24, 2304, 768, 1.0),       # one window, many heads
    (2, 14, 21, 7, 3, 6, 576, 192, 30.0),      # non-square grid: the wrap differs per axis; logits of order +-30
    (2, 8, 8, 4, 2, 4, 384, 128, 1.0),         # 16 of 64 slots live
    (2, 10, 15, 5, 2, 2, 192, 64, 1.0),        # odd token count 25
    (3, 16, 8, 8, 4, 2, 192, 64, 1.0),         # full 64-slot tile
    (2, 56, 56, 7, 3, 3, 384, 128, 1.0),       # padded rows: input pad 7.0 never read, output pad exactly zero
]


def _qkv(B, H, W, heads, ld_qkv, gain, seed):
    """q and k at trained-network scale: unit channels plus outlier channels in q and k (the same channels of every
    head pair up in q . k), scaled so that scale * q . k has standard deviation ``gain``; v with outliers; the columns
    behind 3 C hold 7.0"""
    c = 32 * heads
    x = torch.full((B, H, W, ld_qkv), 7.0)
    q, k, v = (_features((B, H, W, c), seed + i).float() for i in range(3))
    std = float((32 ** -0.5 * (q.reshape(-1, heads, 32) * k.reshape(-1, heads, 32)).sum(-1)).std())
    amp = (gain / std) ** 0.5
    x[..., :c], x[..., c:2 * c], x[..., 2 * c:3 * c] = q * amp, k * amp, v
    return x.to(torch.bfloat16)


@pytest.mark.parametrize("B,H,W,ws,shift,heads,ld_qkv,ld_out,gain", WA_CASES)
def test_window_attention_against_fp64(nat, B, H, W, ws, shift, heads, ld_qkv, ld_out, gain):
    c, n, scale = 32 * heads, ws * ws, 32 ** -0.5
    g = torch.Generator().manual_seed(H * W + heads)
    qkv = _qkv(B, H, W, heads, ld_qkv, gain, seed=H + W + ws)
    table = 0.5 * torch.randn((2 * ws - 1) ** 2, heads, generator=g)
    bias = R.expand_bias(table, ws)                                       # [heads, N, N] fp32
    img = nat.window_bias_image(bias.cuda())
    assert img.shape == (heads, 64, 64) and torch.equal(img[:, :n, :n].cpu(), bias)
    got = nat.window_attention(qkv.cuda(), img, ws, shift, heads, scale, ld_out=ld_out)
    torch.cuda.synchronize()
    assert got.shape == (B, H, W, ld_out) and got.dtype == torch.bfloat16
    if ld_out > c:
        assert float(got[..., c:].float().abs().max()) == 0.0
    want = R.window_attention(qkv[..., :3 * c].double(), bias.double(), ws, shift, heads, scale)
    yard = R.window_attention(qkv[..., :3 * c].cuda().float(), bias.cuda(), ws, shift, heads, scale,
                              round_p=True).to(torch.bfloat16)
    logits = float((scale * (qkv[..., :c].float().reshape(-1, heads, 32) * qkv[..., c:2 * c].float().reshape(-1, heads, 32)).sum(-1)).std())
    r_k, r_y, m_k, m_y = _errors(got[..., :c], yard, want)
    print(f"window attention {B}x{H}x{W} ws {ws} shift {shift} heads {heads} (logit std {logits:.1f}): rel-L2 kernel "
          f"{r_k:.3e} yardstick {r_y:.3e} ratio {r_k / r_y:.3f}; max-abs kernel {m_k:.3e} yardstick {m_y:.3e} "
          f"ratio {m_k / m_y:.3f}")
    assert gain / 1.5 < logits < gain * 1.5
    assert r_k <= 2.0 * r_y and m_k <= 2.0 * m_y
    again = nat.window_attention(qkv.cuda(), img, ws, shift, heads, scale, ld_out=ld_out)
    assert torch.equal(again, got)                                        # no atomics, no schedule dependence


def test_shifted_windows_do_not_leak_across_mask_labels(nat):
    """v = one-hot of the token's mask label: on the device too, no token receives weight from another label"""
    ws, shift, n, heads = 7, 3, 14, 1
    lab = torch.roll(R.slice_labels(n, n, ws, shift).long(), shifts=(shift, shift), dims=(0, 1))
    qkv = torch.zeros(2, n, n, 96)
    qkv[..., :64] = torch.randn(2, n, n, 64, generator=torch.Generator().manual_seed(0))
    qkv[..., 64:73] = F.one_hot(lab, 9).float()
    img = nat.window_bias_image(torch.zeros(heads, 49, 49, device="cuda"))
    got = nat.window_attention(qkv.to(torch.bfloat16).cuda(), img, ws, shift, heads, 32 ** -0.5).float().cpu()[..., :9]
    own = F.one_hot(lab, 9).bool().expand(2, n, n, 9)
    assert float(got[~own].abs().max()) <= 1e-30                          # exp(-100 + a logit difference of order 10)
    assert float((got[own] - 1.0).abs().max()) <= 2 ** -7                 # the bf16 probabilities of a row sum to 1


def test_window_attention_refuses_what_it_does_not_tile(nat):
    """window 12 (the 384 px presets), head dim 64 (C != 32 heads), a grid that is no multiple of the window, a shift
    outside the window: an error status and no launch"""
    x = torch.zeros(1, 24, 24, 768, dtype=torch.bfloat16, device="cuda")
    out = torch.full((1, 24, 24, 256), 3.0, dtype=torch.bfloat16, device="cuda")
    img = torch.zeros(4, 64, 64, device="cuda")
    call = nat.lib().basd_window_attention_fwd_bf16
    bad = [dict(ws=12), dict(C=256), dict(H=20), dict(W=22), dict(shift=8), dict(ld_qkv=380), dict(ld_out=120)]
    for change in bad:
        a = dict(B=1, H=24, W=24, heads=4, C=128, ws=8, shift=4, ld_qkv=768, ld_out=256)
        a.update(change)
        rc = call(nat._ptr(x), nat._ptr(img), a["B"], a["H"], a["W"], a["heads"], a["C"], a["ws"], a["shift"], a["ld_qkv"],
                  a["ld_out"], 0.17, nat._ptr(out), nat._stream())
        assert rc != 0, change
        assert b"window_attention_fwd" in nat.lib().basd_last_error()
    torch.cuda.synchronize()
    assert float((out.float() - 3.0).abs().max()) == 0.0                  # nothing ran
    assert not nat.window_attention_supported(24, 24, 12, 6, 4, 128, 384, 128)
    assert not nat.window_attention_supported(24, 24, 8, 4, 4, 256, 768, 256)
    assert not nat.window_attention_supported(20, 24, 8, 4, 4, 128, 384, 128)
    assert nat.window_attention_supported(24, 24, 8, 4, 4, 128, 384, 128)
    with pytest.raises(nat.BasdNativeError):
        nat.window_attention(x, img, 12, 6, 4, 0.17)


PM_CASES = [  # B, H, W, C, ld_in
    (2, 56, 56, 96, 128), (2, 28, 28, 192, 192), (2, 14, 14, 384, 384), (3, 6, 10, 128, 128), (2, 2, 2, 96, 128)]


@pytest.mark.parametrize("B,H,W,C,ld_in", PM_CASES)
def test_patch_merge_ln_against_fp64(nat, B, H, W, C, ld_in):
    g = torch.Generator().manual_seed(C + H)
    x = torch.full((B, H, W, ld_in), 7.0).to(torch.bfloat16)             # pad columns of the input are never read
    x[..., :C] = _features((B, H, W, C), seed=H * W + C)
    gamma = 1.0 + 0.2 * torch.randn(4 * C, generator=g)
    beta = 0.1 * torch.randn(4 * C, generator=g)
    got = nat.patch_merge_ln(x.cuda(), C, gamma.cuda(), beta.cuda(), 1e-5)
    torch.cuda.synchronize()
    assert got.shape == (B, H // 2, W // 2, 4 * C) and got.dtype == torch.bfloat16 and got.is_contiguous()

    def ref(dev, dt):
        return F.layer_norm(R.patch_merge(x[..., :C].to(dev, dt)), (4 * C,), gamma.to(dev, dt), beta.to(dev, dt), 1e-5)
    want = ref("cpu", torch.float64)
    yard = ref("cuda", torch.float32).to(torch.bfloat16)
    r_k, r_y, m_k, m_y = _errors(got, yard, want)
    print(f"patch_merge_ln {B}x{H}x{W}x{C}: rel-L2 kernel {r_k:.3e} yardstick {r_y:.3e} ratio {r_k / r_y:.3f}; "
          f"max-abs kernel {m_k:.3e} yardstick {m_y:.3e} ratio {m_k / m_y:.3f}")
    assert r_k <= 2.0 * r_y and m_k <= 2.0 * m_y
    again = nat.patch_merge_ln(x.cuda(), C, gamma.cuda(), beta.cuda(), 1e-5)
    assert torch.equal(again, got)                                        # fixed summation order


def test_patch_merge_neighbour_order(nat):
    """an input whose value encodes (row parity, column parity): with gamma = 1 and beta = 0 the four quarters of an
    output row are the normalised codes in the order (0, 0), (1, 0), (0, 1), (1, 1)"""
    B, H, W, C = 2, 6, 10, 16
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    code = (2 * (yy % 2) + 4 * (xx % 2)).float()                          # (0,0) 0, (1,0) 2, (0,1) 4, (1,1) 6
    x = code[None, :, :, None].expand(B, H, W, C).contiguous().to(torch.bfloat16)
    got = nat.patch_merge_ln(x.cuda(), C, torch.ones(4 * C).cuda(), torch.zeros(4 * C).cuda(), 1e-5).float().cpu()
    want = (torch.tensor([0.0, 2.0, 4.0, 6.0]) - 3.0) / (5.0 + 1e-5) ** 0.5
    assert torch.allclose(got.reshape(-1, 4, C), want[None, :, None].expand(B * 15, 4, C), atol=2 ** -7, rtol=0)


def test_patch_merge_refuses_what_it_does_not_tile(nat):
    x = torch.zeros(1, 4, 4, 1040, dtype=torch.bfloat16, device="cuda")
    y = torch.full((1, 2, 2, 4160), 3.0, dtype=torch.bfloat16, device="cuda")
    f = torch.zeros(4160, device="cuda")
    call = nat.lib().basd_patch_merge_ln_bf16
    for H, W, C, ld in [(4, 4, 1032, 1040), (3, 4, 96, 128), (4, 5, 96, 128), (4, 4, 100, 104), (4, 4, 96, 88), (4, 4, 96, 100)]:
        assert call(nat._ptr(x), nat._ptr(f), nat._ptr(f), 1, H, W, C, ld, 1e-5, nat._ptr(y), nat._stream()) != 0, (H, W, C, ld)
    torch.cuda.synchronize()
    assert float((y.float() - 3.0).abs().max()) == 0.0
    assert not nat.patch_merge_ln_supported(1032, 1040) and not nat.patch_merge_ln_supported(96, 128, 3, 4)
    assert nat.patch_merge_ln_supported(1024, 1024) and nat.patch_merge_ln_supported(96, 128, 56, 56)
