"""fp32 evaluation kernels on split-bf16 (bf16x3) products (csrc/eval_f32x3.hip), called through the C-ABI wrappers and
compared with fp64 references: GEMM with every epilogue (any M, padded K, student and teacher widths), attention with
fp32 logits, LayerNorm with and without the residual add."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _native():
    import basd_amd._native as native
    from basd_amd.losses import _ops
    native.lib()
    _ops.set_ops(None)
    yield native


def _img(native, a, k_pad=None):
    """split image of an fp32 matrix through the table kernel"""
    return native.split_table([(a.contiguous(), k_pad or a.shape[1])])[0]


def _unsplit(img, n):
    return img[:, :n].float() + img[:, img.shape[1] // 2:img.shape[1] // 2 + n].float()


def test_split_image_layout(_native):
    a = torch.randn(37, 48, device="cuda") * 3
    img = _img(_native, a, 64)
    hi = a.to(torch.bfloat16)
    lo = (a - hi.float()).to(torch.bfloat16)
    assert img.shape == (37, 128)
    assert torch.equal(img[:, :48], hi) and torch.equal(img[:, 64:112], lo)
    assert not img[:, 48:64].float().any() and not img[:, 112:].float().any()


_SHAPES = []
for _d in (192, 384, 640, 768):
    _SHAPES += [(_d, _d, _d), (3 * _d, _d, _d), (4 * _d, _d, _d), (_d, 4 * _d, 4 * _d)]
_SHAPES += [(192, 48, 64), (640, 588, 608), (1024, 1024, 1024), (3840, 1280, 1280), (1280, 5120, 5120)]


def _check_gemm(native, m, n, k, kp, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(m, k, device="cuda", generator=g)
    w = torch.randn(n, k, device="cuda", generator=g) * k ** -0.5
    b = torch.randn(n, device="cuda", generator=g) * 0.1
    xi, wi = _img(native, x, kp), _img(native, w, kp)
    y64 = torch.addmm(b.double(), x.double(), w.double().t())
    bound = 3e-5 * (x.double().abs() @ w.double().abs().t()) + 1e-7 * b.double().abs() + 1e-30
    y = native.gemm_f32x3(xi, wi, b)
    assert y.dtype == torch.float32 and y.shape == (m, n)
    ratio = float(((y.double() - y64).abs() / bound).max())
    assert ratio <= 1.0, (m, n, k, ratio)
    # exact-erf GELU epilogue (|gelu'| <= 1.13)
    yg = native.gemm_f32x3(xi, wi, b, gelu=True)
    g64 = torch.nn.functional.gelu(y64)
    ratio_g = float(((yg.double() - g64).abs() / (1.13 * bound + 2e-7 * g64.abs() + 1e-7)).max())
    assert ratio_g <= 1.0, (m, n, k, ratio_g)
    # split outputs reconstruct the fp32 results
    for gelu, ref in ((False, y), (True, yg)):
        yi = native.gemm_f32x3(xi, wi, b, gelu=gelu, split_out=True)
        assert yi.dtype == torch.bfloat16 and yi.shape == (m, 2 * n)
        rec = _unsplit(yi, n).double()
        assert float(((rec - ref.double()).abs() - 2.0 ** -16 * ref.double().abs()).max()) <= 0.0, (m, n, k, gelu)
    return ratio


@pytest.mark.parametrize("n,k,kp", _SHAPES)
@pytest.mark.parametrize("m", [1, 80 * 197])
def test_gemm_f32x3_matches_fp64(_native, m, n, k, kp):
    _check_gemm(_native, m, n, k, kp, seed=m + n + k)


@pytest.mark.parametrize("n,k", [(576, 192), (768, 3072), (3072, 768)])
def test_gemm_f32x3_full_batch(_native, n, k):
    _check_gemm(_native, 256 * 197, n, k, k, seed=n + k)


@pytest.mark.parametrize("m", [2, 15, 127, 129, 300])
def test_gemm_f32x3_ragged_rows(_native, m):
    _check_gemm(_native, m, 384, 192, 192, seed=m)


def test_gemm_f32x3_rejects_unsupported_shapes(_native):
    x = torch.zeros(4, 2 * 40, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(_native.BasdNativeError):
        _native.gemm_f32x3(x, x[:4], None)                  # k_pad = 40 is not a multiple of 32


def _attn64(q, k, v, scale):
    s = (q @ k.transpose(-2, -1)) * scale
    return torch.softmax(s, dim=-1) @ v


@pytest.mark.parametrize("hd", [64, 80])
@pytest.mark.parametrize("t", [65, 197, 257, 272])
def test_attention_f32x3_matches_fp64(_native, hd, t):
    b, h = 2, 3
    g = torch.Generator(device="cuda").manual_seed(t * hd)
    qkv = torch.randn(b, t, 3, h, hd, device="cuda", generator=g)
    qkv[:, :, :2] *= 2.6                                  # logits q.k / sqrt(hd) of std ~7: spans about +-20 and beyond
    qkv = qkv.reshape(b, t, 3 * h * hd)
    scale = hd ** -0.5
    out = _native.attention_fwd_f32x3(qkv, h, hd, scale)
    assert out.shape == (b * t, 2 * h * hd) and out.dtype == torch.bfloat16
    o = _unsplit(out, h * hd).double().view(b, t, h, hd).permute(0, 2, 1, 3).cpu()
    q, k, v = qkv.double().cpu().view(b, t, 3, h, hd).permute(2, 0, 3, 1, 4).unbind(0)
    logits = (q @ k.transpose(-2, -1)) * scale
    assert float(logits.abs().max()) > 20.0
    want = _attn64(q, k, v, scale)
    err = (o - want).abs().amax(dim=(2, 3))                   # [B, H]
    vmax = v.abs().amax(dim=(2, 3))
    assert bool((err <= 5e-5 * vmax).all()), float((err / vmax).max())


@pytest.mark.parametrize("d", [192, 384, 640, 768, 1280])
@pytest.mark.parametrize("add", [False, True])
def test_layernorm_f32_matches_fp64(_native, d, add):
    rows = 1000
    g = torch.Generator(device="cuda").manual_seed(d + add)
    x = torch.randn(rows, d, device="cuda", generator=g) * 2 + 0.5
    res = torch.randn(rows, d, device="cuda", generator=g) if add else None
    ls = torch.rand(d, device="cuda", generator=g) + 0.5 if add else None
    gamma = 1 + 0.2 * torch.randn(d, device="cuda", generator=g)
    beta = 0.1 * torch.randn(d, device="cuda", generator=g)
    s, y, img = _native.add_layernorm_f32(x, gamma, beta, 1e-6, residual=res, xscale=ls, want_s=True, want_y=True,
                                          want_img=True)
    s64 = x.double() * (ls.double() if add else 1.0) + (res.double() if add else 0.0)
    y64 = torch.nn.functional.layer_norm(s64, (d,), gamma.double(), beta.double(), 1e-6)
    assert float((s.double() - s64).abs().max()) <= 1e-5
    assert float((y.double() - y64).abs().max()) <= 1e-5
    rec = _unsplit(img, d).double()
    assert float(((rec - y.double()).abs() - 2.0 ** -16 * y.double().abs()).max()) <= 0.0
