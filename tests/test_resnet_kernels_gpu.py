"""The entries of csrc/resnet.hip against fp64 on the same bf16 inputs.

basd_maxpool3x3s2_bf16, basd_add_relu_bf16 and the p = 1 row gather of basd_patchify_bf16 on a [::2, ::2] view are
exact: bitwise against torch.  For the two convolutions the yardstick is the same arithmetic in torch fp32 on the
device, rounded to bf16 at the same point, on the same tensors: kernel and yardstick differ in fp32 summation order and
nothing else, so the kernel's error against fp64 (rel-L2 and max-abs) may be at most twice the yardstick's (the rule of
DESIGN section 8, as in test_convnext_kernels_gpu.py)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nat():
    import basd_amd._native as native
    native.lib()
    return native


@pytest.fixture(scope="module", autouse=True)
def _fp32_yardstick():
    """the fp32 yardstick convolutions are fp32: no TF32-style shortcuts"""
    prev = torch.backends.cudnn.allow_tf32
    torch.backends.cudnn.allow_tf32 = False
    yield
    torch.backends.cudnn.allow_tf32 = prev


def _features(shape, seed, signed):
    """ReLU-network statistics: signed pre-activations (the ReLU is applied by the kernel) or half-normal
    post-activations, with a few channels 50x larger"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    if not signed:
        x = x.abs()
    c = shape[-1]
    idx = torch.randperm(c, generator=g)[:max(2, c // 48)]
    x[..., idx] *= 50.0
    return x.to(torch.bfloat16)


def _errors(got, yard, want):
    got, yard, want = got.double().cpu(), yard.double().cpu(), want.double()
    scale = float(want.norm())
    return (float((got - want).norm()) / scale, float((yard - want).norm()) / scale,
            float((got - want).abs().max()), float((yard - want).abs().max()))


CONV_CASES = [  # B, H, W, C, stride, ld_in, ld_out, relu_in
    (2, 7, 7, 512, 1, 512, 512, 1), (2, 14, 14, 256, 2, 256, 256, 1), (2, 9, 5, 128, 2, 128, 128, 0),
    (2, 5, 9, 64, 1, 128, 128, 1), (3, 1, 1, 64, 1, 64, 128, 1), (2, 2, 3, 128, 2, 128, 128, 1),
    (4, 56, 56, 64, 1, 128, 128, 1),
    (2, 9, 7, 192, 1, 192, 200, 1), (2, 6, 6, 320, 2, 320, 320, 0), (1, 5, 5, 448, 1, 448, 448, 1)]   # C % 128 != 0


@pytest.mark.parametrize("B,H,W,C,s,ld_in,ld_out,relu_in", CONV_CASES)
def test_conv3x3_against_fp64(nat, B, H, W, C, s, ld_in, ld_out, relu_in):
    g = torch.Generator().manual_seed(C + H + s)
    x = torch.full((B, H, W, ld_in), 7.0).to(torch.bfloat16)            # pad columns of the INPUT are never read
    x[..., :C] = _features((B, H, W, C), seed=H * W + C, signed=bool(relu_in))
    w = (torch.randn(C, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5).to(torch.bfloat16)
    bias = (torch.randn(C, generator=g) * 0.1).to(torch.bfloat16)
    w9 = w.permute(0, 2, 3, 1).reshape(C, 9 * C).contiguous()
    xd = x.cuda()
    got = nat.conv3x3(xd, w9.cuda(), bias.cuda(), stride=s, relu_in=bool(relu_in), relu_out=True, ld_out=ld_out)
    torch.cuda.synchronize()
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    assert got.shape == (B, Ho, Wo, ld_out) and got.dtype == torch.bfloat16
    if ld_out > C:
        assert float(got[..., C:].float().abs().max()) == 0.0
    again = nat.conv3x3(xd, w9.cuda(), bias.cuda(), stride=s, relu_in=bool(relu_in), relu_out=True, ld_out=ld_out)
    assert torch.equal(again, got)

    def ref(dev, dt):
        xin = x[..., :C].to(dev, dt).permute(0, 3, 1, 2)
        if relu_in:
            xin = F.relu(xin)
        return F.relu(F.conv2d(xin, w.to(dev, dt), bias.to(dev, dt), stride=s, padding=1)).permute(0, 2, 3, 1)
    want = ref("cpu", torch.float64)
    yard = ref("cuda", torch.float32).to(torch.bfloat16)
    r_k, r_y, m_k, m_y = _errors(got[..., :C], yard, want)
    print(f"conv3x3 {B}x{H}x{W}x{C} s{s}: rel-L2 kernel {r_k:.3e} yardstick {r_y:.3e} ratio {r_k / r_y:.3f}; "
          f"max-abs kernel {m_k:.3e} yardstick {m_y:.3e} ratio {m_k / m_y:.3f}")
    assert r_k <= 2.0 * r_y and m_k <= 2.0 * m_y


def test_conv3x3_without_the_output_relu(nat):
    """relu_out = 0 keeps the negative results (the epilogue flag is not hard-wired)"""
    g = torch.Generator().manual_seed(1)
    C = 128
    x = _features((2, 6, 5, C), seed=4, signed=True)
    w = (torch.randn(C, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5).to(torch.bfloat16)
    bias = (torch.randn(C, generator=g) * 0.1).to(torch.bfloat16)
    w9 = w.permute(0, 2, 3, 1).reshape(C, 9 * C).contiguous()
    got = nat.conv3x3(x.cuda(), w9.cuda(), bias.cuda(), stride=1, relu_in=False, relu_out=False)

    def ref(dev, dt):
        return F.conv2d(x.to(dev, dt).permute(0, 3, 1, 2), w.to(dev, dt), bias.to(dev, dt), padding=1).permute(0, 2, 3, 1)
    want = ref("cpu", torch.float64)
    yard = ref("cuda", torch.float32).to(torch.bfloat16)
    assert float(got.float().min()) < 0.0
    r_k, r_y, m_k, m_y = _errors(got, yard, want)
    assert r_k <= 2.0 * r_y and m_k <= 2.0 * m_y


@pytest.mark.parametrize("B,H,W", [(2, 32, 32), (2, 30, 34), (2, 224, 224)])
@pytest.mark.parametrize("cl", [False, True], ids=["nchw", "channels-last"])
def test_stem_against_fp64(nat, B, H, W, cl):
    g = torch.Generator().manual_seed(H + W)
    x = torch.randn(B, 3, H, W, generator=g).to(torch.bfloat16)
    w = (torch.randn(64, 3, 7, 7, generator=g) * (2.0 / 147) ** 0.5).to(torch.bfloat16)
    bias = (torch.randn(64, generator=g) * 0.1).to(torch.bfloat16)
    img = torch.zeros(64, nat.STEM_K_PAD, dtype=torch.bfloat16)
    img[:, :147] = w.permute(0, 2, 3, 1).reshape(64, 147)
    xd = x.cuda()
    if cl:
        xd = xd.contiguous(memory_format=torch.channels_last)
    got = nat.conv7x7s2_relu(xd, img.cuda(), bias.cuda(), ld_out=128)
    torch.cuda.synchronize()
    H1, W1 = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    assert got.shape == (B, H1, W1, 128) and float(got[..., 64:].float().abs().max()) == 0.0
    assert torch.equal(nat.conv7x7s2_relu(xd, img.cuda(), bias.cuda(), ld_out=128), got)

    def ref(dev, dt):
        return F.relu(F.conv2d(x.to(dev, dt), w.to(dev, dt), bias.to(dev, dt), stride=2, padding=3)).permute(0, 2, 3, 1)
    want = ref("cpu", torch.float64)
    yard = ref("cuda", torch.float32).to(torch.bfloat16)
    r_k, r_y, m_k, m_y = _errors(got[..., :64], yard, want)
    print(f"stem {B}x{H}x{W} cl={cl}: rel-L2 kernel {r_k:.3e} yardstick {r_y:.3e}; max-abs {m_k:.3e} / {m_y:.3e}")
    assert r_k <= 2.0 * r_y and m_k <= 2.0 * m_y


SIZES = [(2, 112, 112), (3, 9, 5), (2, 18, 18), (2, 1, 1), (2, 5, 8)]


@pytest.mark.parametrize("B,H,W", SIZES)
def test_maxpool_is_exact(nat, B, H, W):
    C, ld = 64, 128
    x = torch.full((B, H, W, ld), 7.0).to(torch.bfloat16)
    x[..., :C] = torch.randn(B, H, W, C, generator=torch.Generator().manual_seed(H)).to(torch.bfloat16)
    got = nat.maxpool3x3s2(x.cuda(), C, ld)
    want = F.max_pool2d(x[..., :C].cuda().permute(0, 3, 1, 2), 3, stride=2, padding=1).permute(0, 2, 3, 1)
    assert got.shape == (B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, ld)
    assert torch.equal(got[..., :C], want) and float(got[..., C:].float().abs().max()) == 0.0


@pytest.mark.parametrize("rows,C,ld_y,ld_r", [(6272, 256, 256, 256), (45, 64, 128, 128), (7, 2048, 2048, 2048),
                                               (50, 64, 128, 64)])
def test_add_relu_is_exact(nat, rows, C, ld_y, ld_r):
    g = torch.Generator().manual_seed(rows)
    y = torch.randn(rows, ld_y, generator=g).to(torch.bfloat16)
    r = torch.randn(rows, ld_r, generator=g).to(torch.bfloat16)
    yd = y.cuda().clone()
    got = nat.add_relu_(yd, r.cuda(), C)
    assert got.data_ptr() == yd.data_ptr()
    want = F.relu(y[:, :C].cuda() + r[:, :C].cuda())                      # bf16 add (one rounding), then ReLU
    assert torch.equal(got[:, :C], want)
    assert torch.equal(got[:, C:].cpu(), y[:, C:])                        # the columns behind C are not touched


@pytest.mark.parametrize("B,H,W", SIZES)
def test_strided_row_gather_through_patchify_is_exact(nat, B, H, W):
    """the stride-2 1 x 1 downsample convolution's input: basd_patchify_bf16 at p = 1 on the [:, :, ::2, ::2] NCHW view
    of padded channels-last rows (64 channels in rows of 128, the pad columns travel along)"""
    ld = 128
    rows = torch.randn(B * H * W, ld, generator=torch.Generator().manual_seed(W)).to(torch.bfloat16).cuda()
    grid = rows.view(B, H, W, ld).permute(0, 3, 1, 2)[:, :, ::2, ::2]
    got = nat.patchify(grid, 1, ld)
    want = rows.view(B, H, W, ld)[:, ::2, ::2, :].reshape(-1, ld)
    assert got.shape == want.shape and torch.equal(got, want)


def test_entries_refuse_what_they_do_not_tile(nat):
    """by argument check, before any launch: through the wrappers and at the C entries"""
    bf = dict(dtype=torch.bfloat16, device="cuda")
    assert not nat.conv3x3_supported(96, 96, 96) and not nat.conv3x3_supported(64, 64, 136)
    assert not nat.conv3x3_supported(64, 64, 64, stride=3) and not nat.conv7x7s2_relu_supported(136)
    assert not nat.maxpool3x3s2_supported(60, 64, 64) and not nat.add_relu_supported(64, 60, 64)
    x96, x64 = torch.zeros(1, 4, 4, 96, **bf), torch.zeros(1, 4, 4, 64, **bf)
    with pytest.raises(nat.BasdNativeError):
        nat.conv3x3(x96, torch.zeros(96, 864, **bf), torch.zeros(96, **bf))
    with pytest.raises(nat.BasdNativeError):
        nat.conv3x3(x64, torch.zeros(64, 576, **bf), torch.zeros(64, **bf), ld_out=136)
    with pytest.raises(nat.BasdNativeError):
        nat.conv3x3(x64, torch.zeros(64, 576, **bf), torch.zeros(64, **bf), stride=3)
    with pytest.raises(nat.BasdNativeError):
        nat.conv7x7s2_relu(torch.zeros(1, 3, 8, 8, **bf), torch.zeros(64, 152, **bf), torch.zeros(64, **bf))
    with pytest.raises(nat.BasdNativeError):
        nat.maxpool3x3s2(x64, 60)
    y = torch.zeros(1, 4, 4, 256, **bf)
    L, p, s = nat.lib(), nat._ptr, nat._stream()
    for args in ((1, 4, 4, 96, 1, 96, 96), (1, 4, 4, 64, 1, 64, 136), (1, 4, 4, 64, 3, 64, 64), (1, 4, 4, 576, 1, 576, 576)):
        with pytest.raises(nat.BasdNativeError):
            nat._check(L.basd_conv3x3_bf16(p(x96), p(x96), p(x96), *args, 1, 1, p(y), s), "conv3x3")
    with pytest.raises(nat.BasdNativeError):
        nat._check(L.basd_conv7x7s2_relu_bf16(p(x96), p(x96), p(x96), 1, 8, 8, 192, 64, 8, 1, 152, 128, p(y), s), "stem")
    with pytest.raises(nat.BasdNativeError):
        nat._check(L.basd_maxpool3x3s2_bf16(p(x64), 1, 4, 4, 60, 64, 64, p(y), s), "maxpool")
    with pytest.raises(nat.BasdNativeError):
        nat._check(L.basd_add_relu_bf16(p(y), p(x64), 16, 64, 60, 64, s), "add_relu")
    torch.cuda.synchronize()
