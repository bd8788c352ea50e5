"""The entries of csrc/convnext.hip against fp64 on the same bf16 inputs.

basd_patchify_bf16 is a copy: bitwise.  For basd_dwconv7_ln_bf16 and basd_grn_bf16 the yardstick is the same arithmetic
in torch fp32 on the device, rounded to bf16 at the same point, on the same tensor: the kernel and the yardstick may
differ in fp32 summation order and nothing else, so the kernel's error against fp64 (rel-L2 and max-abs) may be at most
twice the yardstick's (the rule of DESIGN section 8)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nat():
    import basd_amd._native as native
    native.lib()
    return native


def _features(shape, seed, outliers=True):
    """feature-map statistics of a ConvNeXt: unit-scale channels plus a few whose magnitude is 50 - 100 times larger"""
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


DW_CASES = [  # B, H, W, C, ld_in, ld_out
    (2, 56, 56, 96, 128, 128), (2, 28, 28, 192, 192, 192), (2, 14, 14, 384, 384, 384), (2, 7, 7, 768, 768, 768),
    (3, 5, 5, 96, 128, 128), (2, 9, 13, 192, 192, 192), (4, 1, 1, 384, 384, 384), (2, 9, 13, 96, 96, 128),
    (2, 6, 7, 80, 128, 128), (16, 56, 56, 96, 128, 128)]


@pytest.mark.parametrize("B,H,W,C,ld_in,ld_out", DW_CASES)
def test_dwconv7_ln_against_fp64(nat, B, H, W, C, ld_in, ld_out):
    g = torch.Generator().manual_seed(C + H)
    x = torch.full((B, H, W, ld_in), 7.0).to(torch.bfloat16)            # pad columns of the INPUT are never read
    x[..., :C] = _features((B, H, W, C), seed=H * W + C)
    w = (torch.randn(C, 1, 7, 7, generator=g) * 0.15).to(torch.bfloat16)
    bias = (torch.randn(C, generator=g) * 0.1).to(torch.bfloat16).float()
    gamma = 1.0 + 0.2 * torch.randn(C, generator=g)
    beta = 0.1 * torch.randn(C, generator=g)
    w49 = w.reshape(C, 49).t().contiguous()
    got = nat.dwconv7_ln(x.cuda(), w49.cuda(), bias.cuda(), gamma.cuda(), beta.cuda(), 1e-6, ld_out=ld_out)
    torch.cuda.synchronize()
    assert got.shape == (B, H, W, ld_out) and got.dtype == torch.bfloat16
    if ld_out > C:
        assert float(got[..., C:].float().abs().max()) == 0.0

    def ref(dev, dt):
        y = F.conv2d(x[..., :C].to(dev, dt).permute(0, 3, 1, 2), w.to(dev, dt), bias.to(dev, dt), padding=3, groups=C)
        return F.layer_norm(y.permute(0, 2, 3, 1), (C,), gamma.to(dev, dt), beta.to(dev, dt), 1e-6)
    want = ref("cpu", torch.float64)
    yard = ref("cuda", torch.float32).to(torch.bfloat16)
    r_k, r_y, m_k, m_y = _errors(got[..., :C], yard, want)
    print(f"dwconv7_ln {B}x{H}x{W}x{C}: rel-L2 kernel {r_k:.3e} yardstick {r_y:.3e} ratio {r_k / r_y:.3f}; "
          f"max-abs kernel {m_k:.3e} yardstick {m_y:.3e} ratio {m_k / m_y:.3f}")
    assert r_k <= 2.0 * r_y and m_k <= 2.0 * m_y


def test_layernorm_over_padded_rows_through_the_centre_tap(nat):
    """H = W = 1 with the one-hot centre tap: LayerNorm over 96 of 128 columns (the stem's norm of ConvNeXt-T)"""
    rows, C, ld = 5000, 96, 128
    x = torch.zeros(rows, ld).to(torch.bfloat16)
    x[:, :C] = _features((rows, C), seed=3)
    g = torch.Generator().manual_seed(5)
    gamma, beta = 1.0 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    w49 = torch.zeros(49, C).to(torch.bfloat16)
    w49[24] = 1.0
    got = nat.dwconv7_ln(x.view(rows, 1, 1, ld).cuda(), w49.cuda(), torch.zeros(C).cuda(), gamma.cuda(), beta.cuda(), 1e-6)
    want = F.layer_norm(x[:, :C].double(), (C,), gamma.double(), beta.double(), 1e-6)
    yard = F.layer_norm(x[:, :C].cuda().float(), (C,), gamma.cuda(), beta.cuda(), 1e-6).to(torch.bfloat16)
    got = got.view(rows, ld)
    assert float(got[:, C:].float().abs().max()) == 0.0
    r_k, r_y, m_k, m_y = _errors(got[:, :C], yard, want)
    print(f"centre-tap LayerNorm: rel-L2 kernel {r_k:.3e} yardstick {r_y:.3e}; max-abs {m_k:.3e} / {m_y:.3e}")
    assert r_k <= 2.0 * r_y and m_k <= 2.0 * m_y


GRN_CASES = [(2, 3136, 384), (2, 784, 768), (2, 196, 1536), (2, 49, 3072), (3, 25, 384), (2, 117, 768), (4, 1, 1536),
             (2, 300, 320), (24, 3136, 384)]


@pytest.mark.parametrize("B,HW,C", GRN_CASES)
def test_grn_against_fp64(nat, B, HW, C):
    x = F.gelu(_features((B, HW, C), seed=HW + C).float()).to(torch.bfloat16)      # what fc1's epilogue leaves
    g = torch.Generator().manual_seed(C)
    weight, bias = 0.3 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)

    def ref(dev, dt):
        xf = x.to(dev, dt)
        gg = (xf * xf).sum(dim=1, keepdim=True).sqrt()
        n = gg / (gg.mean(dim=-1, keepdim=True) + 1e-6)
        return xf + (bias.to(dev, dt) + weight.to(dev, dt) * (xf * n))
    want = ref("cpu", torch.float64)
    yard = ref("cuda", torch.float32).to(torch.bfloat16)
    xd = x.cuda().clone()
    got = nat.grn_(xd, weight.cuda(), bias.cuda(), 1e-6)
    torch.cuda.synchronize()
    assert got.data_ptr() == xd.data_ptr()
    r_k, r_y, m_k, m_y = _errors(got, yard, want)
    print(f"grn {B}x{HW}x{C}: rel-L2 kernel {r_k:.3e} yardstick {r_y:.3e} ratio {r_k / r_y:.3f}; "
          f"max-abs kernel {m_k:.3e} yardstick {m_y:.3e} ratio {m_k / m_y:.3f}")
    assert r_k <= 2.0 * r_y and m_k <= 2.0 * m_y
    again = nat.grn_(x.cuda().clone(), weight.cuda(), bias.cuda(), 1e-6)            # fixed summation order
    assert torch.equal(again, got)


PATCH_CASES = [  # B, C, H, W, p, K_pad, channels_last
    (2, 3, 224, 224, 4, 64, False), (2, 3, 224, 224, 4, 64, True), (2, 128, 56, 56, 2, 512, True),
    (2, 192, 28, 28, 2, 768, True), (2, 384, 14, 14, 2, 1536, True), (3, 8, 6, 10, 2, 64, True),
    (2, 12, 6, 10, 2, 64, True), (2, 16, 2, 2, 2, 64, False), (64, 128, 56, 56, 2, 512, True)]


@pytest.mark.parametrize("B,C,H,W,p,K_pad,cl", PATCH_CASES)
def test_patchify_is_exact(nat, B, C, H, W, p, K_pad, cl):
    x = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(C + H)).to(torch.bfloat16)
    xd = x.cuda()
    if cl:
        xd = xd.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)               # channels-last rows, NCHW view
    got = nat.patchify(xd, p, K_pad)
    torch.cuda.synchronize()
    want = torch.zeros(B * (H // p) * (W // p), K_pad, dtype=torch.bfloat16)
    want[:, :C * p * p] = x.reshape(B, C, H // p, p, W // p, p).permute(0, 2, 4, 3, 5, 1).reshape(-1, p * p * C)
    assert torch.equal(got.cpu(), want)


def test_patch_rows_times_weight_image_is_the_strided_convolution(nat):
    """the gather order and the weight re-layout belong together: patches x image == conv2d(stride p)"""
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 128, 8, 8, generator=g).to(torch.bfloat16)
    w = (torch.randn(192, 128, 2, 2, generator=g) * 0.05).to(torch.bfloat16)
    xd = x.cuda().permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    rows = nat.patchify(xd, 2, 512)
    y = nat.gemm_bf16(rows, w.permute(0, 2, 3, 1).reshape(192, 512).contiguous().cuda())
    want = F.conv2d(x.double(), w.double(), stride=2).permute(0, 2, 3, 1).reshape(-1, 192)
    assert float((y.double().cpu() - want).norm() / want.norm()) < 4e-3            # one bf16 rounding of the output


def test_entries_refuse_what_they_do_not_tile(nat):
    x = torch.zeros(1, 4, 4, 100, dtype=torch.bfloat16, device="cuda")
    assert not nat.dwconv7_ln_supported(100, 104, 104) and not nat.grn_supported(4104)
    with pytest.raises(nat.BasdNativeError):
        nat._check(nat.lib().basd_dwconv7_ln_bf16(nat._ptr(x), nat._ptr(x), nat._ptr(x), nat._ptr(x), nat._ptr(x), 1, 4, 4,
                                                  100, 104, 104, 1e-6, nat._ptr(x), nat._stream()), "dwconv7_ln")
    ws = torch.zeros(8, dtype=torch.uint8, device="cuda")
    h = torch.zeros(1, 4, 384, dtype=torch.bfloat16, device="cuda")
    f = torch.zeros(384, device="cuda")
    assert nat.lib().basd_grn_workspace_bytes(1, 4, 384) == 384 * 4
    with pytest.raises(nat.BasdNativeError):
        nat._check(nat.lib().basd_grn_bf16(nat._ptr(h), nat._ptr(f), nat._ptr(f), 1, 4, 384, 1e-6, nat._ptr(ws), 8,
                                           nat._stream()), "grn")
