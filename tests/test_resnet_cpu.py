"""The fused ResNet trunk without a GPU: the BatchNorm fold and the weight images against explicit formulas, and
``_forward_fused`` on the emulated entries (tests/_resnet_emul.py) against the fp64 restatement (tests/_resnet_ref.py)
with the module's own plain bf16 forward as the yardstick."""
import pytest
import torch
import torch.nn.functional as F

from tests import _resnet_emul, _resnet_ref as R


@pytest.fixture
def emulated_kernels():
    from basd_amd.losses import _ops
    _ops.set_ops(_resnet_emul)
    yield _resnet_emul
    _ops.set_ops(None)


def _bf16_teacher(model):
    model = model.to(torch.bfloat16)
    for p in model.parameters():
        p.requires_grad = False
    return model.eval()


def _small(depths, seed):
    from basd_amd.models.cnn import ResNet
    torch.manual_seed(seed)
    return _bf16_teacher(R.randomise_bn(ResNet(depths), seed=seed + 10))


def test_module_forward_equals_the_fp64_restatement():
    """the restatement is the module's architecture: fp32 module against fp64 restatement, bounded by 10x the
    restatement's own fp32 error"""
    from basd_amd.models.cnn import ResNet
    torch.manual_seed(0)
    depths = (2, 1, 1, 1)
    model = R.randomise_bn(ResNet(depths), seed=3).eval()
    x = torch.randn(2, 3, 72, 72)
    with torch.no_grad():
        got = model.forward_features(x)
    want = R.forward_features(model.state_dict(), x, depths)
    own = R.forward_features(model.state_dict(), x, depths, dtype=torch.float32)
    assert got.shape == want.shape == (2, 2048, 3, 3)
    err = float(R.rel_l2_per_sample(got, want).max())
    bound = 10.0 * float(R.rel_l2_per_sample(own, want).max())
    assert 0.0 < bound < 1e-4 and err <= bound, (err, bound)


@pytest.mark.parametrize("depths,size", [((1, 1, 1, 1), 64), ((2, 1, 1, 1), 72)], ids=["1111-64px", "2111-72px"])
def test_fused_forward_on_emulated_kernels_against_fp64(emulated_kernels, depths, size):
    """Both bf16 paths are measured against fp64 on the same bf16 weights; the fused path (folded BatchNorm, rounding
    after every convolution + bias) may err at most twice as much per sample as the plain bf16 forward (DESIGN
    section 8's rule).  Every BatchNorm is random, so a wrong fold, a dropped bias image or a wrong tap order gives an
    error of order 1.  At 72 px the maps are 18, 9, 5, 3: odd sizes in front of the stride-2 3 x 3 convolution and the
    stride-2 row gather."""
    model = _small(depths, seed=1)
    assert model.fused_refusal() is None and model.prepare_fused()
    x = torch.randn(2, 3, size, size, generator=torch.Generator().manual_seed(2)).to(torch.bfloat16)
    with torch.no_grad():
        got = model.forward_features(x)
        assert model._takes_fused(x)
        plain = model._forward_plain(x)
    hw = (size + 31) // 32
    assert got.shape == plain.shape == (2, 2048, hw, hw) and got.dtype == torch.bfloat16
    want = R.forward_features(model.state_dict(), x, depths)
    e_f, e_p = R.rel_l2_per_sample(got, want), R.rel_l2_per_sample(plain, want)
    print(f"fused (emulated) vs fp64 {e_f.tolist()}, plain bf16 vs fp64 {e_p.tolist()}")
    assert bool((e_f <= 2.0 * e_p).all()), (e_f.tolist(), e_p.tolist())


def test_a_dropped_bias_image_is_seen(emulated_kernels):
    model = _small((1, 1, 1, 1), seed=1)
    assert model.prepare_fused()
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(2)).to(torch.bfloat16)
    with torch.no_grad():
        plain = model._forward_plain(x)
        good = float(R.rel_l2_per_sample(model.forward_features(x), plain).max())
        model._fused["blocks"][0]["c2"][1].zero_()
        bad = float(R.rel_l2_per_sample(model.forward_features(x), plain).max())
    assert good < 3e-2 < bad, (good, bad)


def test_batchnorm_fold_is_exact_in_fp64():
    """folded convolution + bias == convolution then BatchNorm, both in fp64, to 1e-12 relative"""
    g = torch.Generator().manual_seed(0)
    conv = torch.nn.Conv2d(16, 24, 3, padding=1, bias=False).double()
    bn = R.randomise_bn(torch.nn.BatchNorm2d(24), seed=4).double().eval()
    x = torch.randn(2, 16, 9, 7, generator=g, dtype=torch.float64)
    with torch.no_grad():
        want = bn(conv(x))
        s = bn.weight / torch.sqrt(bn.running_var + bn.eps)
        got = F.conv2d(x, conv.weight * s.view(-1, 1, 1, 1), bn.bias - bn.running_mean * s, padding=1)
    assert float((got - want).norm() / want.norm()) <= 1e-12


def _im2col(x, k, stride, padding):
    """[B, C, H, W] -> [B Ho Wo, (dy k + dx) C + c] by explicit indexing"""
    b, c, h, w = x.shape
    xp = F.pad(x, (padding,) * 4)
    ho, wo = (h + 2 * padding - k) // stride + 1, (w + 2 * padding - k) // stride + 1
    cols = torch.zeros(b, ho, wo, k * k * c, dtype=x.dtype)
    for dy in range(k):
        for dx in range(k):
            patch = xp[:, :, dy:dy + stride * (ho - 1) + 1:stride, dx:dx + stride * (wo - 1) + 1:stride]
            cols[..., (dy * k + dx) * c:(dy * k + dx + 1) * c] = patch.permute(0, 2, 3, 1)
    return cols.reshape(b * ho * wo, k * k * c)


def test_weight_images_times_im2col_are_the_convolutions(emulated_kernels):
    """the prepared images, read as the kernels read them: tap-major w9 and the stem image times an explicit im2col
    equal conv2d of the folded weights; the 1 x 1 images are zero-padded [N_ld, K_ld]"""
    model = _small((1, 1, 1, 1), seed=5)
    assert model.prepare_fused()
    fz = model._fused
    g = torch.Generator().manual_seed(6)

    def folded(conv, bn):
        s = bn.weight.float() / torch.sqrt(bn.running_var.float() + bn.eps)
        return ((conv.weight.float() * s.view(-1, 1, 1, 1)).to(torch.bfloat16).double(),
                (bn.bias.float() - bn.running_mean.float() * s).to(torch.bfloat16).double())

    # stem
    w_img, b_img = fz["stem"]
    assert w_img.shape == (64, 160) and float(w_img[:, 147:].abs().max()) == 0.0
    wf, bf = folded(model.conv1, model.bn1)
    x = torch.randn(2, 3, 11, 14, generator=g, dtype=torch.float64)
    want = F.conv2d(x, wf, bf, stride=2, padding=3).permute(0, 2, 3, 1).reshape(-1, 64)
    got = _im2col(x, 7, 2, 3) @ w_img[:, :147].double().t() + b_img.double()
    assert float((got - want).norm() / want.norm()) < 1e-12
    # 3 x 3, stride 2 (layer2.0) and stride 1 (layer1.0)
    for rec, blk in ((fz["blocks"][1], model.layer2[0]), (fz["blocks"][0], model.layer1[0])):
        p, s = rec["planes"], rec["stride"]
        w9, b9 = rec["c2"]
        assert w9.shape == (p, 9 * p) and s == blk.conv2.stride[0]
        wf, bf = folded(blk.conv2, blk.bn2)
        x = torch.randn(2, p, 5, 6, generator=g, dtype=torch.float64)
        want = F.conv2d(x, wf, bf, stride=s, padding=1).permute(0, 2, 3, 1).reshape(-1, p)
        got = _im2col(x, 3, s, 1) @ w9.double().t() + b9.double()
        assert float((got - want).norm() / want.norm()) < 1e-12
    # 1 x 1 images of layer1.0: 64 channels in rows of 128
    rec, blk = fz["blocks"][0], model.layer1[0]
    w1, b1 = rec["c1"]
    assert w1.shape == (128, 128) and b1.shape == (128,)
    assert float(w1[64:].abs().max()) == 0.0 and float(w1[:, 64:].abs().max()) == 0.0 and float(b1[64:].abs().max()) == 0.0
    wf, bf = folded(blk.conv1, blk.bn1)
    assert torch.equal(w1[:64, :64].double(), wf.flatten(1)) and torch.equal(b1[:64].double(), bf)
    w3, b3 = rec["c3"]
    assert w3.shape == (256, 128) and float(w3[:, 64:].abs().max()) == 0.0 and float(w3[:, :64].abs().max()) > 0.0
    wd, bd = rec["down"]
    assert wd.shape == (256, 128) and float(wd[:, 64:].abs().max()) == 0.0 and bd.shape == (256,)


def test_prepare_needs_a_frozen_model_and_a_cast_drops_the_images(emulated_kernels):
    from basd_amd.models.cnn import ResNet
    model = ResNet((1, 1, 1, 1)).to(torch.bfloat16).eval()
    assert not model.prepare_fused() and model._fused is None          # parameters still require grad
    for p in model.parameters():
        p.requires_grad = False
    assert model.prepare_fused() and model._fused is not None
    x = torch.zeros(1, 3, 32, 32, dtype=torch.bfloat16)
    with torch.no_grad():
        assert model._takes_fused(x)
    assert not model._takes_fused(x)                                    # grad mode: the plain path
    model.float()
    assert model._fused is None
    assert model.prepare_fused()
    with torch.no_grad():
        assert not model._takes_fused(x)                                # fp32 weights
    model.to(torch.bfloat16)
    assert model._fused is None


def test_refused_bf16_forward_reports_instead_of_hiding(emulated_kernels):
    """an unprepared bf16 no-grad forward on tensors the provider handles goes through library_fallback (strict mode
    names it); other dtypes stay unreported"""
    import basd_amd.losses._ops as O
    from basd_amd.models.cnn import ResNet
    model = ResNet((1, 1, 1, 1)).eval()
    O.FALLBACKS.clear()
    O.set_strict(True)
    try:
        with torch.no_grad():
            model.forward_features(torch.zeros(1, 3, 32, 32))          # fp32: unreported
            model.to(torch.bfloat16)
            with pytest.raises(O.StrictModeError):
                model.forward_features(torch.zeros(1, 3, 32, 32, dtype=torch.bfloat16))
    finally:
        O.set_strict(False)
        O.FALLBACKS.clear()


def test_cpu_teacher_takes_the_plain_path():
    from basd_amd.models import extract_intermediates, load_teacher
    teacher = load_teacher("resnet50", 64, device="cpu")
    assert teacher.model._fused is None and teacher.feature_format == "nchw" and teacher.embed_dim == 2048
    tok, imp = extract_intermediates(teacher, torch.randn(2, 3, 64, 64))
    assert tok[0].shape == (2, 4, 2048) and torch.equal(imp[0], torch.full((2, 4), 0.25))
