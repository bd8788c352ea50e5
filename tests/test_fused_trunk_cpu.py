"""What the three fused teacher trunks share (models/fused_trunk.py) without a GPU: the state protocol of the weight
images, pinned for ResNet, ConvNeXt-V2 and Swin alike on their emulated providers, and the image helpers against
explicit indexing and ``F.conv2d`` in fp64."""
import pytest
import torch
import torch.nn.functional as F

from tests import _convnext_emul, _resnet_emul, _swin_emul
from tests._teacher_cases import bf16_frozen

TINY = (96, 192, 384, 768)


def _resnet():
    from basd_amd.models.cnn import ResNet
    return ResNet((1, 1, 1, 1))


def _convnext():
    from basd_amd.models.convnext import ConvNeXtV2
    return ConvNeXtV2((1, 1, 1, 1), TINY)


def _swin():
    from basd_amd.models.swin import SwinTransformer
    return SwinTransformer((1, 1, 1, 1), TINY, (3, 6, 12, 24), window_size=4)


# size: the smallest the trunk takes (Swin: grids 32, 16, 8, 4 at window 4).  keys / modules / sentinels: state_dict()
# and named_modules() of the preset as recorded before the trunks shared a base (first, middle and last key).
TRUNKS = {
    "resnet": dict(emul=_resnet_emul, make=_resnet, size=32, name="resnet trunk", fp32_reports=False, preset="resnet50",
                   keys=318, modules=150,
                   sentinels=("conv1.weight", "layer3.0.bn3.running_mean", "layer4.2.bn3.num_batches_tracked")),
    "convnext": dict(emul=_convnext_emul, make=_convnext, size=32, name="convnext trunk", fp32_reports=True,
                     preset="convnextv2_tiny", keys=196, modules=168,
                     sentinels=("stem.0.weight", "stages.2.blocks.2.mlp.grn.weight", "stages.3.blocks.2.mlp.fc2.bias")),
    "swin": dict(emul=_swin_emul, make=_swin, size=128, name="swin trunk", fp32_reports=True,
                 preset="swin_tiny_patch4_window7_224", keys=171, modules=145,
                 sentinels=("patch_embed.proj.weight", "layers.2.blocks.1.mlp.fc1.bias", "norm.bias")),
}


@pytest.fixture(params=sorted(TRUNKS))
def trunk(request):
    from basd_amd.losses import _ops
    case = TRUNKS[request.param]
    _ops.set_ops(case["emul"])
    yield case
    _ops.set_ops(None)


def _zeros(case, dtype):
    return torch.zeros(1, 3, case["size"], case["size"], dtype=dtype)


def test_prepare_needs_a_frozen_model_and_a_cast_drops_the_images(trunk):
    model = trunk["make"]().to(torch.bfloat16).eval()
    assert not model.prepare_fused() and model._fused is None          # parameters still require grad
    model = bf16_frozen(model)
    assert model.fused_refusal() is None and model.prepare_fused() and model._fused is not None
    x = _zeros(trunk, torch.bfloat16)
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


def test_unprepared_bf16_forward_is_named_under_strict_mode(trunk):
    import basd_amd.losses._ops as O
    model = bf16_frozen(trunk["make"]())
    O.FALLBACKS.clear()
    O.set_strict(True)
    try:
        with pytest.raises(O.StrictModeError, match=trunk["name"] + ".*prepared=False"), torch.no_grad():
            model.forward_features(_zeros(trunk, torch.bfloat16))
        assert dict(O.FALLBACKS) == {trunk["name"]: 1}
    finally:
        O.set_strict(False)
        O.FALLBACKS.clear()


def test_fp32_forward_reports_as_its_class_does(trunk):
    """ResNet reports a bf16 no-grad forward only; ConvNeXt-V2 and Swin report every forward on tensors the provider
    handles, unless the caller declares its library calls (the probe of models/teacher.py)"""
    import basd_amd.losses._ops as O
    model = trunk["make"]().eval()
    x = _zeros(trunk, torch.float32)
    O.FALLBACKS.clear()
    O.set_strict(True)
    try:
        with torch.no_grad():
            if trunk["fp32_reports"]:
                with pytest.raises(O.StrictModeError, match=trunk["name"]):
                    model.forward_features(x)
                O.FALLBACKS.clear()
                with O.declared_library_calls():
                    out = model.forward_features(x)
            else:
                out = model.forward_features(x)
        assert not O.FALLBACKS and out.dtype == torch.float32 and out.shape[0] == 1
    finally:
        O.set_strict(False)
        O.FALLBACKS.clear()


def test_the_base_adds_nothing_to_state_dict_or_modules(trunk):
    from basd_amd.models.cnn import create_cnn
    model = create_cnn(trunk["preset"])
    keys, modules = list(model.state_dict()), [n for n, _ in model.named_modules()]
    assert len(keys) == trunk["keys"] and len(modules) == trunk["modules"]
    assert (keys[0], keys[len(keys) // 2], keys[-1]) == trunk["sentinels"]
    assert not any("fused" in k for k in keys + modules) and model._fused is None
    assert hasattr(model, "prepare_fused")                              # what load_teacher looks for


def test_patch_and_padded_image_times_patch_rows_are_the_convolution():
    """2 images, 5 input channels in rows of 8, a 3 x 3 patch convolution to 12 channels in rows of 16, K = 72 padded to
    80.  All values are bf16, so the products are exact in fp64 up to summation order.  The pad channels of the input
    hold garbage: only zero image columns keep them out."""
    from basd_amd.models.fused_trunk import padded_image, patch_image
    g = torch.Generator().manual_seed(0)
    bf = torch.bfloat16
    weight, bias = torch.randn(12, 5, 3, 3, generator=g).to(bf), torch.randn(12, generator=g).to(bf)
    x = torch.randn(2, 8, 6, 9, generator=g).to(bf)
    w2d = patch_image(weight, 8)
    assert w2d.shape == (12, 72) and w2d.dtype == bf
    for i in range(3):
        for j in range(3):
            tap = w2d[:, (i * 3 + j) * 8:(i * 3 + j + 1) * 8]
            assert torch.equal(tap[:, :5], weight[:, :, i, j]) and float(tap[:, 5:].abs().max()) == 0.0
    w_img, b_img = padded_image(w2d, bias, 16, 80)
    assert w_img.shape == (16, 80) and b_img.shape == (16,) and w_img.dtype == b_img.dtype == bf and w_img.is_contiguous()
    assert torch.equal(w_img[:12, :72], w2d) and torch.equal(b_img[:12], bias)
    assert float(w_img[12:].abs().max()) == 0.0 and float(w_img[:, 72:].abs().max()) == 0.0
    assert float(b_img[12:].abs().max()) == 0.0
    rows = _convnext_emul.patchify(x, 3, 80)
    got = rows.double() @ w_img.double().t() + b_img.double()
    want = F.conv2d(x[:, :5].double(), weight.double(), bias.double(), stride=3).permute(0, 2, 3, 1).reshape(-1, 12)
    assert got.shape == (12, 16) and float(got[:, 12:].abs().max()) == 0.0
    assert float((got[:, :12] - want).norm() / want.norm()) <= 1e-12
    # no bias, no padding, and the one rounding of an fp32 (folded) weight
    w32 = torch.randn(12, 5, 3, 3, generator=g)
    assert patch_image(w32).dtype == torch.float32 and torch.equal(patch_image(weight), patch_image(weight, 5))
    w_img, none = padded_image(patch_image(w32), None, 12, 45)
    assert none is None and torch.equal(w_img, w32.permute(0, 2, 3, 1).reshape(12, 45).to(bf))


def test_norm_rows_through_the_centre_tap_equals_the_layernorm_kernel():
    """rows of 16 with 8 channels go through dwconv7_ln and the one-hot centre tap: the same bits as layernorm_fwd on
    rows of 8, pad columns zero whatever they held"""
    from basd_amd.models.fused_trunk import FusedTrunk, centre_tap_identity, norm_params
    E = _convnext_emul
    g = torch.Generator().manual_seed(1)
    ln = torch.nn.LayerNorm(8, eps=1e-5).requires_grad_(False)
    with torch.no_grad():
        ln.weight.normal_(generator=g)
        ln.bias.normal_(generator=g)
    gamma, beta, eps = norm_params(ln.to(torch.bfloat16))
    assert gamma.dtype == beta.dtype == torch.float32 and eps == 1e-5
    w49, zero = centre_tap_identity(8, "cpu")
    assert w49.shape == (49, 8) and float(w49.sum()) == 8.0 and float(w49[24].min()) == 1.0 and zero.dtype == torch.float32
    host = FusedTrunk()
    host._fused = {"ident": {8: (w49, zero)}}
    x = torch.randn(6, 16, generator=g).to(torch.bfloat16)
    wide = host._norm_rows(E, x, 8, gamma, beta, eps)
    narrow = host._norm_rows(E, x[:, :8].contiguous(), 8, gamma, beta, eps)
    assert wide.shape == (6, 16) and torch.equal(wide[:, :8], narrow) and float(wide[:, 8:].abs().max()) == 0.0
