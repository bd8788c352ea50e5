"""fp32 "high" evaluation attention for up to 1024 tokens (attn_f32x3_long_kernel, basd_attention_fwd_f32x3_long): the
kernel against fp64 with the contract's plain-torch emulation (tests/_f32x3_emul.py) as the yardstick, against the short
kernel at the short kernel's sizes, the dispatch of the wrapper, and the model / evaluate_model in strict mode at 384 px.

Measured on an MI355X: worst err_kernel / max-over-heads err_emul over the nine fp64 cases = 1.07 (bound 2);
errors 2.5e-5 .. 5.1e-5 of max|V| for T > 1, the emulation within 7 % of the same figures.
"""
import copy
import ctypes

import pytest
import torch
import torch.nn as nn

from tests import _f32x3_emul

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _native():
    import basd_amd._native as native
    import basd_amd.losses._ops as O
    native.lib()
    O.set_ops(None)
    O.FALLBACKS.clear()
    prev = torch.get_float32_matmul_precision()
    yield native
    O.set_strict(False)
    torch.set_float32_matmul_precision(prev)


def _unsplit(img, n):
    return img[:, :n].float() + img[:, img.shape[1] // 2:img.shape[1] // 2 + n].float()


def _qkv(b, t, h, hd, seed):
    """the inputs of test_attention_f32x3_matches_fp64: logits q.k / sqrt(hd) of std ~7"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    qkv = torch.randn(b, t, 3, h, hd, device="cuda", generator=g)
    qkv[:, :, :2] *= 2.6
    return qkv.reshape(b, t, 3 * h * hd)


def _fp64(qkv, b, t, h, hd, scale):
    q, k, v = qkv.double().cpu().view(b, t, 3, h, hd).permute(2, 0, 3, 1, 4).unbind(0)
    logits = (q @ k.transpose(-2, -1)) * scale
    return torch.softmax(logits, dim=-1) @ v, v.abs().amax(dim=(2, 3)), float(logits.abs().max())


def _heads(img, b, t, h, hd):
    """image [B T, 2 H hd] -> fp64 [B, H, T, hd] on the CPU"""
    return _unsplit(img, h * hd).double().view(b, t, h, hd).permute(0, 2, 1, 3).cpu()


def _call(native, name, qkv, b, t, h, hd, scale):
    out = torch.empty(b * t, 2 * h * hd, dtype=torch.bfloat16, device="cuda")
    rc = getattr(native.lib(), name)(ctypes.c_void_p(qkv.data_ptr()), b, t, h, hd, ctypes.c_float(scale),
                                     ctypes.c_void_p(out.data_ptr()),
                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, native.lib().basd_last_error()
    return out


_CASES = [(2, 273, 3, 64), (2, 273, 3, 80), (2, 577, 3, 64), (1, 577, 2, 80), (1, 730, 3, 64), (1, 1024, 3, 64),
          (1, 1024, 2, 80), (2, 1, 2, 64), (2, 129, 2, 80)]


@pytest.mark.parametrize("b,t,h,hd", _CASES)
def test_long_kernel_matches_fp64_within_twice_the_emulation(_native, b, t, h, hd):
    """err_kernel <= 2 max_heads err_emul, both against fp64 on the same tensor and relative to max|V| of the head.  The
    kernel may differ from the emulation in the fp32 summation order and in __expf against exp only: a few 1e-6 at
    |x| ~ 40, an order below the 2^-16 split error that sets err_emul; a dropped lo product costs 2^-9."""
    scale = hd ** -0.5
    qkv = _qkv(b, t, h, hd, t * hd)
    out = _call(_native, "basd_attention_fwd_f32x3_long", qkv, b, t, h, hd, scale)
    want, vmax, lmax = _fp64(qkv, b, t, h, hd, scale)
    if t > 1:
        assert lmax > 20.0
    err_k = (_heads(out, b, t, h, hd) - want).abs().amax(dim=(2, 3)) / vmax           # [B, H]
    err_e = (_f32x3_emul.attention_f32x3(qkv, h, hd, scale).double() - want).abs().amax(dim=(2, 3)) / vmax
    print(f"B {b} T {t} H {h} hd {hd}: err_kernel {float(err_k.max()):.3e} err_emul {float(err_e.max()):.3e} "
          f"ratio {float(err_k.max() / err_e.max()):.3f}")
    assert bool((err_k <= 2.0 * err_e.max()).all()), (float(err_k.max()), float(err_e.max()))


@pytest.mark.parametrize("hd", [64, 80])
@pytest.mark.parametrize("t", [65, 197, 272])
def test_long_kernel_agrees_with_the_short_one(_native, hd, t):
    """at the short kernel's sizes the two differ per head by no more than the short kernel's own error against fp64"""
    b, h, scale = 2, 3, hd ** -0.5
    qkv = _qkv(b, t, h, hd, t * hd + 1)
    short = _heads(_call(_native, "basd_attention_fwd_f32x3", qkv, b, t, h, hd, scale), b, t, h, hd)
    long_ = _heads(_call(_native, "basd_attention_fwd_f32x3_long", qkv, b, t, h, hd, scale), b, t, h, hd)
    want, _, _ = _fp64(qkv, b, t, h, hd, scale)
    err_short = (short - want).abs().amax(dim=(2, 3))
    diff = (long_ - short).abs().amax(dim=(2, 3))
    print(f"T {t} hd {hd}: |long - short| {float(diff.max()):.3e}  short vs fp64 {float(err_short.max()):.3e}")
    assert bool((diff <= err_short).all()), (float(diff.max()), float(err_short.max()))


def test_dispatch_and_reproducibility(_native, monkeypatch):
    names = ("basd_attention_fwd_f32x3", "basd_attention_fwd_f32x3_long")
    calls = []
    for name in names:
        fn = getattr(_native.lib(), name)

        def spy(*args, _fn=fn, _name=name):
            calls.append(_name)
            return _fn(*args)
        monkeypatch.setattr(_native.lib(), name, spy)

    def run(t, h, hd):
        calls.clear()
        qkv = _qkv(2, t, h, hd, t + hd)
        out = _native.attention_fwd_f32x3(qkv, h, hd, hd ** -0.5)
        assert out.shape == (2 * t, 2 * h * hd) and out.dtype == torch.bfloat16
        return qkv, out, list(calls)

    assert run(272, 2, 64)[2] == ["basd_attention_fwd_f32x3"]
    assert run(272, 2, 80)[2] == ["basd_attention_fwd_f32x3"]
    assert run(273, 2, 64)[2] == ["basd_attention_fwd_f32x3_long"]
    for hd in (64, 80):
        qkv, out, seen = run(577, 3, hd)
        assert seen == ["basd_attention_fwd_f32x3_long"]
        again = _native.attention_fwd_f32x3(qkv, 3, hd, hd ** -0.5)
        assert torch.equal(out, again)


def _student(img, patch, **arch):
    from basd_amd.models.vit import create_vit
    torch.manual_seed(0)
    m = create_vit("deit_tiny_patch16_224", num_classes=100, img_size=img, patch_size=patch, **arch)
    with torch.no_grad():                                  # non-trivial biases / LayerNorm affine parameters
        for name, p in m.named_parameters():
            if name.endswith("bias") or "norm" in name:
                p.add_(0.05 * torch.randn_like(p))
    return m.cuda().eval()


def _rel(a, b):
    return float((a.double().cpu() - b.double().cpu()).norm() / b.double().cpu().norm())


# the /14 model is built for 384 px (27 x 27 patches + CLS = 730 tokens); its input is the 378 px the grid covers
_MODELS = [(384, 384, 16, {}, 2, 577), (384, 378, 14, {"embed_dim": 640, "num_heads": 8, "depth": 4}, 1, 730)]


@pytest.mark.parametrize("img,side,patch,arch,batch,tokens", _MODELS)
def test_high_precision_forward_is_strict_and_matches_fp64_at_384(img, side, patch, arch, batch, tokens):
    import basd_amd.losses._ops as O
    from basd_amd.evaluation import matmul_precision
    model = _student(img, patch, **arch)
    assert model.pos_embed.shape[1] == tokens
    x = torch.randn(batch, 3, side, side, device="cuda")
    O.set_strict(True)
    with matmul_precision("high"), torch.no_grad():
        y = model(x)
    O.set_strict(False)
    assert not O.FALLBACKS, dict(O.FALLBACKS)
    ref = copy.deepcopy(model).cpu().double()
    with torch.no_grad():
        want = ref(x.cpu().double())
    rel = _rel(y, want)
    print(f"img {img} patch {patch} T {tokens} {arch}: logits rel-L2 vs fp64 = {rel:.3e}")
    assert rel <= 2e-4, rel


def test_evaluate_model_strict_matches_fp64_at_384():
    """the assertions and constants of test_evaluate_model_strict_matches_fp64, at 577 tokens with a ragged last batch"""
    import basd_amd.losses._ops as O
    from basd_amd.evaluation import evaluate_model, matmul_precision
    model = _student(384, 16)
    g = torch.Generator().manual_seed(3)
    batches = [{"pixel_values": torch.randn(n, 3, 384, 384, generator=g), "label": torch.randint(0, 60, (n,), generator=g)}
               for n in (4, 4, 3)]
    valid = list(range(0, 100, 2)) + [1, 3, 5, 7, 9, 11, 13, 15, 17, 19]
    crit = nn.CrossEntropyLoss()
    O.set_strict(True)
    with matmul_precision("high"):
        got = evaluate_model(model, [{k: v.cuda() for k, v in bt.items()} for bt in batches], crit, num_classes=60,
                             valid_indices=valid)
    O.set_strict(False)
    assert not O.FALLBACKS, dict(O.FALLBACKS)
    ref = copy.deepcopy(model).cpu().double()
    want = evaluate_model(ref, [{"pixel_values": bt["pixel_values"].double(), "label": bt["label"]} for bt in batches],
                          crit, num_classes=60, valid_indices=valid)
    keep = torch.tensor(valid)
    n = 0
    close = 0
    with torch.no_grad():
        for bt in batches:
            lg = ref(bt["pixel_values"].double()).index_select(1, keep)
            top = lg.topk(6, dim=1).values
            close += int(((top[:, 0] - top[:, 1]) < 1e-4).sum() + ((top[:, 4] - top[:, 5]) < 1e-4).sum())
            n += lg.shape[0]
    print(f"384 px evaluate_model: loss {got['loss']:.8f} vs fp64 {want['loss']:.8f} "
          f"(rel {abs(got['loss'] - want['loss']) / abs(want['loss']):.3e}), close decisions {close} of {n}")
    assert abs(got["val_acc"] - want["val_acc"]) * n / 100 <= close + 1e-9
    assert abs(got["val_acc_top5"] - want["val_acc_top5"]) * n / 100 <= close + 1e-9
    assert abs(got["loss"] - want["loss"]) <= 1e-5 * abs(want["loss"])


def test_other_precisions_keep_their_routes_at_384():
    """"highest" stays on the library path and bf16 autocast on the bf16 kernels: the same fallback keys as at 224 px"""
    import basd_amd.losses._ops as O
    from basd_amd.evaluation import matmul_precision
    keys = {}
    for img in (224, 384):
        model = _student(img, 16)
        x = torch.randn(2, 3, img, img, device="cuda")
        O.FALLBACKS.clear()
        with matmul_precision("highest"), torch.no_grad():
            model(x)
        highest = set(O.FALLBACKS)
        O.FALLBACKS.clear()
        with matmul_precision("high"), torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            model(x)
        keys[img] = (highest, set(O.FALLBACKS))
    O.FALLBACKS.clear()
    assert keys[224][0], "the default precision must keep the library fp32 path"
    assert keys[384][0] == keys[224][0], keys
    assert keys[384][1] == keys[224][1] and "attention" not in keys[384][1], keys
