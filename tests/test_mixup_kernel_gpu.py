"""basd_mixup_cutmix (csrc/mixup.hip) through the binding against the torch chain of training/mixup.py on the same device
tensors and the same host parameters: MixUp blend, CutMix paste, soft targets, error paths, the dispatch of
``mixup_cutmix`` and one captured train step per mode.

Bounds.  CutMix moves bits: ``torch.equal``.  MixUp evaluates the same two-operation fp32 formula on both sides, which
can differ only by the contraction of the product into an FMA (one rounding of w (b - a), at most 2^-24 * 2 max(|a|, |b|),
plus the final rounding landing one ulp apart): |got - ref| <= 2^-22 max(|a|, |b|) for fp32 images, one bf16 ulp for bf16
images, and exact where lam is 0 or 1.  Targets: the products are by 0 or +-1, hence exact: 2^-23 against the chain, a row
sum within 2^-22 of 1, exactly one-hot where both labels agree."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BATCHES = (1, 2, 3, 8)
SHAPES = ((3, 5, 7), (3, 32, 32), (3, 30, 34), (1, 8, 8))
CLASSES = (1, 5, 100, 1000)
DTYPES = (torch.float32, torch.bfloat16)
LAMS = (0.0, 1.0, 0.25, 0.5, 0.75, 5e-4)


def _native():
    import basd_amd._native as native
    return native


def _chain(x, y, k, mode, lam, box):
    from basd_amd.training.mixup import _torch_chain
    return _torch_chain(x, y, k, mode, lam, box)


def _inputs(b, shape, dtype, k, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + 10 * b + shape[1])
    x = torch.randn(b, *shape, generator=g).to(dtype).cuda()
    y = torch.randint(0, k, (b,), generator=g)
    if b >= 3:
        y[1] = y[0]                                   # one pair with equal labels, whatever the class count
    return x, y.cuda()


def _run(x, y, k, mode, lam, box):
    out = torch.full_like(x, float("nan"))
    tgt = torch.full((x.shape[0], k), float("nan"), device=x.device)
    got = _native().mixup_cutmix(x, y, k, mode, lam, box, out, tgt)
    assert got[0] is out and got[1] is tgt
    return out, tgt


def _boxes(h, w):
    return {
        "empty": (0, 0, 0, 0),
        "empty_rows": (2, 2, 1, w - 1),
        "empty_cols": (1, h - 1, 3, 3),
        "whole": (0, h, 0, w),
        "pixel": (h // 2, h // 2 + 1, w // 2, w // 2 + 1),
        "top": (0, h // 2, 1, w - 1),
        "bottom": (h // 2, h, 1, w - 1),
        "left": (1, h - 1, 0, w // 2),
        "right": (1, h - 1, w // 2, w),
        "odd_x0": (1, h - 1, 1, 4),                   # x0 odd, three columns wide
        "last_pixel": (h - 1, h, w - 1, w),
    }


def _check_targets(tgt, y, k, lam, ref):
    assert not bool(torch.isnan(tgt).any()), "an element of out_targets was not written"
    sums = tgt.double().sum(1)
    assert float((sums - 1.0).abs().max()) <= 2.0 ** -22, sums
    same = y == y.roll(1, 0)
    onehot = torch.nn.functional.one_hot(y, k).float()
    assert torch.equal(tgt[same], onehot[same])
    assert float((tgt - ref).abs().max()) <= 2.0 ** -23


def _check_mixup(out, x, lam, ref):
    a, b = x.roll(1, 0), x
    assert not bool(torch.isnan(out).any()), "an element of out_images was not written"
    if lam == 0.0:
        assert torch.equal(out, a)
    elif lam == 1.0:
        assert torch.equal(out, b)
    if x.dtype == torch.float32:
        bound = 2.0 ** -22 * torch.maximum(a.abs(), b.abs())
    else:                                             # one ulp of the larger of the two bf16 values
        big = torch.maximum(out.float().abs(), ref.float().abs())
        bound = torch.ldexp(torch.ones_like(big), torch.frexp(big).exponent - 8)
    err = (out.float() - ref.float()).abs()
    print(f"mixup {tuple(x.shape)} {x.dtype} lam {lam}: bitwise {bool(torch.equal(out, ref))}, "
          f"max err / bound {float((err / bound.clamp_min(1e-45)).max()):.3f}")
    assert bool((err <= bound).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16"))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("b", BATCHES)
def test_cutmix_pastes_the_partner_box_bit_for_bit(b, shape, dtype):
    h, w = shape[1:]
    for n, (name, box) in enumerate(_boxes(h, w).items()):
        k = CLASSES[(n + b) % 4]
        x, y = _inputs(b, shape, dtype, k, seed=n)
        lam = 1.0 - (box[1] - box[0]) * (box[3] - box[2]) / float(h * w)
        out, tgt = _run(x, y, k, 1, lam, box)
        ref, ref_t = _chain(x, y, k, 1, lam, box)
        assert torch.equal(out.view(torch.int32 if dtype == torch.float32 else torch.int16),
                           ref.view(torch.int32 if dtype == torch.float32 else torch.int16)), name
        _check_targets(tgt, y, k, lam, ref_t)


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16"))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("b", BATCHES)
def test_mixup_blends_with_the_partner(b, shape, dtype):
    for n, lam in enumerate(LAMS):
        k = CLASSES[(n + b) % 4]
        x, y = _inputs(b, shape, dtype, k, seed=n)
        out, tgt = _run(x, y, k, 0, lam, (0, 0, 0, 0))
        ref, ref_t = _chain(x, y, k, 0, lam, None)
        _check_mixup(out, x, lam, ref)
        _check_targets(tgt, y, k, lam, ref_t)


@pytest.mark.parametrize("k", CLASSES)
@pytest.mark.parametrize("b", BATCHES)
def test_soft_targets_for_every_batch_and_class_count(b, k):
    for mode in (0, 1):
        for n, lam in enumerate(LAMS):
            x, y = _inputs(b, (1, 8, 8), torch.float32, k, seed=n)
            out, tgt = _run(x, y, k, mode, lam, (0, 8, 0, 8) if mode else (0, 0, 0, 0))
            _, ref_t = _chain(x, y, k, mode, lam, (0, 8, 0, 8))
            _check_targets(tgt, y, k, lam, ref_t)
            if lam == 1.0:
                assert torch.equal(tgt, torch.nn.functional.one_hot(y, k).float())
            if lam == 0.0:
                assert torch.equal(tgt, torch.nn.functional.one_hot(y.roll(1, 0), k).float())


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16"))
def test_pointers_off_the_16_byte_grid_take_element_accesses(dtype):
    """samples of 105 elements: every sample but the first of a larger buffer starts off the 16-byte grid"""
    k = 5
    store, y_all = _inputs(4, (3, 5, 7), dtype, k)
    x, y = store[1:], y_all[1:].contiguous()
    assert x.is_contiguous() and x.data_ptr() % 16 != 0
    out_store = torch.full_like(store, float("nan"))
    tgt_store = torch.full((4, k), float("nan"), device="cuda")
    for mode, lam, box in ((0, 0.25, (0, 0, 0, 0)), (0, 0.75, (0, 0, 0, 0)), (1, 1.0 - 6 / 35.0, (1, 4, 2, 4))):
        out_store.fill_(float("nan"))
        tgt_store.fill_(float("nan"))
        _native().mixup_cutmix(x, y, k, mode, lam, box, out_store[1:], tgt_store[1:])
        ref, ref_t = _chain(x, y, k, mode, lam, box)
        assert bool(torch.isnan(out_store[0]).all()) and bool(torch.isnan(tgt_store[0]).all())    # nothing in front
        if mode:
            assert torch.equal(out_store[1:], ref)
        else:
            _check_mixup(out_store[1:], x, lam, ref)
        _check_targets(tgt_store[1:], y, k, lam, ref_t)


def test_a_label_outside_the_classes_matches_no_column():
    k = 5
    x, _ = _inputs(3, (1, 8, 8), torch.float32, k)
    y = torch.tensor([2, k, -1], device="cuda")
    guard = torch.full((5, k), float("nan"), device="cuda")
    out = torch.empty_like(x)
    _native().mixup_cutmix(x, y, k, 0, 0.25, (0, 0, 0, 0), out, guard[1:4])
    assert bool(torch.isnan(guard[0]).all()) and bool(torch.isnan(guard[4]).all())
    want = torch.zeros(3, k)
    want[0, 2] = 0.25                                 # own label 2, partner -1
    want[1, 2] = 0.75                                 # own label out of range, partner 2
    assert torch.equal(guard[1:4].cpu(), want)


def test_error_paths_fail_on_the_host():
    native = _native()
    x, y = _inputs(3, (3, 32, 32), torch.float32, 5)
    tgt = torch.empty(3, 5, device="cuda")
    with pytest.raises(native.BasdNativeError, match="status 1"):
        native.mixup_cutmix(x, y, 5, 0, 0.5, (0, 0, 0, 0), x, tgt)                    # out is the input
    store = torch.zeros(4, 3, 32, 32, device="cuda")
    for src, dst in ((store[:3], store[1:]), (store[1:], store[:3])):                 # overlapping ranges
        with pytest.raises(native.BasdNativeError, match="status 1"):
            native.mixup_cutmix(src, y, 5, 1, 0.5, (0, 8, 0, 8), dst, tgt)
    out = torch.empty_like(x)
    for box in ((0, 33, 0, 8), (0, 8, 0, 33), (-1, 8, 0, 8), (0, 8, -1, 8), (9, 8, 0, 8), (0, 8, 9, 8)):
        with pytest.raises(native.BasdNativeError, match="status 1"):
            native.mixup_cutmix(x, y, 5, 1, 0.5, box, out, tgt)
    with pytest.raises(native.BasdNativeError, match="status 1"):
        native.mixup_cutmix(x, y, 5, 2, 0.5, (0, 0, 0, 0), out, tgt)
    torch.cuda.synchronize()
    assert not native.mixup_supported(x.cpu()) and not native.mixup_supported(x.double())
    assert not native.mixup_supported(x[:, :, :, ::2]) and not native.mixup_supported(x[0])
    assert native.mixup_supported(x) and native.mixup_supported(x.bfloat16())


def _spy(monkeypatch):
    native = _native()
    calls = []
    real = native.mixup_cutmix

    def spy(images, labels, num_classes, mode, lam, box, out, out_targets):
        calls.append((mode, lam, tuple(box)))
        return real(images, labels, num_classes, mode, lam, box, out, out_targets)

    monkeypatch.setattr(native, "mixup_cutmix", spy)
    return calls


def test_dispatch_sends_device_batches_to_the_kernel_once(monkeypatch):
    from basd_amd.training import mixup as M
    native = _native()
    x, y = _inputs(8, (3, 30, 34), torch.float32, 100)
    seen = set()
    for seed in range(16):
        calls = _spy(monkeypatch)
        torch.manual_seed(seed)
        out, tgt = M.mixup_cutmix(x, y, 100, generator=torch.Generator().manual_seed(seed),
                                  out=torch.full_like(x, float("nan")), out_targets=torch.full((8, 100), float("nan"), device="cuda"))
        monkeypatch.undo()
        assert len(calls) == 1
        mode, lam, box = calls[0]
        with monkeypatch.context() as m:                       # the torch chain forced, same seeds
            m.setattr(native, "mixup_supported", lambda images: False)
            m.setattr(native, "mixup_cutmix", None)
            torch.manual_seed(seed)
            ref, ref_t = M.mixup_cutmix(x, y, 100, generator=torch.Generator().manual_seed(seed))
        if mode == M.CUTMIX:
            assert torch.equal(out, ref)
        else:
            _check_mixup(out, x, lam, ref)
        _check_targets(tgt, y, 100, lam, ref_t)
        seen.add(mode)
    assert seen == {M.MIXUP, M.CUTMIX}


def test_dispatch_keeps_the_torch_chain_for_other_layouts(monkeypatch):
    from basd_amd.training import mixup as M
    calls = _spy(monkeypatch)
    x, y = _inputs(8, (3, 32, 32), torch.float32, 10)
    for strided in (x.to(memory_format=torch.channels_last), x.double(), x.half()):
        assert not strided.is_contiguous() or strided.dtype != torch.float32
        for seed in range(4):
            torch.manual_seed(seed)
            out, tgt = M.mixup_cutmix(strided, y, 10, generator=torch.Generator().manual_seed(seed))
            torch.manual_seed(seed)
            mode, lam, box = M._draw(32, 32, torch.Generator().manual_seed(seed))
            ref, ref_t = _chain(strided.contiguous(), y, 10, mode, lam, box)
            assert torch.equal(out.contiguous(), ref) and torch.equal(tgt, ref_t)
    assert calls == []


def _trainer(batch):
    import os
    from basd_amd.config import load_config
    from basd_amd.train import SyntheticLoader, build
    cfg_path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                            "vit-bias-aware-structural-distillation_amd", "configs", "config.yaml")
    torch.manual_seed(0)
    cfg = load_config(cfg_path, "basd_cifar100", [f"data.batch_size={batch}", "model.drop_path_rate=0.0"])
    trainer, _ = build(cfg, device="cuda")
    assert trainer.use_mixup
    trainer.optimizer.train()
    trainer.model.train()
    return trainer, next(iter(SyntheticLoader(batch, 32, 100, 1, "cuda", seed=5)))


def _seed_for(mode):
    from basd_amd.training.mixup import _draw
    for seed in range(64):
        torch.manual_seed(seed)
        if _draw(32, 32)[0] == mode:
            return seed
    raise AssertionError(mode)


@pytest.mark.parametrize("mode", (1, 0), ids=("cutmix", "mixup"))
def test_captured_step_with_the_kernel_equals_the_step_with_the_torch_chain(mode, monkeypatch):
    """First step of two trainers built from one seed, the captured step fed by the kernel and by the torch chain.  The
    step's inputs are compared under the bounds of this module (bitwise for CutMix); the loss of a step on identical
    weights and inputs is reproducible up to the arrival order of the kernels' atomics, 1e-5 relative, the bound
    tests/test_train_step_gpu.py holds a replayed step to, and a MixUp batch that differs by the contraction of one
    product (2^-22 relative per pixel, far below the bf16 activations' 2^-9) moves it by less than that."""
    native = _native()
    seed = _seed_for(mode)
    results = []
    for use_kernel in (True, False):
        trainer, batch = _trainer(32)
        assert trainer.enable_graph(batch), trainer.graph_error
        calls = _spy(monkeypatch)
        if not use_kernel:
            monkeypatch.setattr(native, "mixup_supported", lambda images: False)
        torch.manual_seed(seed)
        loss, _ = trainer.train_step(batch)
        torch.cuda.synchronize()
        monkeypatch.undo()
        assert len(calls) == (1 if use_kernel else 0)
        if use_kernel:
            assert calls[0][0] == mode
        trainer.check_health()
        results.append((float(loss), trainer._g_imgs.clone(), trainer._g_targets.clone()))
    (loss_k, imgs_k, tgt_k), (loss_c, imgs_c, tgt_c) = results
    print(f"mode {mode}: loss {loss_k!r} (kernel) vs {loss_c!r} (torch chain), bitwise {loss_k == loss_c}")
    if mode == 1:
        assert torch.equal(imgs_k, imgs_c) and torch.equal(tgt_k, tgt_c)
    else:
        aug = batch["augmented"]
        bound = 2.0 ** -22 * torch.maximum(aug.abs(), aug.roll(1, 0).abs())
        assert bool(((imgs_k - imgs_c).abs() <= bound).all())
        assert float((tgt_k - tgt_c).abs().max()) <= 2.0 ** -23
    assert loss_k == loss_k and abs(loss_k - loss_c) <= 1e-5 * abs(loss_c), (loss_k, loss_c)
