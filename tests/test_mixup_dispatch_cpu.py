"""training/mixup.py without a device: CPU tensors never reach the binding, the host draws are those of the torch-only
version for a fixed seed, and a plain torch restatement of basd_mixup_cutmix's contract (include/basd_hip.h) equals the
torch chain on the shapes the GPU test runs."""
import pytest
import torch

BATCHES = (1, 2, 3, 8)
SHAPES = ((3, 5, 7), (3, 32, 32), (3, 30, 34), (1, 8, 8))
CLASSES = (1, 5, 100, 1000)
LAMS = (0.0, 1.0, 0.25, 0.5, 0.75, 5e-4)


def _lerp(a, b, lam):
    """at::native::lerp with a scalar weight, in fp32, one operation at a time"""
    w = torch.tensor(lam, dtype=torch.float32)
    d = b - a
    return torch.where(w.abs() < 0.5, a + w * d, b - d * (1.0 - w))


def emulate(x, y, k, mode, lam, box):
    """the contract of basd_mixup_cutmix: partner (i - 1) mod B, fp32 blend rounded once, bit copies inside the box,
    every target written, a label outside [0, k) matching no column"""
    prev = x.roll(1, 0)
    if mode == 0:
        out = _lerp(prev.float(), x.float(), lam).to(x.dtype)
    else:
        y0, y1, x0, x1 = box
        inside = torch.zeros(x.shape[-2:], dtype=torch.bool)
        inside[y0:y1, x0:x1] = True
        out = torch.where(inside, prev, x)
    cols = torch.arange(k)
    own, partner = (y[:, None] == cols).float(), (y.roll(1, 0)[:, None] == cols).float()
    return out, _lerp(partner, own, lam)


def _parent_draws(h, w, generator=None):
    """the draws of the torch-only mixup_cutmix, in its order"""
    lam = float(torch.distributions.Beta(1.0, 1.0).sample())
    if float(torch.rand((), generator=generator)) < 0.5:
        return 0, lam, None
    r = (1.0 - lam) ** 0.5
    ch, cw = int(h * r), int(w * r)
    cy = int(torch.randint(h, (1,), generator=generator))
    cx = int(torch.randint(w, (1,), generator=generator))
    y0, y1 = max(cy - ch // 2, 0), min(cy + ch // 2, h)
    x0, x1 = max(cx - cw // 2, 0), min(cx + cw // 2, w)
    return 1, 1.0 - (y1 - y0) * (x1 - x0) / float(h * w), (y0, y1, x0, x1)


def _inputs(b, shape, dtype, k, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + 10 * b + shape[1])
    x = torch.randn(b, *shape, generator=g).to(dtype)
    y = torch.randint(0, k, (b,), generator=g)
    if b >= 3:
        y[1] = y[0]
    return x, y


def _check(got, ref, x, mode, lam):
    (out, tgt), (ref_out, ref_t) = got, ref
    if mode == 1 or lam in (0.0, 1.0):
        assert torch.equal(out, ref_out)
    elif x.dtype == torch.float32:              # the CPU's lerp may contract the product into an FMA
        bound = 2.0 ** -22 * torch.maximum(x.abs(), x.roll(1, 0).abs())
        assert bool(((out - ref_out).abs() <= bound).all())
    else:
        big = torch.maximum(out.float().abs(), ref_out.float().abs())
        ulp = torch.ldexp(torch.ones_like(big), torch.frexp(big).exponent - 8)
        assert bool(((out.float() - ref_out.float()).abs() <= ulp).all())
    assert float((tgt - ref_t).abs().max()) <= 2.0 ** -23
    assert float((tgt.double().sum(1) - 1.0).abs().max()) <= 2.0 ** -22


def test_cpu_tensors_never_reach_the_binding(monkeypatch):
    import basd_amd._native as native
    from basd_amd.training import mixup as M

    def refuse(*args, **kwargs):
        raise AssertionError("the binding was reached with CPU tensors")

    monkeypatch.setattr(native, "mixup_cutmix", refuse)
    monkeypatch.setattr(native, "lib", refuse)
    x, y = _inputs(8, (3, 32, 32), torch.float32, 10)
    assert not native.mixup_supported(x)
    for dtype in (torch.float32, torch.bfloat16, torch.float64):
        for seed in range(6):
            torch.manual_seed(seed)
            out, tgt = M.mixup_cutmix(x.to(dtype), y, 10, generator=torch.Generator().manual_seed(seed))
            assert out.shape == x.shape and out.dtype == dtype and tgt.shape == (8, 10)
            torch.testing.assert_close(tgt.sum(1), torch.ones(8))


def test_host_draws_are_unchanged_and_reach_the_kernel_path_as_drawn(monkeypatch):
    """ten calls on one generator: what the kernel path would be handed (the binding replaced by the restatement above)
    is what the torch-only version drew from the same seeds, and the results equal the torch chain's"""
    import basd_amd._native as native
    from basd_amd.training import mixup as M
    x, y = _inputs(8, (3, 30, 34), torch.float32, 100)
    torch.manual_seed(7)
    gen = torch.Generator().manual_seed(11)
    want = [_parent_draws(30, 34, gen) for _ in range(10)]
    assert {d[0] for d in want} == {0, 1}

    received = []

    def fake(images, labels, num_classes, mode, lam, box, out, out_targets):
        received.append((mode, lam, tuple(box)))
        res, res_t = emulate(images, labels, num_classes, mode, lam, box)
        out.copy_(res)
        out_targets.copy_(res_t)
        return out, out_targets

    monkeypatch.setattr(M, "_kernel_takes", lambda *args: True)
    monkeypatch.setattr(native, "mixup_cutmix", fake)
    torch.manual_seed(7)
    gen = torch.Generator().manual_seed(11)
    got = [M.mixup_cutmix(x, y, 100, generator=gen) for _ in range(10)]
    monkeypatch.undo()
    assert len(received) == 10
    for (mode, lam, box), (r_mode, r_lam, r_box) in zip(want, received):
        assert (mode, lam) == (r_mode, r_lam) and r_box == (box or (0, 0, 0, 0))

    torch.manual_seed(7)
    gen = torch.Generator().manual_seed(11)
    for (mode, lam, box), g in zip(want, got):                  # the torch path, same seeds
        ref = M.mixup_cutmix(x, y, 100, generator=gen)
        _check(g, ref, x, mode, lam)
        assert M.MIXUP == 0 and M.CUTMIX == 1


@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16), ids=("fp32", "bf16"))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_restated_contract_equals_the_torch_chain(shape, dtype):
    from basd_amd.training.mixup import _torch_chain
    h, w = shape[1:]
    boxes = ((0, 0, 0, 0), (0, h, 0, w), (h // 2, h // 2 + 1, w // 2, w // 2 + 1), (0, h // 2, 1, w - 1),
             (h // 2, h, 1, w - 1), (1, h - 1, 0, w // 2), (1, h - 1, w // 2, w), (1, h - 1, 1, 4))
    for b in BATCHES:
        for n, k in enumerate(CLASSES):
            x, y = _inputs(b, shape, dtype, k, seed=n)
            for lam in LAMS:
                _check(emulate(x, y, k, 0, lam, None), _torch_chain(x, y, k, 0, lam, None), x, 0, lam)
            for box in boxes[n::2] if b != 3 else boxes:
                lam = 1.0 - (box[1] - box[0]) * (box[3] - box[2]) / float(h * w)
                _check(emulate(x, y, k, 1, lam, box), _torch_chain(x, y, k, 1, lam, box), x, 1, lam)
