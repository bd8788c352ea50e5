"""The dual-view kernels (csrc/dual_view.hip) against the CPU transforms of data/transforms.py, stage by stage.

Tolerance "one level": a pixel may differ from the CPU oracle by one uint8 level (1 / (255 std_c) in normalised units),
at most 1 % of a case's pixels may, none by more.  The 1 % is a cap, not a measurement: tests/test_device_views_cases_cpu.py
holds the CPU-side figures of the chosen cases (fp64 restatement of the colour ops: at most 0.55 %; affine pixels left
out near a rounding boundary: at most 0.40 %).  Exact equality where the arithmetic is integer: Identity, Posterize,
Solarize, Equalize, TranslateX / Y and windows of the output's size.  A case of the TrivialAugment kernel is one
(op, magnitude) on the four input images; a case of the resample kernel is one window of one image."""
import os

import numpy as np
import pytest
import torch

from tests import _dual_view_cases as C

pytestmark = pytest.mark.gpu

CFG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                   "vit-bias-aware-structural-distillation_amd", "configs", "config.yaml")


def _check_one_level(got_u8, want_u8, what, exact=False):
    worst, share = C.one_level_report(got_u8.cpu(), want_u8)
    print(f"{what}: max {worst}, share {100 * share:.4f} %")
    if exact:
        assert worst == 0, (what, worst, share)
    assert worst <= 1 and share <= C.ONE_LEVEL_CAP, (what, worst, share)


# ----------------------------------------------------------------------------------------------------- basd_resample_u8
@pytest.mark.parametrize("hw", [(40, 56), (64, 48), (16, 200)])
@pytest.mark.parametrize("s", [32, 31])
def test_resample_windows_against_resize_crop_and_flip(hw, s):
    import basd_amd._native as native
    h, w = hw
    windows = C.resample_windows(h, w, s)
    assert len(windows) <= 16
    sources = [C.random_image(h, w, 7) if i % 2 == 0 else C.smooth_image(h, w, 0.3 * i) for i in range(len(windows))]
    flips = [i % 3 == 1 for i in range(len(windows))]
    assert any(flips) and not all(flips)
    got = native.resample_u8(torch.stack(sources).cuda(), C.augment_records(windows, flips, s).cuda(), s)
    assert got.dtype == torch.uint8 and got.shape == (len(windows), 3, s, s)
    for i, (img, win, fl) in enumerate(zip(sources, windows, flips)):
        want = C.resample_oracle(img, win, s, fl)
        _check_one_level(got[i], want, f"{h}x{w} -> {s} window {win} flip {fl}", exact=win[2:] == (s, s))
    if hw == (16, 200):
        assert any(win[3] / s > 2 for win in windows)          # a horizontal filter of more than four taps


@pytest.mark.parametrize("hw,ratio", [((40, 56), 0.8), ((64, 48), 0.8), ((40, 56), 32 / 52), ((64, 48), 32 / 52),
                                      ((16, 200), 32 / 52)])
def test_clean_view_against_resize_and_center_crop(hw, ratio):
    """resized sizes 40 (the shorter side of 40 x 56 as it is: a pure crop, exact) and 52"""
    from basd_amd.data import transforms as T
    from basd_amd.data.device_views import _CleanView
    view = _CleanView(32, C.MEAN, C.STD, ratio)
    images = torch.stack([C.random_image(*hw, 5), C.smooth_image(*hw), C.random_image(*hw, 6)])
    got = view.uint8(images.cuda())
    want = view.uint8(images)
    for i in range(3):
        assert torch.equal(want[i], T.center_crop(T.resize(images[i], view.resize_size), 32))
        _check_one_level(got[i], want[i], f"clean {hw} resize {view.resize_size} image {i}",
                         exact=view.resize_size == min(hw))
    got_f = view.normalized(images.cuda())
    torch.testing.assert_close(got_f.cpu(), C.normalized(got.cpu(), C.MEAN, C.STD), atol=1e-6, rtol=1e-6)


def test_resample_256_to_224():
    import basd_amd._native as native
    sources = [C.random_image(256, 256, 9), C.smooth_image(256, 256)]
    windows, flips = [(0, 0, 256, 256), (17, 40, 160, 120)], [True, False]
    got = native.resample_u8(torch.stack(sources).cuda(), C.augment_records(windows, flips, 224).cuda(), 224)
    for i in range(2):
        _check_one_level(got[i], C.resample_oracle(sources[i], windows[i], 224, flips[i]), f"256 -> 224 window {windows[i]}")


def test_resample_clamps_a_bad_record_into_the_image():
    """a window reaching outside the canvas is cut to it (no out-of-bounds read): the result is that of the cut window"""
    import basd_amd._native as native
    img = C.random_image(40, 56, 4)
    rec = torch.tensor([[30, 50, 40, 56, 32, 32, 0, 0, 0]], dtype=torch.int32)
    got = native.resample_u8(img[None].cuda(), rec.cuda(), 32)
    _check_one_level(got[0], C.resample_oracle(img, (30, 50, 10, 6), 32, False), "cut window")


# ------------------------------------------------------------------------------------------------- basd_ta_normalize_u8
def _run_ta(s, keep_ops=None):
    import basd_amd._native as native
    from basd_amd.data import transforms as T
    imgs = C.ta_inputs(s)
    cases = [(o, m) for o, m in C.ta_cases() if keep_ops is None or T.TA_WIDE_OPS[o] in keep_ops]
    batch = imgs.repeat(len(cases), 1, 1, 1)
    ops = torch.tensor([o for o, _ in cases], dtype=torch.int32).repeat_interleave(len(imgs))
    mags = torch.tensor([m for _, m in cases], dtype=torch.float64).repeat_interleave(len(imgs))
    got = native.ta_normalize_u8(batch.cuda(), ops.cuda(), mags.cuda(), C.MEAN, C.STD)
    assert got.dtype == torch.float32 and got.shape == (len(cases) * len(imgs), 3, s, s)
    got = got.cpu().view(len(cases), len(imgs), 3, s, s)
    for k, (op_id, mag) in enumerate(cases):
        op = T.TA_WIDE_OPS[op_id]
        want = torch.stack([C.ta_oracle(img, op_id, mag) for img in imgs])
        lev = C.levels(got[k])
        # the normalisation itself: the fp32 value of the level the kernel chose
        torch.testing.assert_close(got[k], C.normalized(lev.to(torch.uint8)), atol=1e-6, rtol=1e-6)
        what = f"S={s} {op} {mag:+.3f}"
        if op in C.EXACT_OPS:
            torch.testing.assert_close(got[k], C.normalized(want), atol=1e-6, rtol=1e-6)
            assert torch.equal(lev, want.long()), what
        elif op in C.AFFINE_OPS:
            near = C.affine_boundary_mask(s, op, mag)
            assert float(near.double().mean()) < 0.01
            worst, share = C.one_level_report(lev, want, keep=~near)
            print(f"{what}: {int(near.sum())} pixels left out, max {worst}, share {100 * share:.4f} %")
            assert worst == 0, what
        else:
            _check_one_level(lev, want, what)


def test_every_trivial_augment_op_at_32():
    _run_ta(32)


def test_reductions_and_rotation_at_224():
    _run_ta(224, keep_ops=("Equalize", "AutoContrast", "Contrast", "Sharpness", "Rotate"))


def test_identity_without_ops_and_odd_size():
    """ops = NULL is the clean view; S = 31 leaves images off the 16-byte grid (scalar head and tail of the stores)"""
    import basd_amd._native as native
    imgs = torch.stack([C.random_image(31, 31, i) for i in range(5)])
    got = native.ta_normalize_u8(imgs.cuda(), None, None, C.MEAN, C.STD)
    torch.testing.assert_close(got.cpu(), C.normalized(imgs), atol=1e-6, rtol=1e-6)
    ops = torch.tensor([13, 9, 5, 12, 8], dtype=torch.int32)
    mags = torch.tensor([0.0, 0.99, 67.5, 0.0, -0.495], dtype=torch.float64)
    got = native.ta_normalize_u8(imgs.cuda(), ops.cuda(), mags.cuda(), C.MEAN, C.STD).cpu()
    from basd_amd.data import transforms as T
    for i in range(5):
        op = T.TA_WIDE_OPS[int(ops[i])]
        keep = ~C.affine_boundary_mask(31, op, float(mags[i])) if op in C.AFFINE_OPS else None
        worst, share = C.one_level_report(C.levels(got[i]), C.ta_oracle(imgs[i], int(ops[i]), float(mags[i])), keep=keep)
        assert worst <= (0 if op in C.EXACT_OPS + C.AFFINE_OPS else 1) and share <= C.ONE_LEVEL_CAP, (op, worst, share)


# -------------------------------------------------------------------------------------------------------- end to end
def test_device_dual_view_against_its_cpu_fallback():
    from basd_amd.data import DeviceDualView
    views = DeviceDualView(32, (0.41, 0.52, 0.47), (0.21, 0.26, 0.24), C.MEAN, C.STD, crop_ratio=32 / 52)
    b = 8
    images = torch.stack([C.random_image(40, 56, i) if i % 2 else C.smooth_image(40, 56, 0.2 * i) for i in range(b)])
    vp = torch.stack([views.draw(40, 56, torch.Generator().manual_seed(100 + i)) for i in range(b)])
    label = torch.arange(b, dtype=torch.int64)
    for op_id in (0, 6):                                             # Identity, Brightness: a one-level difference of
        vp[:, 5] = op_id                                             # the resample stays one level under them
        if op_id == 0:
            vp[:, 6] = 0.0
        else:
            # factors below 1: a one-level difference of the resample is at most one level behind the blend
            vp[:, 6] = torch.tensor([-0.33 if i % 2 else -0.66 for i in range(b)], dtype=torch.float64)
        batch = {"image": images, "view_params": vp, "label": label}
        want = views(batch)
        got = views({k: v.cuda() for k, v in batch.items()})
        assert sorted(got) == ["augmented", "clean", "label"]
        for k in ("clean", "augmented"):
            assert got[k].dtype == torch.float32 and got[k].shape == (b, 3, 32, 32) and got[k].is_cuda
        assert got["label"].is_cuda and torch.equal(got["label"].cpu(), label)
        for i in range(b):
            _check_one_level(C.levels(got["clean"][i].cpu()), C.levels(want["clean"][i]), f"clean view {i}")
            _check_one_level(C.levels(got["augmented"][i].cpu(), views.mean, views.std),
                             C.levels(want["augmented"][i], views.mean, views.std), f"augmented view {i} op {op_id}")
        u8c, u8a = views.resample({k: v.cuda() for k, v in batch.items()})
        assert u8c.dtype == u8a.dtype == torch.uint8 and u8c.shape == u8a.shape == (b, 3, 32, 32)
        torch.testing.assert_close(got["clean"].cpu(), C.normalized(u8c.cpu()), atol=1e-6, rtol=1e-6)


def test_captured_train_step_fed_by_a_device_view_loader(tmp_path):
    """Trainer._train_epoch on a two-batch .npz loader with device_views: the step is captured, the loss finite and the
    kernels' fallback ledger as empty as after the same epoch from the classic loader"""
    from basd_amd.config import load_config
    from basd_amd.data import create_dataloaders
    from basd_amd.evaluation import evaluate_model
    from basd_amd.losses import _ops as O
    from basd_amd.train import build
    rng = np.random.default_rng(0)
    root = tmp_path / "toy"
    root.mkdir()
    for split, n in (("train", 16), ("validation", 8)):
        imgs = rng.integers(0, 256, size=(n, 40, 48, 3), dtype=np.uint8)
        np.savez(root / f"{split}.npz", images=imgs, labels=np.arange(n) % 4)
    cfg = load_config(CFG, "basd_cifar100", [f"data.dataset={root}", "data.batch_size=8", "model.drop_path_rate=0.0"])
    ledgers, losses = {}, {}
    for device_views in (False, True):
        trainer, _ = build(cfg, device="cuda")
        train, val = create_dataloaders(cfg, teacher_stats=(trainer._teacher.mean, trainer._teacher.std), num_workers=0,
                                        device_views=device_views)
        assert len(train) == 2 and hasattr(train, "device_views") == device_views
        trainer.optimizer.train()
        trainer.model.train()
        O.FALLBACKS.clear()
        metrics = trainer._train_epoch(train)
        ledgers[device_views] = dict(O.FALLBACKS)
        assert trainer._graph is not None, trainer.graph_error
        assert np.isfinite(metrics["train_loss"]) and trainer.optimizer.k == 2
        losses[device_views] = metrics["train_loss"]
        trainer.optimizer.eval()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            res = evaluate_model(trainer.model, val, torch.nn.CrossEntropyLoss(), num_classes=4)
        assert np.isfinite(res["loss"]) and 0.0 <= res["val_acc"] <= 100.0
    assert ledgers[True] == ledgers[False], ledgers
    print("train loss classic / device views:", losses[False], losses[True])
