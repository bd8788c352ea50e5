"""Device views from images of different sizes, the host half (``device_views="packed"``): the packing collate
function followed by the CPU fallback of ``DeviceDualView`` / ``DeviceEvalView`` gives the classic loader's batches bit
for bit on a directory split, ``pack_images`` and the host-side record builders do what they say, and ``True`` /
``False`` keep their meaning."""
import os

import numpy as np
import pytest
import torch

from tests import _dual_view_cases as C

STATS = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
SIZES = ((40, 56), (64, 48), (33, 71), (50, 50))


def _cfg(root, *extra):
    from basd_amd.config import load_config
    cfg_path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                            "vit-bias-aware-structural-distillation_amd", "configs", "config.yaml")
    return load_config(cfg_path, None, [f"data.dataset={root}", "data.batch_size=4", "model.vit.img_size=32",
                                        "model.vit.patch_size=4", *extra])


def _directory_root(tmp_path, n_train=5, n_val=3):
    """root/<split>/<class>/*.png with a different size from file to file (PNG: lossless)"""
    from PIL import Image
    rng = np.random.default_rng(2)
    k = 0
    for split, n in (("train", n_train), ("validation", n_val)):
        for c in ("ant", "bee", "cat"):
            d = tmp_path / "folders" / split / c
            d.mkdir(parents=True)
            for i in range(n):
                h, w = SIZES[k % len(SIZES)]
                k += 1
                Image.fromarray(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)).save(d / f"{i}.png")
    return str(tmp_path / "folders")


def _npz_root(tmp_path, hw=(40, 56)):
    rng = np.random.default_rng(0)
    root = tmp_path / "toyset"
    root.mkdir()
    for split, n in (("train", 12), ("validation", 6)):
        imgs = rng.integers(0, 256, size=(n, hw[0], hw[1], 3), dtype=np.uint8)
        np.savez(root / f"{split}.npz", images=imgs, labels=np.arange(n) % 3)
    return str(root)


def test_directory_root_equals_the_classic_loader(tmp_path):
    from basd_amd.data import DeviceDualView, create_dataloaders
    from basd_amd.data.device_views import DeviceEvalView
    cfg = _cfg(_directory_root(tmp_path))
    classic, classic_val = create_dataloaders(cfg, teacher_stats=STATS, num_workers=0)
    packed, packed_val = create_dataloaders(cfg, teacher_stats=STATS, num_workers=0, device_views="packed")
    assert isinstance(packed.device_views, DeviceDualView) and isinstance(packed_val.device_views, DeviceEvalView)
    seen_sizes = set()
    for epoch in (0, 1):
        classic.dataset.set_epoch(epoch)
        packed.dataset.set_epoch(epoch)
        want, raw = list(classic), list(packed)
        assert len(raw) == len(want) == 3
        for b, w in zip(raw, want):
            assert sorted(b) == ["aug_rec", "clean_rec", "geometry", "label", "pixels", "view_params"]
            assert b["pixels"].dtype == torch.uint8 and b["pixels"].dim() == 1
            assert b["geometry"].dtype == torch.int64 and b["geometry"].shape == (4, 3)
            assert b["clean_rec"].dtype == b["aug_rec"].dtype == torch.int32
            assert b["clean_rec"].shape == b["aug_rec"].shape == (4, 9)
            assert b["view_params"].dtype == torch.float64 and b["view_params"].shape == (4, 7)
            seen_sizes |= {(int(h), int(w_)) for _, h, w_ in b["geometry"].tolist()}
            got = packed.device_views(b)
            assert sorted(got) == ["augmented", "clean", "label"]
            for k in ("clean", "augmented", "label"):
                assert got[k].dtype == w[k].dtype and torch.equal(got[k], w[k]), (epoch, k)
    assert len(seen_sizes) == len(SIZES)                       # the batches really mixed sizes
    n = 0
    for b, w in zip(packed_val, classic_val):
        assert sorted(b) == ["clean_rec", "geometry", "label", "pixels"]
        got = packed_val.device_views(b)
        assert sorted(got) == ["label", "pixel_values"]
        assert torch.equal(got["pixel_values"], w["pixel_values"]) and torch.equal(got["label"], w["label"])
        n += 1
    assert n == 3                                              # 9 images: the last batch is a partial one


def test_pack_images_and_host_records():
    from basd_amd.data import DeviceDualView, clean_view_geometry
    from basd_amd.data.device_views import PACK_ALIGN, augment_records, clean_records, pack_images, unpack_image
    sizes = [(40, 56), (64, 48), (33, 71), (50, 50), (5, 7), (37, 91), (71, 33)]
    images = [torch.clamp(C.random_image(h, w, 20 + i), min=1) for i, (h, w) in enumerate(sizes)]    # no zero byte
    pixels, geometry = pack_images(images)
    assert pixels.dtype == torch.uint8 and pixels.dim() == 1
    assert geometry.dtype == torch.int64 and geometry.shape == (len(sizes), 3)
    assert PACK_ALIGN == 16
    covered = torch.zeros(pixels.numel(), dtype=torch.bool)
    prev_end = 0
    for img, (off, h, w) in zip(images, geometry.tolist()):
        assert off % 16 == 0 and off >= prev_end and off - prev_end < 16 and (h, w) == tuple(img.shape[1:])
        assert torch.equal(unpack_image(pixels, (off, h, w)), img)
        covered[off:off + 3 * h * w] = True
        prev_end = off + 3 * h * w
    assert prev_end == pixels.numel()
    assert (~covered).any() and bool((pixels[~covered] == 0).all()) and bool((pixels[covered] != 0).all())
    with pytest.raises(ValueError):
        pack_images([torch.zeros(1, 4, 4, dtype=torch.uint8)])
    with pytest.raises(ValueError):
        pack_images([torch.zeros(3, 4, 4)])

    for size, ratio in ((32, 0.8), (31, 0.9), (32, 1.0), (5, 0.875)):
        rec = clean_records(geometry, size, ratio)
        assert rec.dtype == torch.int32 and rec.shape == (len(sizes), 9)
        for row, (h, w) in zip(rec.tolist(), sizes):
            nh, nw, top, left = clean_view_geometry(h, w, size, ratio)
            assert row == [0, 0, h, w, nh, nw, top, left, 0], (size, ratio, h, w)
    # resize sizes at which int(size * long / short) truncates differently from rounding, and odd differences
    geo = torch.tensor([[0, h, w] for h in range(7, 40, 3) for w in range(5, 60, 7)], dtype=torch.int64)
    rec = clean_records(geo, 3, 0.43)
    for row, (_, h, w) in zip(rec.tolist(), geo.tolist()):
        assert row == [0, 0, h, w, *clean_view_geometry(h, w, 3, 0.43), 0]
    with pytest.raises(ValueError, match="do not pad"):
        clean_records(torch.tensor([[0, 40, 56], [7680, 8, 100]], dtype=torch.int64), 32, 1.25)

    views = DeviceDualView(32, (0.5,) * 3, (0.25,) * 3, *STATS, crop_ratio=0.8)
    vp = torch.stack([views.draw(h, w, torch.Generator().manual_seed(i)) for i, (h, w) in enumerate(sizes)])
    rec = augment_records(vp, 32)
    assert rec.dtype == torch.int32 and torch.equal(rec, views._augment_record(vp))
    for row, p in zip(rec.tolist(), vp.tolist()):
        assert row == [int(p[0]), int(p[1]), int(p[2]), int(p[3]), 32, 32, 0, 0, int(p[4])]
    assert rec[:, 8].any() and not rec[:, 8].all()


def test_npz_root_packed_equals_uniform_device_views(tmp_path):
    from basd_amd.data import create_dataloaders
    cfg = _cfg(_npz_root(tmp_path))
    uniform, uniform_val = create_dataloaders(cfg, teacher_stats=STATS, num_workers=0, device_views=True)
    packed, packed_val = create_dataloaders(cfg, teacher_stats=STATS, num_workers=0, device_views="packed")
    n = 0
    for u, p in zip(uniform, packed):
        assert "image" in u and "pixels" in p and "image" not in p
        want, got = uniform.device_views(u), packed.device_views(p)
        for k in ("clean", "augmented", "label"):
            assert torch.equal(got[k], want[k]), k
        uc, ua = uniform.device_views.resample(u)
        pc, pa = packed.device_views.resample(p)
        assert torch.equal(uc, pc) and torch.equal(ua, pa)
        n += 1
    assert n == 3
    for u, p in zip(uniform_val, packed_val):
        want, got = uniform_val.device_views(u), packed_val.device_views(p)
        assert torch.equal(got["pixel_values"], want["pixel_values"]) and torch.equal(got["label"], want["label"])


def test_unknown_mode_config_key_and_cpu_tensors(tmp_path):
    import basd_amd._native as native
    from basd_amd.data import create_dataloaders, create_eval_loader
    root = _directory_root(tmp_path, n_train=2, n_val=2)
    cfg = _cfg(root)
    for bad in ("pack", "true", "PACKED", ""):
        with pytest.raises(ValueError, match="packed"):
            create_dataloaders(cfg, teacher_stats=STATS, num_workers=0, device_views=bad)
        with pytest.raises(ValueError, match="packed"):
            create_eval_loader(root, image_size=32, batch_size=4, mean=(0.5,) * 3, std=(0.25,) * 3, crop_ratio=0.8,
                               num_workers=0, device_views=bad)
    with pytest.raises(ValueError, match="packed"):
        create_dataloaders(_cfg(root, "data.device_views=pack"), teacher_stats=STATS, num_workers=0)
    train, val = create_dataloaders(_cfg(root, "data.device_views=packed"), teacher_stats=STATS, num_workers=0)
    assert hasattr(train, "device_views") and hasattr(val, "device_views")
    assert "pixels" in next(iter(train)) and "pixels" in next(iter(val))
    train, val = create_dataloaders(_cfg(root, "data.device_views=packed"), teacher_stats=STATS, num_workers=0,
                                    device_views=False)
    assert not hasattr(train, "device_views") and not hasattr(val, "device_views")
    val = create_eval_loader(root, image_size=32, batch_size=4, mean=(0.5,) * 3, std=(0.25,) * 3, crop_ratio=0.8,
                             num_workers=0, device_views="packed")
    assert "pixels" in next(iter(val))
    with pytest.raises(native.BasdNativeError):
        native.resample_u8_packed(torch.zeros(192, dtype=torch.uint8), torch.tensor([[0, 8, 8]], dtype=torch.int64),
                                  torch.zeros(1, 9, dtype=torch.int32), 8)
