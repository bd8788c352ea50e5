"""basd_resample_u8_packed (csrc/dual_view.hip): samples of different sizes in one flat uint8 buffer.

Two expectations for every case (one case = one record on one sample):
(a) bit-equal to basd_resample_u8 on that sample alone, as a B = 1 uniform batch with the same record;
(b) against the CPU oracle (data/transforms.py through tests/_dual_view_cases.py): no pixel more than one uint8 level
    off and at most ONE_LEVEL_CAP of the case's pixels one level off -- the cap of tests/test_device_views_gpu.py.
Geometry that does not lie inside the buffer must give zeros without a read: the buffer of that test is a slice from the
middle of a larger allocation filled with a sentinel, so a wrong kernel reads sentinel bytes and fails the comparison
instead of leaving the allocation."""
import pytest
import torch

from tests import _dual_view_cases as C

pytestmark = pytest.mark.gpu

MIXED_SIZES = ((40, 56), (64, 48), (16, 200), (37, 91), (9, 300), (5, 7))


def _image(h, w, i):
    return C.random_image(h, w, 40 + i) if i % 2 == 0 else C.smooth_image(h, w, 0.3 * i)


def _fits(win, h, w):
    top, left, ch, cw = win
    return top >= 0 and left >= 0 and ch >= 1 and cw >= 1 and top + ch <= h and left + cw <= w


def _alone(img, rec_row, s):
    """the uniform entry on one sample: a B = 1 batch"""
    import basd_amd._native as native
    return native.resample_u8(img[None].contiguous().cuda(), rec_row[None].contiguous().cuda(), s)[0].cpu()


def _packed(images, sample_of, rec, s):
    """images packed once; record i runs on sample sample_of[i] (rows of the geometry table may share a sample)"""
    import basd_amd._native as native
    from basd_amd.data.device_views import pack_images
    pixels, geometry = pack_images(images)
    got = native.resample_u8_packed(pixels.cuda(), geometry[sample_of].contiguous().cuda(), rec.cuda(), s)
    assert got.dtype == torch.uint8 and got.shape == (len(sample_of), 3, s, s) and got.is_cuda
    return got.cpu()


def _check_one_level(got, want, what, exact=False):
    worst, share = C.one_level_report(got, want)
    print(f"{what}: max {worst}, share {100 * share:.4f} %")
    if exact:
        assert worst == 0, (what, worst, share)
    assert worst <= 1 and share <= C.ONE_LEVEL_CAP, (what, worst, share)


def _check_windows(images, sample_of, windows, flips, s):
    rec = C.augment_records(windows, flips, s)
    got = _packed(images, sample_of, rec, s)
    for i, (k, win, fl) in enumerate(zip(sample_of, windows, flips)):
        img = images[k]
        what = f"{tuple(img.shape[1:])} -> {s} window {win} flip {fl}"
        assert torch.equal(got[i], _alone(img, rec[i], s)), what                                   # (a)
        _check_one_level(got[i], C.resample_oracle(img, win, s, fl), what, exact=win[2:] == (s, s))   # (b)


@pytest.mark.parametrize("s", [32, 31, 12, 3])
def test_mixed_batch(s):
    images = [_image(h, w, i) for i, (h, w) in enumerate(MIXED_SIZES)]
    sample_of, windows = [], []
    for k, (h, w) in enumerate(MIXED_SIZES):
        wins = [(0, 0, h, w)] + [win for win in C.resample_windows(h, w, s)[1:] if _fits(win, h, w)]
        sample_of += [k] * len(wins)
        windows += wins
    assert set(sample_of) == set(range(len(MIXED_SIZES))) and len(windows) > 3 * len(MIXED_SIZES)
    flips = [i % 3 == 1 for i in range(len(windows))]
    _check_windows(images, sample_of, windows, flips, s)


def _band_sizes():
    import basd_amd._native as native
    r = native.PACKED_BAND_ROWS
    return [r - 1, r, r + 1]


@pytest.mark.parametrize("hw,sizes", [((256, 256), [32]), ((5, 7), [32]), ((64, 48), [33, "band"])])
def test_filter_widths_and_band_edges(hw, sizes):
    """256 -> 32: scale 8, sixteen taps per axis (more than the eight the tables hold); 5 x 7 -> 32: an upscale;
    64 x 48 -> 33 and band height - 1, band height, band height + 1: the last, partial band.  B = 1."""
    img = _image(*hw, 1 if hw == (256, 256) else 2)
    for s in [v for size in sizes for v in (_band_sizes() if size == "band" else [size])]:
        for flip in (False, True):
            _check_windows([img], [0], [(0, 0, *hw)], [flip], s)


def test_workload_geometry_224():
    """B = 2, S = 224 from 256 x 256 and 375 x 500: the clean records at crop ratio 0.875 and drawn augment records"""
    from basd_amd.data import DeviceDualView
    from basd_amd.data import transforms as T
    from basd_amd.data.device_views import augment_records, clean_records, pack_images
    images = [C.random_image(256, 256, 9), C.smooth_image(375, 500)]
    _, geometry = pack_images(images)
    views = DeviceDualView(224, C.MEAN, C.STD, C.MEAN, C.STD, crop_ratio=0.875)
    rec_clean = clean_records(geometry, 224, 0.875)
    got = _packed(images, [0, 1], rec_clean, 224)
    for i, img in enumerate(images):
        assert torch.equal(got[i], _alone(img, rec_clean[i], 224)), i
        _check_one_level(got[i], T.center_crop(T.resize(img, 256), 224), f"clean 224 image {i}", exact=i == 0)
    vp = torch.stack([views.draw(img.shape[1], img.shape[2], torch.Generator().manual_seed(3 + i))
                      for i, img in enumerate(images)])
    vp[0, 4], vp[1, 4] = 1.0, 0.0
    rec_aug = augment_records(vp, 224)
    got = _packed(images, [0, 1], rec_aug, 224)
    for i, img in enumerate(images):
        win = tuple(int(v) for v in vp[i, :4])
        assert torch.equal(got[i], _alone(img, rec_aug[i], 224)), i
        _check_one_level(got[i], C.resample_oracle(img, win, 224, bool(vp[i, 4])), f"augmented 224 window {win}")


def test_bad_geometry_reads_nothing_and_bad_records_are_clamped():
    import basd_amd._native as native
    from basd_amd.data.device_views import pack_images
    s, sentinel, margin = 32, 0xA5, 1 << 21
    images = [_image(40, 56, 0), _image(64, 48, 1), _image(37, 91, 2)]
    pixels, geometry = pack_images(images)
    n = pixels.numel() - 1                                    # the last image overruns pixels_bytes by ONE byte
    big = torch.full((2 * margin + pixels.numel(),), sentinel, dtype=torch.uint8).cuda()
    big[margin:margin + pixels.numel()] = pixels.cuda()
    view = big[margin:margin + n]                             # numel() = n is what the wrapper passes as pixels_bytes
    assert view.numel() == n and view.data_ptr() == big.data_ptr() + margin
    g = geometry.tolist()
    geo = torch.tensor([g[0],                                 # valid
                        g[2],                                 # ends one byte behind pixels_bytes
                        g[1],                                 # valid
                        [g[1][0], 0, 48],                     # h = 0
                        [-16, 40, 56],                        # negative offset (sentinel bytes lie there)
                        [n + 16, 40, 56],                     # starts behind pixels_bytes (sentinel bytes lie there)
                        [g[0][0], 40, 16385],                 # w above 16384
                        g[0]], dtype=torch.int64)             # valid again
    assert n + 16 + 3 * 40 * 56 < margin + n and g[0][0] + 3 * 40 * 16385 < margin + n       # all inside `big`
    whole = [[0, 0, h, w, s, s, 0, 0, i % 2] for i, (_, h, w) in enumerate(geo.tolist())]
    rec = torch.tensor(whole, dtype=torch.int32)
    got = native.resample_u8_packed(view, geo.cuda(), rec.cuda(), s).cpu()
    valid = {0: images[0], 2: images[1], 7: images[0]}
    for i in range(len(geo)):
        if i in valid:
            assert torch.equal(got[i], _alone(valid[i], rec[i], s)), i
            _check_one_level(got[i], C.resample_oracle(valid[i], tuple(whole[i][:4]), s, bool(whole[i][8])), f"valid {i}")
        else:
            assert int(got[i].max()) == 0, (i, geo[i].tolist(), int(got[i].max()))
    # records out of range, on valid geometry: clamped like the uniform entry clamps them
    bad = torch.tensor([[30, 50, 40, 56, 32, 32, 0, 0, 0],          # window past the bottom right corner
                        [-5, -7, 20, 20, 32, 32, 0, 0, 1],          # negative corner
                        [100, 100, 0, -3, 32, 32, 0, 0, 0],         # corner outside, empty window
                        [0, 0, 40, 56, 0, -1, 0, 0, 0],             # resized size below 1
                        [0, 0, 40, 56, 52, 72, -9, 60, 7],          # offsets outside the resized image, flip = 7
                        [2, 3, 30, 40, 40, 40, 20, 20, 1]], dtype=torch.int32)
    geo = torch.tensor([g[0]] * len(bad), dtype=torch.int64)
    got = native.resample_u8_packed(view, geo.cuda(), bad.cuda(), s).cpu()
    for i in range(len(bad)):
        assert torch.equal(got[i], _alone(images[0], bad[i], s)), bad[i].tolist()
    _check_one_level(got[0], C.resample_oracle(images[0], (30, 50, 10, 6), s, False), "cut window")
    assert bool((big[:margin] == sentinel).all()) and bool((big[margin + pixels.numel():] == sentinel).all())


def test_status_codes():
    import basd_amd._native as native
    L = native.lib()
    buf = torch.zeros(4096, dtype=torch.uint8).cuda()
    geo, rec = torch.tensor([[0, 8, 8]]).cuda(), torch.zeros(1, 9, dtype=torch.int32).cuda()
    out = torch.zeros(3 * 32 * 32, dtype=torch.uint8).cuda()
    p = native._ptr

    def args(**kw):
        return [kw.get("pixels", p(buf)), kw.get("n", 4096), kw.get("geo", p(geo)), kw.get("rec", p(rec)),
                kw.get("b", 1), kw.get("s", 32), kw.get("out", p(out)), native._stream()]

    assert L.basd_resample_u8_packed(*args()) == 0
    assert L.basd_resample_u8_packed(*args(b=0)) == 0
    for kw in (dict(s=2), dict(s=1025), dict(b=-1), dict(pixels=None), dict(geo=None), dict(rec=None), dict(out=None),
               dict(n=-1), dict(out=out.data_ptr() + 1)):
        assert L.basd_resample_u8_packed(*args(**kw)) != 0, kw
    torch.cuda.synchronize()


def test_device_views_on_a_packed_batch_against_the_cpu_fallback():
    """a packed batch through DeviceDualView.__call__ / .resample and DeviceEvalView on the device, against the CPU
    fallback of the same batch, in uint8 levels.  Rotate by 90 degrees maps pixel centres onto pixel centres exactly
    in fp32 (no source coordinate near a rounding boundary), and the Contrast factors are below 1, so a one-level
    difference of the resample stays one level behind the operation."""
    from basd_amd.data import DeviceDualView
    from basd_amd.data import transforms as T
    from basd_amd.data.device_views import DeviceEvalView, augment_records, clean_records, pack_images
    sizes = ((40, 56), (64, 48), (33, 71), (50, 50), (37, 91), (16, 200), (71, 33), (5, 7))
    mean, std, ratio = (0.41, 0.52, 0.47), (0.21, 0.26, 0.24), 32 / 52
    views = DeviceDualView(32, mean, std, C.MEAN, C.STD, crop_ratio=ratio)
    images = [_image(h, w, i) for i, (h, w) in enumerate(sizes)]
    pixels, geometry = pack_images(images)
    vp = torch.stack([views.draw(h, w, torch.Generator().manual_seed(100 + i)) for i, (h, w) in enumerate(sizes)])
    ops = ["Identity", "Rotate", "Contrast", "Equalize", "Rotate", "Contrast", "Equalize", "Identity"]
    mags = [0.0, 90.0, -0.33, 0.0, -90.0, -0.66, 0.0, 0.0]
    vp[:, 5] = torch.tensor([T.TA_WIDE_OPS.index(o) for o in ops], dtype=torch.float64)
    vp[:, 6] = torch.tensor(mags, dtype=torch.float64)
    label = torch.arange(len(sizes), dtype=torch.int64)
    batch = {"pixels": pixels, "geometry": geometry, "clean_rec": clean_records(geometry, 32, ratio),
             "aug_rec": augment_records(vp, 32), "view_params": vp, "label": label}
    on_gpu = {k: v.cuda() for k, v in batch.items()}
    want, got = views(batch), views(on_gpu)
    assert sorted(got) == ["augmented", "clean", "label"] and torch.equal(got["label"].cpu(), label)
    for k in ("clean", "augmented"):
        assert got[k].dtype == torch.float32 and got[k].shape == (len(sizes), 3, 32, 32) and got[k].is_cuda
    for i in range(len(sizes)):
        _check_one_level(C.levels(got["clean"][i].cpu()), C.levels(want["clean"][i]), f"clean view {i}")
        _check_one_level(C.levels(got["augmented"][i].cpu(), mean, std), C.levels(want["augmented"][i], mean, std),
                         f"augmented view {i} {ops[i]}")
    u8c, u8a = views.resample(on_gpu)
    wc, wa = views.resample(batch)
    for i in range(len(sizes)):
        _check_one_level(u8c[i].cpu(), wc[i], f"clean uint8 {i}")
        _check_one_level(u8a[i].cpu(), wa[i], f"augmented uint8 {i}")
    torch.testing.assert_close(got["clean"].cpu(), C.normalized(u8c.cpu()), atol=1e-6, rtol=1e-6)
    ev = DeviceEvalView(32, mean, std, ratio)
    eval_batch = {k: batch[k] for k in ("pixels", "geometry", "clean_rec", "label")}
    want_e, got_e = ev(eval_batch), ev({k: v.cuda() for k, v in eval_batch.items()})
    assert sorted(got_e) == ["label", "pixel_values"] and got_e["pixel_values"].is_cuda
    for i in range(len(sizes)):
        _check_one_level(C.levels(got_e["pixel_values"][i].cpu(), mean, std), C.levels(want_e["pixel_values"][i], mean, std),
                         f"evaluation view {i}")
