"""The input pipeline's two ways of building the dual views, side by side:

* the CPU pipeline (data/transforms.py in the loader workers): both views per sample, one thread, no decoding ->
  images / s per worker;
* the device pipeline (csrc/dual_view.hip): basd_resample_u8 (clean + augmented) and basd_ta_normalize_u8 (clean +
  augmented) per 256-image uint8 batch -> device-event medians and the achieved bytes / s (algorithmic traffic: uint8
  source read once per view, uint8 intermediate written and read, fp32 views written).

    python scripts/time_input_pipeline.py [--batch 256] [--iters 30] [--cpu-samples 64] [--skip-cpu]

One JSON line per configuration (32 px from 32 x 32 sources, 224 px from 256 x 256 sources).

    python scripts/time_input_pipeline.py --packed [--batch 256] [--iters 30] [--rounds 5]

basd_resample_u8_packed instead: (1) the uniform 256 x 256 -> 224 batch in packed form against basd_resample_u8 on the
same records, both views, the two entries timed alternately in one process (``rounds`` medians each, and the spread of
the old entry's medians); (2) one synthetic ImageNet-like batch (fixed seed, short side 333 .. 500, aspect up to 4:3),
new entry only, with the achieved bytes / s."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def median_ms(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def cpu_images_per_second(src: int, size: int, ratio: float, samples: int) -> float:
    from basd_amd.data import transforms as T
    torch.set_num_threads(1)
    g = torch.Generator().manual_seed(0)
    imgs = torch.randint(0, 256, (samples, 3, src, src), generator=g, dtype=torch.uint8)
    clean, aug = T.EvalTransform(size, mean=MEAN, std=STD, crop_ratio=ratio), T.AugmentTransform(size, mean=MEAN, std=STD)
    t0 = time.perf_counter()
    for i, img in enumerate(imgs):
        clean(img)
        aug(img, torch.Generator().manual_seed(i))
    return samples / (time.perf_counter() - t0)


def packed_ab(args):
    import random

    import basd_amd._native as native
    from basd_amd.data import DeviceDualView
    from basd_amd.data.device_views import augment_records, clean_records, pack_images
    b, size, ratio = args.batch, 224, 0.875
    views = DeviceDualView(size, MEAN, STD, MEAN, STD, crop_ratio=ratio)

    def prepare(images):
        pixels, geometry = pack_images(images)
        vp = torch.stack([views.draw(im.shape[1], im.shape[2], torch.Generator().manual_seed(i))
                          for i, im in enumerate(images)])
        dev = [t.cuda() for t in (pixels, geometry, clean_records(geometry, size, ratio), augment_records(vp, size))]

        def run():
            return (native.resample_u8_packed(dev[0], dev[1], dev[2], size),
                    native.resample_u8_packed(dev[0], dev[1], dev[3], size))
        return dev, run

    g = torch.Generator().manual_seed(1)
    uniform = torch.randint(0, 256, (b, 3, 256, 256), generator=g, dtype=torch.uint8)
    dev, new = prepare(list(uniform))
    images = uniform.cuda()

    def old():
        return native.resample_u8(images, dev[2], size), native.resample_u8(images, dev[3], size)

    equal = all(torch.equal(x, y) for x, y in zip(old(), new()))
    t_old, t_new = [], []
    for _ in range(args.rounds):
        t_old.append(median_ms(old, args.iters))
        t_new.append(median_ms(new, args.iters))
    traffic = 2 * uniform.numel() + 2 * b * 3 * size * size
    print(json.dumps({"case": "uniform 256x256 -> 224, both views", "batch": b, "bit_equal": equal,
                      "resample_u8_ms": [round(t, 4) for t in t_old],
                      "resample_u8_packed_ms": [round(t, 4) for t in t_new],
                      "old_median_ms": round(statistics.median(t_old), 4),
                      "old_spread_ms": round(max(t_old) - min(t_old), 4),
                      "new_median_ms": round(statistics.median(t_new), 4),
                      "new_GBps": round(traffic / statistics.median(t_new) / 1e6, 1)}), flush=True)

    rng = random.Random(0)
    mixed = []
    for i in range(b):
        short = rng.randint(333, 500)
        long_side = int(short * rng.uniform(1.0, 4.0 / 3.0))
        h, w = (short, long_side) if rng.random() < 0.5 else (long_side, short)
        mixed.append(torch.randint(0, 256, (3, h, w), generator=g, dtype=torch.uint8))
    dev, new = prepare(mixed)
    t_mixed = [median_ms(new, args.iters) for _ in range(args.rounds)]
    traffic = 2 * dev[0].numel() + 2 * b * 3 * size * size
    print(json.dumps({"case": "mixed sizes (short side 333 .. 500, aspect <= 4:3) -> 224, both views", "batch": b,
                      "packed_bytes": dev[0].numel(), "pcie_bytes_packed": dev[0].numel() + b * (3 * 8 + 2 * 36 + 7 * 8 + 8),
                      "pcie_bytes_fp32_views": 8 * b * 3 * size * size,
                      "resample_u8_packed_ms": [round(t, 4) for t in t_mixed],
                      "median_ms": round(statistics.median(t_mixed), 4),
                      "GBps": round(traffic / statistics.median(t_mixed) / 1e6, 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--cpu-samples", type=int, default=64)
    ap.add_argument("--skip-cpu", action="store_true")
    ap.add_argument("--packed", action="store_true", help="time basd_resample_u8_packed against basd_resample_u8")
    ap.add_argument("--rounds", type=int, default=5, help="--packed: medians per entry, taken alternately")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_input_pipeline.py needs the GPU for the kernel side")
    if args.packed:
        return packed_ab(args)
    import basd_amd._native as native
    from basd_amd.data import DeviceDualView
    b = args.batch
    for src, size, ratio in ((32, 32, 32 / 40), (256, 224, 0.875)):
        views = DeviceDualView(size, MEAN, STD, MEAN, STD, crop_ratio=ratio)
        g = torch.Generator().manual_seed(1)
        images = torch.randint(0, 256, (b, 3, src, src), generator=g, dtype=torch.uint8)
        vp = torch.stack([views.draw(src, src, torch.Generator().manual_seed(i)) for i in range(b)])
        batch = {"image": images.cuda(), "view_params": vp.cuda(), "label": torch.zeros(b, dtype=torch.int64).cuda()}
        rec_clean = views._clean.record(b, src, src, images.cuda().device)
        rec_aug = views._augment_record(batch["view_params"])
        ops, mags = batch["view_params"][:, 5].to(torch.int32), batch["view_params"][:, 6].contiguous()
        u8c, u8a = views.resample(batch)

        def resample():
            native.resample_u8(batch["image"], rec_clean, size)
            native.resample_u8(batch["image"], rec_aug, size)

        def ta_normalize():
            native.ta_normalize_u8(u8c, None, None, MEAN, STD)
            native.ta_normalize_u8(u8a, ops, mags, MEAN, STD)

        t_res, t_ta, t_all = (median_ms(f, args.iters) for f in (resample, ta_normalize, lambda: views(batch)))
        u8_out = 2 * b * 3 * size * size
        bytes_res = 2 * b * 3 * src * src + u8_out                 # upper bound of the source reads: the whole image per view
        bytes_ta = u8_out + 4 * u8_out
        out = {"source": src, "image_size": size, "batch": b, "resample_ms": round(t_res, 4),
               "ta_normalize_ms": round(t_ta, 4), "device_dual_view_ms": round(t_all, 4),
               "resample_GBps": round(bytes_res / t_res / 1e6, 1), "ta_normalize_GBps": round(bytes_ta / t_ta / 1e6, 1),
               "pcie_bytes_uint8": b * 3 * src * src + vp.numel() * 8, "pcie_bytes_fp32_views": 8 * b * 3 * size * size}
        if not args.skip_cpu:
            out["cpu_images_per_s_per_worker"] = round(cpu_images_per_second(src, size, ratio, args.cpu_samples), 1)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
