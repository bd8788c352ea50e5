"""Both training views built ON THE DEVICE from one uint8 batch (``data.device_views``, off by default).

The loader workers of the classic pipeline (``datasets._DualView``) build two fp32 ``[3, S, S]`` views per sample with
torch tensor ops on the CPU.  With device views they only fetch the uint8 image and DRAW the augmentation decisions of
sample i from the same ``(seed, epoch, i)`` generator (``draw_augment_params`` consumes it exactly as
``AugmentTransform.__call__`` does); one uint8 ``[B, 3, H, W]`` batch and a ``[B, 7]`` parameter table cross PCIe, and
two kernels (csrc/dual_view.hip) produce ``{"clean", "augmented", "label"}`` on the device:

* ``basd_resample_u8``: window -> antialiased bilinear resize -> offset crop -> flip, uint8 out (both views);
* ``basd_ta_normalize_u8``: the TrivialAugmentWide operation and the normalisation, fp32 out.

A CPU batch takes the torch functions of ``transforms.py`` with the drawn parameters: bit-equal to the classic loader,
and the oracle of the kernels' tests.
"""
from __future__ import annotations

import torch

from . import transforms as T

# columns of the per-sample parameter table (float64: the magnitudes are the doubles apply_ta_op is called with)
PARAM_COLUMNS = ("top", "left", "ch", "cw", "flip", "op", "magnitude")
_SIGNED_OPS = ("ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Brightness", "Color", "Contrast", "Sharpness")
# int32 record of basd_resample_u8 (include/basd_hip.h)
RECORD_FIELDS = ("top", "left", "h", "w", "nh", "nw", "off_y", "off_x", "flip")


def draw_augment_params(h: int, w: int, image_size: int, gen):
    """The random decisions of ``AugmentTransform(image_size)(img [3, h, w], gen)``, drawn from ``gen`` in the same
    order (RandomResizedCrop attempts, flip, op index, magnitude bin, sign of signed ops) ->
    ((top, left, ch, cw), flip, op id into TA_WIDE_OPS, signed magnitude).  ``image_size`` does not enter the draws."""
    window = T.random_resized_crop_params(h, w, gen)
    flip = T._rand(gen) < 0.5
    op_id = T._randint(gen, len(T.TA_WIDE_OPS))
    op = T.TA_WIDE_OPS[op_id]
    mag = T._ta_magnitude(op, T._randint(gen, T._TA_BINS))
    if op in _SIGNED_OPS and T._randint(gen, 2):
        mag = -mag
    return tuple(int(v) for v in window), bool(flip), op_id, float(mag)


def apply_augment_params(img: torch.Tensor, image_size: int, window, flip: bool, op_id: int, mag: float) -> torch.Tensor:
    """the uint8 augmented view of ``img`` for drawn parameters (the stages of ``AugmentTransform`` before the
    normalisation)"""
    top, left, ch, cw = window
    x = T.resize(img[:, top:top + ch, left:left + cw], (image_size, image_size))
    if flip:
        x = T.hflip(x)
    return T.apply_ta_op(x, T.TA_WIDE_OPS[op_id], mag)


def clean_view_geometry(h: int, w: int, image_size: int, crop_ratio: float):
    """``center_crop(resize(img [3, h, w], round(image_size / crop_ratio)), image_size)`` as numbers: the resized size
    (nh, nw) by ``resize(int)``'s rule and the crop offset (top, left) by ``center_crop``'s.  The zero-padding case of
    ``center_crop`` (a resized side below ``image_size``) is not supported."""
    size = round(image_size / crop_ratio)
    if h <= w:
        nh, nw = size, max(1, int(size * w / h))
    else:
        nh, nw = max(1, int(size * h / w)), size
    if nh < image_size or nw < image_size:
        raise ValueError(f"device views do not pad: a {h} x {w} image resizes to {nh} x {nw}, smaller than the "
                         f"{image_size} px crop (crop ratio {crop_ratio}); use the CPU pipeline (device_views=False)")
    return nh, nw, int(round((nh - image_size) / 2.0)), int(round((nw - image_size) / 2.0))


def _check_no_padding(image_size: int, crop_ratio: float) -> None:
    if not crop_ratio > 0 or crop_ratio > 1 or round(image_size / crop_ratio) < image_size:
        raise ValueError(f"device views do not support crop ratio {crop_ratio} (the centre crop would zero-pad the "
                         "resized image); use the CPU pipeline (device_views=False)")


class _CleanView:
    """resize -> centre crop (-> normalise) of a uniform uint8 batch; the records of the device path are cached per
    batch geometry (no host-to-device copy in the steady state)"""

    def __init__(self, image_size: int, mean, std, crop_ratio: float):
        _check_no_padding(int(image_size), float(crop_ratio))
        self.image_size, self.crop_ratio = int(image_size), float(crop_ratio)
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        self.resize_size = round(self.image_size / self.crop_ratio)
        self._records: dict = {}

    def record(self, b: int, h: int, w: int, device) -> torch.Tensor:
        key = (b, h, w, str(device))
        rec = self._records.get(key)
        if rec is None:
            nh, nw, top, left = clean_view_geometry(h, w, self.image_size, self.crop_ratio)
            if len(self._records) > 8:
                self._records.clear()
            rec = self._records[key] = torch.tensor([[0, 0, h, w, nh, nw, top, left, 0]] * b, dtype=torch.int32,
                                                    device=device)
        return rec

    def uint8(self, images: torch.Tensor) -> torch.Tensor:
        b, _, h, w = images.shape
        if images.is_cuda:
            from .. import _native as native
            return native.resample_u8(images, self.record(b, h, w, images.device), self.image_size)
        clean_view_geometry(h, w, self.image_size, self.crop_ratio)
        return torch.stack([T.center_crop(T.resize(img, self.resize_size), self.image_size) for img in images])

    def normalized(self, images: torch.Tensor) -> torch.Tensor:
        u8 = self.uint8(images)
        if u8.is_cuda:
            from .. import _native as native
            return native.ta_normalize_u8(u8, None, None, self.mean, self.std)
        return torch.stack([T.to_normalized_float(x, self.mean, self.std) for x in u8])


def _check_images(images: torch.Tensor, image_size: int) -> None:
    if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[1] != 3:
        raise ValueError(f"device views take uint8 [B, 3, H, W] batches, got {images.dtype} {tuple(images.shape)}")
    if images.is_cuda:
        from .. import _native as native
        if not native.dual_view_supported(image_size):
            raise ValueError(f"the dual-view kernels do not take image size {image_size}; use the CPU pipeline")


class DeviceEvalView:
    """evaluation batches ``{"image": uint8 [B, 3, H, W], "label"}`` -> ``{"pixel_values", "label"}`` (the arithmetic
    of ``EvalTransform``) on the batch's device"""

    def __init__(self, image_size: int, mean, std, crop_ratio: float):
        self.image_size = int(image_size)
        self._clean = _CleanView(image_size, mean, std, crop_ratio)

    def __call__(self, batch: dict) -> dict:
        images = batch["image"]
        _check_images(images, self.image_size)
        return {"pixel_values": self._clean.normalized(images.contiguous()), "label": batch["label"]}


class DeviceDualView:
    """raw training batches ``{"image": uint8 [B, 3, H, W], "view_params": float64 [B, 7], "label"}`` ->
    ``{"clean", "augmented", "label"}`` fp32 ``[B, 3, S, S]`` on the batch's device (the dict ``Trainer.train_step``
    takes).  The clean view is normalised with the teacher's statistics, the augmented one with the dataset's."""

    def __init__(self, image_size: int, mean, std, teacher_mean, teacher_std, crop_ratio: float):
        self.image_size = int(image_size)
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        self._clean = _CleanView(image_size, teacher_mean, teacher_std, crop_ratio)
        self.crop_ratio = self._clean.crop_ratio

    # ------------------------------------------------------------------ loader workers (host)
    def draw(self, h: int, w: int, gen) -> torch.Tensor:
        """one row of ``view_params`` for an ``h x w`` image"""
        window, flip, op_id, mag = draw_augment_params(h, w, self.image_size, gen)
        return torch.tensor([*window, int(flip), op_id, mag], dtype=torch.float64)

    # ------------------------------------------------------------------ batch side
    def _inputs(self, batch: dict):
        images, vp = batch["image"], batch["view_params"]
        _check_images(images, self.image_size)
        if vp.dim() != 2 or vp.shape != (images.shape[0], len(PARAM_COLUMNS)) or vp.dtype != torch.float64:
            raise ValueError(f"view_params must be float64 [B, {len(PARAM_COLUMNS)}], got {vp.dtype} {tuple(vp.shape)}")
        return images.contiguous(), vp

    def _augment_record(self, vp: torch.Tensor) -> torch.Tensor:
        s = self.image_size
        fixed = torch.tensor([s, s, 0, 0], dtype=vp.dtype, device=vp.device).expand(vp.shape[0], 4)
        return torch.cat([vp[:, :4], fixed, vp[:, 4:5]], dim=1).to(torch.int32)

    def resample(self, batch: dict):
        """-> (clean, augmented) uint8 ``[B, 3, S, S]``: the views before the TrivialAugment op and the normalisation"""
        images, vp = self._inputs(batch)
        clean = self._clean.uint8(images)
        if images.is_cuda:
            from .. import _native as native
            return clean, native.resample_u8(images, self._augment_record(vp), self.image_size)
        aug = []
        for img, p in zip(images, vp.tolist()):
            top, left, ch, cw = (int(v) for v in p[:4])
            x = T.resize(img[:, top:top + ch, left:left + cw], (self.image_size, self.image_size))
            aug.append(T.hflip(x) if p[4] else x)
        return clean, torch.stack(aug)

    def __call__(self, batch: dict) -> dict:
        images, vp = self._inputs(batch)
        clean_u8, aug_u8 = self.resample(batch)
        if images.is_cuda:
            from .. import _native as native
            clean = native.ta_normalize_u8(clean_u8, None, None, self._clean.mean, self._clean.std)
            aug = native.ta_normalize_u8(aug_u8, vp[:, 5].to(torch.int32), vp[:, 6].contiguous(), self.mean, self.std)
        else:
            clean = torch.stack([T.to_normalized_float(x, self._clean.mean, self._clean.std) for x in clean_u8])
            aug = torch.stack([T.to_normalized_float(T.apply_ta_op(x, T.TA_WIDE_OPS[int(p[5])], p[6]), self.mean, self.std)
                               for x, p in zip(aug_u8, vp.tolist())])
        return {"clean": clean, "augmented": aug, "label": batch["label"]}
