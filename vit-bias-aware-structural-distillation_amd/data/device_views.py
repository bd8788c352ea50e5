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

``data.device_views: packed`` takes images of DIFFERENT sizes (directory splits).  The collate function packs the
batch's images into one flat uint8 buffer (``pack_images``) and builds both ``[B, 9]`` records on the host
(``clean_records``, ``augment_records``); ``{"pixels", "geometry", "clean_rec", "aug_rec", "view_params", "label"}``
cross PCIe and ``basd_resample_u8_packed`` runs once per view, then the unchanged ``basd_ta_normalize_u8``.
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


PACK_ALIGN = 16             # every image of a packed batch starts at a multiple of this many bytes


def pack_images(images):
    """uint8 ``[3, h_i, w_i]`` images -> (pixels uint8 ``[N]``, geometry int64 ``[B, 3]`` = {offset, h, w}): image i lies
    planar at ``pixels[offset_i : offset_i + 3 h_i w_i]``, every offset is a multiple of ``PACK_ALIGN`` and the bytes
    between two images are zero"""
    geometry = torch.empty(len(images), 3, dtype=torch.int64)
    end = 0
    for i, img in enumerate(images):
        if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[0] != 3 or img.numel() == 0:
            raise ValueError(f"pack_images takes non-empty uint8 [3, h, w] images, got {img.dtype} {tuple(img.shape)}")
        start = -(-end // PACK_ALIGN) * PACK_ALIGN
        geometry[i, 0], geometry[i, 1], geometry[i, 2] = start, img.shape[1], img.shape[2]
        end = start + img.numel()
    pixels = torch.zeros(end, dtype=torch.uint8)
    for img, start in zip(images, geometry[:, 0].tolist()):
        pixels[start:start + img.numel()] = img.reshape(-1)
    return pixels, geometry


def unpack_image(pixels: torch.Tensor, geometry_row) -> torch.Tensor:
    """sample ``geometry_row`` = (offset, h, w) of a packed batch as a ``[3, h, w]`` view of ``pixels``"""
    off, h, w = (int(v) for v in geometry_row)
    return pixels[off:off + 3 * h * w].view(3, h, w)


def clean_records(geometry: torch.Tensor, image_size: int, crop_ratio: float) -> torch.Tensor:
    """int32 ``[B, 9]`` records of the clean view of a packed batch: row i is ``clean_view_geometry(h_i, w_i, ...)``
    with the whole image as the window (vectorised, host side)"""
    s, size = int(image_size), round(int(image_size) / float(crop_ratio))
    h, w = geometry[:, 1], geometry[:, 2]
    long_side = torch.clamp((size * torch.maximum(h, w)).double().div(torch.minimum(h, w).double()).long(), min=1)
    fixed = torch.full_like(h, size)
    nh, nw = torch.where(h <= w, fixed, long_side), torch.where(h <= w, long_side, fixed)
    if bool((nh < s).any()) or bool((nw < s).any()):
        i = int(torch.nonzero((nh < s) | (nw < s))[0])
        clean_view_geometry(int(h[i]), int(w[i]), s, crop_ratio)            # raises, naming the image
    top, left = ((nh - s).double() / 2.0).round().long(), ((nw - s).double() / 2.0).round().long()
    zero = torch.zeros_like(h)
    return torch.stack([zero, zero, h, w, nh, nw, top, left, zero], dim=1).to(torch.int32)


def augment_records(view_params: torch.Tensor, image_size: int) -> torch.Tensor:
    """int32 ``[B, 9]`` records of the augmented view: the window and the flip of ``view_params[:, :5]``, resized to
    ``(S, S)`` at offset 0"""
    s = int(image_size)
    fixed = torch.tensor([s, s, 0, 0], dtype=view_params.dtype, device=view_params.device).expand(view_params.shape[0], 4)
    return torch.cat([view_params[:, :4], fixed, view_params[:, 4:5]], dim=1).to(torch.int32)


def is_packed(batch: dict) -> bool:
    return "pixels" in batch


def _check_packed(batch: dict, image_size: int, train: bool):
    pixels, geometry = batch["pixels"], batch["geometry"]
    b = geometry.shape[0]
    if pixels.dtype != torch.uint8 or pixels.dim() != 1 or geometry.dtype != torch.int64 or geometry.shape != (b, 3):
        raise ValueError(f"a packed batch takes pixels uint8 [N] and geometry int64 [B, 3], got {pixels.dtype} "
                         f"{tuple(pixels.shape)}, {geometry.dtype} {tuple(geometry.shape)}")
    for key in ("clean_rec", "aug_rec") if train else ("clean_rec",):
        rec = batch[key]
        if rec.dtype != torch.int32 or rec.shape != (b, len(RECORD_FIELDS)):
            raise ValueError(f"{key} must be int32 [B, {len(RECORD_FIELDS)}], got {rec.dtype} {tuple(rec.shape)}")
    if train:
        vp = batch["view_params"]
        if vp.shape != (b, len(PARAM_COLUMNS)) or vp.dtype != torch.float64:
            raise ValueError(f"view_params must be float64 [B, {len(PARAM_COLUMNS)}], got {vp.dtype} {tuple(vp.shape)}")
    if pixels.is_cuda:
        from .. import _native as native
        if not native.dual_view_supported(image_size):
            raise ValueError(f"the dual-view kernels do not take image size {image_size}; use the CPU pipeline")


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

    def uint8_packed(self, batch: dict) -> torch.Tensor:
        pixels, geometry = batch["pixels"], batch["geometry"]
        if pixels.is_cuda:
            from .. import _native as native
            return native.resample_u8_packed(pixels.contiguous(), geometry.contiguous(), batch["clean_rec"].contiguous(),
                                             self.image_size)
        return torch.stack([T.center_crop(T.resize(unpack_image(pixels, g), self.resize_size), self.image_size)
                            for g in geometry.tolist()])

    def _normalize(self, u8: torch.Tensor) -> torch.Tensor:
        if u8.is_cuda:
            from .. import _native as native
            return native.ta_normalize_u8(u8, None, None, self.mean, self.std)
        return torch.stack([T.to_normalized_float(x, self.mean, self.std) for x in u8])

    def normalized(self, images: torch.Tensor) -> torch.Tensor:
        return self._normalize(self.uint8(images))


def _check_images(images: torch.Tensor, image_size: int) -> None:
    if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[1] != 3:
        raise ValueError(f"device views take uint8 [B, 3, H, W] batches, got {images.dtype} {tuple(images.shape)}")
    if images.is_cuda:
        from .. import _native as native
        if not native.dual_view_supported(image_size):
            raise ValueError(f"the dual-view kernels do not take image size {image_size}; use the CPU pipeline")


class DeviceEvalView:
    """evaluation batches ``{"image": uint8 [B, 3, H, W], "label"}``, or packed ones ``{"pixels", "geometry",
    "clean_rec", "label"}`` -> ``{"pixel_values", "label"}`` (the arithmetic of ``EvalTransform``) on the batch's
    device"""

    def __init__(self, image_size: int, mean, std, crop_ratio: float):
        self.image_size = int(image_size)
        self._clean = _CleanView(image_size, mean, std, crop_ratio)

    def __call__(self, batch: dict) -> dict:
        if is_packed(batch):
            _check_packed(batch, self.image_size, train=False)
            return {"pixel_values": self._clean._normalize(self._clean.uint8_packed(batch)), "label": batch["label"]}
        images = batch["image"]
        _check_images(images, self.image_size)
        return {"pixel_values": self._clean.normalized(images.contiguous()), "label": batch["label"]}


class DeviceDualView:
    """raw training batches ``{"image": uint8 [B, 3, H, W], "view_params": float64 [B, 7], "label"}`` ->
    ``{"clean", "augmented", "label"}`` fp32 ``[B, 3, S, S]`` on the batch's device (the dict ``Trainer.train_step``
    takes).  The clean view is normalised with the teacher's statistics, the augmented one with the dataset's.
    A packed batch ``{"pixels", "geometry", "clean_rec", "aug_rec", "view_params", "label"}`` (images of different
    sizes, ``pack_images``) gives the same dict."""

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
        return augment_records(vp, self.image_size)

    def _augment_cpu(self, images, vp: torch.Tensor) -> torch.Tensor:
        aug = []
        for img, p in zip(images, vp.tolist()):
            top, left, ch, cw = (int(v) for v in p[:4])
            x = T.resize(img[:, top:top + ch, left:left + cw], (self.image_size, self.image_size))
            aug.append(T.hflip(x) if p[4] else x)
        return torch.stack(aug)

    def _resample_packed(self, batch: dict):
        _check_packed(batch, self.image_size, train=True)
        pixels, geometry = batch["pixels"], batch["geometry"]
        clean = self._clean.uint8_packed(batch)
        if pixels.is_cuda:
            from .. import _native as native
            return clean, native.resample_u8_packed(pixels.contiguous(), geometry.contiguous(),
                                                    batch["aug_rec"].contiguous(), self.image_size)
        return clean, self._augment_cpu([unpack_image(pixels, g) for g in geometry.tolist()], batch["view_params"])

    def resample(self, batch: dict):
        """-> (clean, augmented) uint8 ``[B, 3, S, S]``: the views before the TrivialAugment op and the normalisation"""
        if is_packed(batch):
            return self._resample_packed(batch)
        images, vp = self._inputs(batch)
        clean = self._clean.uint8(images)
        if images.is_cuda:
            from .. import _native as native
            return clean, native.resample_u8(images, self._augment_record(vp), self.image_size)
        return clean, self._augment_cpu(images, vp)

    def __call__(self, batch: dict) -> dict:
        vp = batch["view_params"] if is_packed(batch) else self._inputs(batch)[1]
        clean_u8, aug_u8 = self.resample(batch)
        if clean_u8.is_cuda:
            from .. import _native as native
            clean = native.ta_normalize_u8(clean_u8, None, None, self._clean.mean, self._clean.std)
            aug = native.ta_normalize_u8(aug_u8, vp[:, 5].to(torch.int32), vp[:, 6].contiguous(), self.mean, self.std)
        else:
            clean = torch.stack([T.to_normalized_float(x, self._clean.mean, self._clean.std) for x in clean_u8])
            aug = torch.stack([T.to_normalized_float(T.apply_ta_op(x, T.TA_WIDE_OPS[int(p[5])], p[6]), self.mean, self.std)
                               for x, p in zip(aug_u8, vp.tolist())])
        return {"clean": clean, "augmented": aug, "label": batch["label"]}
