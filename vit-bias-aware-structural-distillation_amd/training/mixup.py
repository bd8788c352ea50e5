"""On-device RandomChoice([MixUp(alpha=1), CutMix(alpha=1)]) producing soft targets
(reference src/training/trainer.py:89-92,138 uses torchvision.transforms.v2, which is not
installed here).  RNG dependent, hence outside the parity boundary.

The draws are made on the host (``_draw``).  A contiguous fp32 / bf16 batch on the device is then blended, pasted and
given its soft targets by ONE kernel launch (``basd_mixup_cutmix``, csrc/mixup.hip); everything else (CPU tensors,
other dtypes, non-contiguous input) takes the torch chain below, which the kernel restates operation by operation."""
from __future__ import annotations

import torch

from .. import _native

MIXUP, CUTMIX = 0, 1


def _draw(h: int, w: int, generator=None):
    """The host-side draws of one call -> (mode, lam, box): lam is the blend weight (MixUp) or the box-area-corrected
    weight of the targets (CutMix); box = (y0, y1, x0, x1), half-open and clipped, None for MixUp."""
    lam = float(torch.distributions.Beta(1.0, 1.0).sample())
    if float(torch.rand((), generator=generator)) < 0.5:          # MixUp: lam * x_i + (1 - lam) * x_{i-1}
        return MIXUP, lam, None
    r = (1.0 - lam) ** 0.5                                         # CutMix
    ch, cw = int(h * r), int(w * r)
    cy = int(torch.randint(h, (1,), generator=generator))
    cx = int(torch.randint(w, (1,), generator=generator))
    y0, y1 = max(cy - ch // 2, 0), min(cy + ch // 2, h)
    x0, x1 = max(cx - cw // 2, 0), min(cx + cw // 2, w)
    return CUTMIX, 1.0 - (y1 - y0) * (x1 - x0) / float(h * w), (y0, y1, x0, x1)


def _kernel_takes(images, targets, num_classes, out, out_targets) -> bool:
    if not (images.is_cuda and _native.mixup_supported(images)):
        return False
    if not (targets.is_cuda and targets.dtype == torch.int64 and targets.shape == images.shape[:1] and targets.is_contiguous()):
        return False
    if out is not None and not (out.is_cuda and out.shape == images.shape and out.dtype == images.dtype and out.is_contiguous()):
        return False
    return out_targets is None or (out_targets.is_cuda and out_targets.shape == (images.shape[0], num_classes)
                                   and out_targets.dtype == torch.float32 and out_targets.is_contiguous())


def mixup_cutmix(images: torch.Tensor, targets: torch.Tensor, num_classes: int, generator=None,
                 out: torch.Tensor | None = None, out_targets: torch.Tensor | None = None):
    """Partner of sample i is sample i - 1 (a roll by one, as torchvision's v2 transforms do).  The rolled batch is never
    materialised: the blend / the pasted box reads the two shifted slices of ``images`` directly and writes ``out``
    (e.g. the static input buffer of the captured step) in one pass.  Returns (mixed images, soft targets)."""
    mode, lam, box = _draw(images.shape[-2], images.shape[-1], generator)
    if _kernel_takes(images, targets, num_classes, out, out_targets):
        if out is None:
            out = torch.empty_like(images)
        if out_targets is None:
            out_targets = torch.empty(images.shape[0], num_classes, dtype=torch.float32, device=images.device)
        return _native.mixup_cutmix(images, targets, num_classes, mode, lam, box or (0, 0, 0, 0), out, out_targets)
    return _torch_chain(images, targets, num_classes, mode, lam, box, out, out_targets)


def _torch_chain(images, targets, num_classes, mode, lam, box, out=None, out_targets=None):
    if out is None:
        out = torch.empty_like(images)
    if mode == MIXUP:
        torch.lerp(images[:-1], images[1:], lam, out=out[1:])
        torch.lerp(images[-1:], images[:1], lam, out=out[:1])
    else:
        y0, y1, x0, x1 = box
        out.copy_(images)
        out[1:, ..., y0:y1, x0:x1] = images[:-1, ..., y0:y1, x0:x1]
        out[:1, ..., y0:y1, x0:x1] = images[-1:, ..., y0:y1, x0:x1]
    onehot = torch.nn.functional.one_hot(targets, num_classes).float()
    if out_targets is None:
        out_targets = torch.empty_like(onehot)
    torch.lerp(onehot.roll(1, 0), onehot, lam, out=out_targets)
    return out, out_targets
