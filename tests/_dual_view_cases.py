"""Inputs, cases and CPU oracles shared by the dual-view kernel tests (tests/test_device_views_gpu.py) and the CPU checks
of those cases (tests/test_device_views_cases_cpu.py).  The oracle is data/transforms.py, stage by stage."""
import math

import torch

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
ONE_LEVEL_CAP = 0.01          # share of a case's pixels that may be one uint8 level off the oracle; none may be off by more
BOUNDARY = 1e-3               # affine ops: pixels whose fp64 source coordinate is this close to a rounding boundary are left out
TIE = 1e-9                    # ... unless it sits ON the boundary: see affine_boundary_mask

EXACT_OPS = ("Identity", "Posterize", "Solarize", "Equalize", "TranslateX", "TranslateY")
AFFINE_OPS = ("ShearX", "ShearY", "Rotate")
COLOUR_OPS = ("Brightness", "Color", "Contrast", "Sharpness", "AutoContrast")
SIGNED_OPS = ("ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Brightness", "Color", "Contrast", "Sharpness")


def smooth_image(h: int, w: int, phase: float = 0.0) -> torch.Tensor:
    ys, xs = torch.meshgrid(torch.linspace(-1, 1, h), torch.linspace(-1, 1, w), indexing="ij")
    chans = [127.5 + 120 * torch.sin(3.1 * xs + phase + c) * torch.cos(2.3 * ys - c) for c in range(3)]
    return torch.stack(chans).round().clamp(0, 255).to(torch.uint8)


def random_image(h: int, w: int, seed: int) -> torch.Tensor:
    return torch.randint(0, 256, (3, h, w), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def ta_inputs(s: int) -> torch.Tensor:
    """[4, 3, s, s] uint8: random, smooth, random with a constant channel (AutoContrast's hi == lo and Equalize's
    step == 0), two-valued"""
    const = random_image(s, s, 2)
    const[1] = 93
    two = torch.where(random_image(s, s, 3) > 100, torch.tensor(200, dtype=torch.uint8), torch.tensor(17, dtype=torch.uint8))
    return torch.stack([random_image(s, s, 1), smooth_image(s, s), const, two])


def ta_cases():
    """every op of TA_WIDE_OPS at magnitude bins 0, 15, 30, signed ops at both signs -> [(op id, magnitude)]"""
    from basd_amd.data import transforms as T
    cases = []
    for op_id, op in enumerate(T.TA_WIDE_OPS):
        for bin_ in (0, 15, 30):
            mag = float(T._ta_magnitude(op, bin_))
            cases.append((op_id, mag))
            if op in SIGNED_OPS:
                cases.append((op_id, -mag))
    return cases


def ta_oracle(img: torch.Tensor, op_id: int, mag: float) -> torch.Tensor:
    from basd_amd.data import transforms as T
    return T.apply_ta_op(img, T.TA_WIDE_OPS[op_id], mag)


def normalized(u8: torch.Tensor, mean=MEAN, std=STD) -> torch.Tensor:
    from basd_amd.data import transforms as T
    return T.to_normalized_float(u8, mean, std)


def levels(x: torch.Tensor, mean=MEAN, std=STD) -> torch.Tensor:
    """normalised fp32 [..., 3, S, S] -> the uint8 levels it encodes (int64)"""
    m = torch.tensor(mean, dtype=torch.float64).view(3, 1, 1)
    s = torch.tensor(std, dtype=torch.float64).view(3, 1, 1)
    return ((x.double() * s + m) * 255.0).round().long()


def affine_matrix(op: str, mag: float):
    if op == "ShearX":
        return 1.0, mag, 0.0, 0.0, 1.0, 0.0
    if op == "ShearY":
        return 1.0, 0.0, 0.0, mag, 1.0, 0.0
    t = math.radians(mag)
    return math.cos(t), -math.sin(t), 0.0, math.sin(t), math.cos(t), 0.0


def affine_boundary_mask(s: int, op: str, mag: float) -> torch.Tensor:
    """bool [s, s]: output pixels whose fp64 source coordinate lies within BOUNDARY of a rounding boundary (k + 0.5).
    Exact ties (distance below TIE) are NOT masked: a rotation by +-135 degrees puts both diagonals of an even-sized
    image exactly on a boundary (6.25 % of a 32 x 32 image, far above the 1 % the mask may cover), and there the CPU's
    fp32 arithmetic is exact -- the two products cancel to 0 and 0 + (S - 1) / 2 is representable -- so the kernel has
    to reproduce round-half-even on them like on any other pixel."""
    a, b, c, d, e, f = affine_matrix(op, mag)
    ctr = (s - 1) / 2.0
    ys, xs = torch.meshgrid(torch.arange(s, dtype=torch.float64) - ctr, torch.arange(s, dtype=torch.float64) - ctr,
                            indexing="ij")
    near = torch.zeros(s, s, dtype=torch.bool)
    for coord in (a * xs + b * ys + c + ctr, d * xs + e * ys + f + ctr):
        frac = coord - torch.floor(coord)
        dist = (frac - 0.5).abs()
        near |= (dist <= BOUNDARY) & (dist > TIE)
    return near


def colour_op_fp64(img: torch.Tensor, op: str, mag: float) -> torch.Tensor:
    """fp64 restatement of the colour ops of data/transforms.py (same formulas, exact arithmetic up to fp64)"""
    x = img.double()
    f = 1.0 + mag
    gray = 0.299 * x[0] + 0.587 * x[1] + 0.114 * x[2]
    if op == "Brightness":
        other = torch.zeros_like(x)
    elif op == "Color":
        other = gray.expand_as(x)
    elif op == "Contrast":
        other = gray.mean().expand_as(x)
    elif op == "Sharpness":
        k = torch.tensor([[1.0, 1.0, 1.0], [1.0, 5.0, 1.0], [1.0, 1.0, 1.0]], dtype=torch.float64) / 13.0
        other = x.clone()
        other[:, 1:-1, 1:-1] = torch.nn.functional.conv2d(x.unsqueeze(1), k.view(1, 1, 3, 3)).squeeze(1).round()
    elif op == "AutoContrast":
        lo, hi = x.amin(dim=(1, 2), keepdim=True), x.amax(dim=(1, 2), keepdim=True)
        same = hi == lo
        scale = torch.where(same, torch.ones_like(hi), 255.0 / torch.where(same, torch.ones_like(hi), hi - lo))
        return ((x - torch.where(same, torch.zeros_like(lo), lo)) * scale).clamp(0, 255).floor().to(torch.uint8)
    else:
        raise ValueError(op)
    return (f * x + (1.0 - f) * other).clamp(0, 255).round().to(torch.uint8)


def one_level_report(got: torch.Tensor, want: torch.Tensor, keep: torch.Tensor | None = None):
    """integer images -> (largest difference, share of compared pixels that differ)"""
    diff = (got.long() - want.long()).abs()
    if keep is not None:
        diff = diff[keep.expand_as(diff)]
    return int(diff.max()) if diff.numel() else 0, float((diff != 0).double().mean()) if diff.numel() else 0.0


# ------------------------------------------------------------------------------------------------------ resample cases
def resample_windows(h: int, w: int, s: int):
    """windows (top, left, ch, cw) of an h x w source for output size s: identity size, the whole image (the largest
    downscale the source allows), an upscale from 5 x 7, windows flush against every border, extreme aspects"""
    wins = [(0, 0, h, w), (h - 5, w - 7, 5, 7), (0, 0, h // 2, w // 2), (h - h // 2, w - w // 2, h // 2, w // 2),
            (0, w - 9, h, 9), (h - 4, 0, 4, w), (1, 2, h - 3, w - 5), (3, 1, 7, 5)]
    if h >= s and w >= s:
        wins += [((h - s) // 2, (w - s) // 3, s, s), (h - s, w - s, s, s)]
    return wins


def resample_oracle(img: torch.Tensor, window, s: int, flip: bool) -> torch.Tensor:
    from basd_amd.data import transforms as T
    top, left, ch, cw = window
    x = T.resize(img[:, top:top + ch, left:left + cw], (s, s))
    return T.hflip(x) if flip else x


def augment_records(windows, flips, s: int) -> torch.Tensor:
    return torch.tensor([[*win, s, s, 0, 0, int(fl)] for win, fl in zip(windows, flips)], dtype=torch.int32)
